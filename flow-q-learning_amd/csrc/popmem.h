// What the setters of the population handle (struct fqlpop, runtime.cpp) replace, each as one
// struct of owners and sizes whose default-constructed value is the handle's documented empty
// state, and the step's streams.  Owners only, as emboot.h: tests/cpp/popmem_test.cpp (and
// rowstage_test.cpp for PopRowStage) runs them on the host over a counting heap.  The kernel-argument structs of kernels.h that two of
// them keep (the env-model leaf layout) are template parameters, so that the test needs no HIP.
#pragma once

#include "hostmem.h"

namespace fq {

// fqlpop_set_dataset, by replace_released (the arrays are large).  Empty: no rows.
template <class BE = DefaultBackend>
struct PopDataset {
    DevBuf<float, BE> obs, act, rew, mask, nobs;
    long long rows = 0;

    static PopDataset make(long long rows, int D, int A) {
        PopDataset d;
        d.obs = DevBuf<float, BE>((size_t)rows * D, "dataset observations");
        d.act = DevBuf<float, BE>((size_t)rows * A, "dataset actions");
        d.rew = DevBuf<float, BE>((size_t)rows, "dataset rewards");
        d.mask = DevBuf<float, BE>((size_t)rows, "dataset masks");
        d.nobs = DevBuf<float, BE>((size_t)rows * D, "dataset next observations");
        d.rows = rows;
        return d;
    }
};

// fqlpop_set_env_model, by replace_built.  Empty (false): no model set.
template <class Layout, class BE = DefaultBackend>
struct PopEnvModel {
    DevBuf<float, BE> sp, tp;         // the two predictors' flat parameters
    Layout args{};                    // the leaf layout (pointers unset: rollout_args fills them)
    fqlpop_envmodel_config cfg{};

    explicit operator bool() const { return sp.get() != nullptr; }

    static PopEnvModel make(const Layout& layout, const fqlpop_envmodel_config& cfg, long long n_sp, long long n_tp) {
        PopEnvModel m;
        m.sp = DevBuf<float, BE>((size_t)n_sp, "env-model state predictor");
        m.tp = DevBuf<float, BE>((size_t)n_tp, "env-model termination predictor");
        m.args = layout;
        m.cfg = cfg;
        return m;
    }
};

// fqlpop_set_env_model_ensemble, by replace_built.  Empty: n == 0.
template <class Layout, class ModelNet, class BE = DefaultBackend>
struct PopEnvModelEnsemble {
    DevBuf<float, BE> sp, tp;         // [n][n_sp], [n][n_tp]
    DevBuf<ModelNet, BE> nets;        // device [n]: the layout with model k's pointers
    Layout args{};                    // the shared leaf layout
    int n = 0;

    static PopEnvModelEnsemble make(const Layout& layout, int n_models, long long n_sp, long long n_tp) {
        PopEnvModelEnsemble e;
        e.sp = DevBuf<float, BE>((size_t)n_sp * n_models, "env-model ensemble state predictors");
        e.tp = DevBuf<float, BE>((size_t)n_tp * n_models, "env-model ensemble termination predictors");
        e.nets = DevBuf<ModelNet, BE>((size_t)n_models, "env-model ensemble table");
        e.args = layout;
        e.n = n_models;
        return e;
    }
};

// fqlpop_synth_create: built aside and moved in.  Empty: cap == 0, no rings.
template <class BE = DefaultBackend>
struct PopSynthRings {
    DevBuf<float, BE> obs, act, rew, mask, nobs;  // [slots][cap] rows of D, A, 1, 1, D floats
    DevBuf<long long, BE> ctr;                    // [slots][n_ctr]
    long long cap = 0;

    // a failed allocation reports the rings as a whole: members x rows and their bytes
    static PopSynthRings make(long long slots, long long cap, int D, int A, int n_ctr) {
        try {
            PopSynthRings r;
            const size_t rows = (size_t)slots * cap;
            r.obs = DevBuf<float, BE>(rows * D);
            r.act = DevBuf<float, BE>(rows * A);
            r.rew = DevBuf<float, BE>(rows);
            r.mask = DevBuf<float, BE>(rows);
            r.nobs = DevBuf<float, BE>(rows * D);
            r.ctr = DevBuf<long long, BE>((size_t)slots * n_ctr);
            r.cap = cap;
            return r;
        } catch (const Err& e) {
            const unsigned long long bytes = sizeof(float) * (unsigned long long)slots * cap * (2ULL * D + A + 2);
            throw Err{e.code, "synthetic-transition rings: allocating " + std::to_string(bytes) + " bytes (" +
                                  std::to_string(slots) + " members x " + std::to_string(cap) + " rows) failed"};
        }
    }
};

// The collect workspace, grown on demand by replace_released.  Empty: capacity 0.
template <class BE = DefaultBackend>
struct PopCollectWs {
    DevBuf<float, BE> buf;
    long long floats = 0;

    static PopCollectWs make(long long floats) {
        PopCollectWs w;
        w.buf = DevBuf<float, BE>((size_t)floats, "collect workspace");
        w.floats = floats;
        return w;
    }
};

// The start rows of the collects in flight: N mapped host buffers used in turn, grown on demand
// by replace_released.  Empty: capacity 0, none in use.
template <int N, class BE = DefaultBackend>
struct PopStartStage {
    HostBuf<long long, BE> host[N];
    bool used[N] = {};  // buffer i has a reader to wait for (the handle's event i)
    long long cap = 0;

    static PopStartStage make(long long cap, unsigned flags) {
        PopStartStage s;
        for (auto& hb : s.host) hb = HostBuf<long long, BE>((size_t)cap, flags, "collect start rows");
        s.cap = cap;
        return s;
    }
};

// The host rows of the ring writes in flight (fqlpop_synth_write, fqlpop_synth_append): N mapped
// host buffers used in turn, each one call's rows field after field (obs, act, rew, mask,
// next_obs), grown on demand by replace_released.  Empty: no rows, none in use.
template <int N, class BE = DefaultBackend>
struct PopRowStage {
    HostBuf<float, BE> host[N];
    bool used[N] = {};  // buffer i has a reader to wait for (the handle's event i)
    long long rows = 0;
    int D = 0, A = 0;

    static PopRowStage make(long long rows, int D, int A, unsigned flags) {
        PopRowStage s;
        for (auto& hb : s.host) hb = HostBuf<float, BE>((size_t)rows * width(D, A), flags, "ring row stage");
        s.rows = rows;
        s.D = D;
        s.A = A;
        return s;
    }
    static long long width(int D, int A) { return 2LL * D + A + 2; }  // floats per row
    // where field f (0 obs, 1 act, 2 rew, 3 mask, 4 next_obs) of an n-row call starts, in floats
    long long field(int f, long long n) const {
        const long long before[5] = {0, D, D + A, D + A + 1, D + A + 2};
        return before[f] * n;
    }
    long long field_width(int f) const { return f == 0 || f == 4 ? D : f == 1 ? A : 1; }
};

// The staging of fqlpop_act: one pinned host buffer and one device buffer of the same layout,
// for `cols` = active members x envs columns, grown on demand by replace_released.  A call of
// n <= cols columns uses the inputs [obs n x D | noise n x A] from float 0 (one copy up) and
// the outputs [actions n x A | noise used n x A] from float out_off() (one copy down).
// Empty: no columns.  (Host test: tests/cpp/actstage_test.cpp.)
template <class BE = DefaultBackend>
struct PopActStage {
    HostBuf<float, BE> host;
    DevBuf<float, BE> dev;
    long long cols = 0;
    int D = 0, A = 0;

    static PopActStage make(long long cols, int D, int A, unsigned flags) {
        PopActStage s;
        s.host = HostBuf<float, BE>((size_t)cols * (D + 3 * A), flags, "act stage (host)");
        s.dev = DevBuf<float, BE>((size_t)cols * (D + 3 * A), "act stage (device)");
        s.cols = cols;
        s.D = D;
        s.A = A;
        return s;
    }
    long long out_off() const { return cols * (D + A); }
};

// The streams of a population step: the main one and three side streams, which are streams of
// their own or, when the step runs on one stream, views of the main one.  One owner per
// stream: the views own nothing.
template <class BE = DefaultBackend>
struct StepStreams {
    using stream_t = typename BE::stream_t;
    stream_t sM{}, sF{}, sB{}, sX{};  // views (sX: the small-population schedule's 4th stream)

    void make_streams(int n_streams) {
        main_ = Stream<BE>::create();
        sM = sF = sB = sX = main_;
        if (n_streams == 1) return;
        stream_t* view[3] = {&sF, &sB, &sX};
        for (int i = 0; i < 3; ++i) {
            side_[i] = Stream<BE>::create();
            *view[i] = side_[i];
        }
    }

   private:
    Stream<BE> main_, side_[3];
};

}  // namespace fq
