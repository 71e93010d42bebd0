// Host-only test of csrc/popmem.h: what the population handle's setters replace, and the
// step's streams, over a counting heap that can be told to fail the N-th allocation.  No HIP
// runtime, no GPU.  Built with -fsanitize=address,undefined by tests/test_hostmem_cpu.py; the
// exit status is the failed checks plus the live allocations at exit plus the double frees.
#define FQ_HOSTMEM_NO_HIP
#include "../../flow-q-learning_amd/csrc/popmem.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

namespace {

// hostmem_test.cpp's heap, which also notes how many allocations were live at each request
struct Heap {
    static inline std::set<void*> live;
    static inline std::vector<size_t> live_at_request;
    static inline long allocs = 0, releases = 0, double_frees = 0;
    static inline long fail_at = 0;  // the fail_at-th allocation from now fails (0: none)
    using event_t = void*;
    using stream_t = void*;
    static const char* get(void** p, size_t bytes) {
        live_at_request.push_back(live.size());
        if (fail_at && --fail_at == 0) return "out of memory (injected)";
        *p = std::malloc(bytes ? bytes : 1);
        live.insert(*p);
        ++allocs;
        return nullptr;
    }
    static void put(void* p) {
        ++releases;
        if (!live.erase(p)) { ++double_frees; return; }
        std::free(p);
    }
    static const char* alloc(void** p, size_t bytes) { return get(p, bytes); }
    static void free(void* p) { put(p); }
    static const char* host_alloc(void** p, size_t bytes, unsigned) { return get(p, bytes); }
    static void host_free(void* p) { put(p); }
    static const char* event_create(event_t* e, unsigned) { return get(e, 1); }
    static void event_destroy(event_t e) { put(e); }
    static const char* stream_create(stream_t* s) { return get(s, 1); }
    static void stream_destroy(stream_t s) { put(s); }
};

int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// stand-ins for the kernel-argument structs the env-model structs keep
struct Layout {
    int dims[3] = {};
    const float* sp = nullptr;
};
struct ModelNet {
    const float *sp, *tp;
};

constexpr int D = 3, A = 2, kCtr = 4, kStage = 4;
using Dataset = fq::PopDataset<Heap>;
using Workspace = fq::PopCollectWs<Heap>;
using Stage = fq::PopStartStage<kStage, Heap>;
using EnvModel = fq::PopEnvModel<Layout, Heap>;
using Ensemble = fq::PopEnvModelEnsemble<Layout, ModelNet, Heap>;
using Rings = fq::PopSynthRings<Heap>;
using Streams = fq::StepStreams<Heap>;

// runs f with the n-th allocation failing; true if it threw the owner's error
template <class F>
bool fails_at(int n, F&& f) {
    Heap::fail_at = n;
    try {
        f();
    } catch (const fq::Err& e) {
        CHECK(e.code == FQLPOP_E_HIP && Heap::fail_at == 0);
        return true;
    }
    Heap::fail_at = 0;
    return false;
}

// A replace_released target: `n_allocs` allocations per build; `empty` tests the documented
// empty state.  After a failure at any N: empty, and nothing of the old or the half-built live.
template <class T, class Make, class Empty>
void released_case(const char* name, int n_allocs, Make make, Empty empty) {
    T t;
    CHECK(empty(t));
    for (int n = 1; n <= n_allocs; ++n) {
        fq::replace_released(t, [&] { return make(10); });
        CHECK(!empty(t) && (int)Heap::live.size() == n_allocs);
        CHECK(fails_at(n, [&] { fq::replace_released(t, [&] { return make(20); }); }));
        CHECK(empty(t) && Heap::live.empty());
    }
    // the order of a successful replacement: the old value is released before the first new allocation
    fq::replace_released(t, [&] { return make(10); });
    Heap::live_at_request.clear();
    fq::replace_released(t, [&] { return make(20); });
    CHECK(Heap::live_at_request.front() == 0 && (int)Heap::live.size() == n_allocs && !empty(t));
    t = T{};
    CHECK(Heap::live.empty() && Heap::double_frees == 0);
    std::printf("  %s: %d allocations per build\n", name, n_allocs);
}

// A built-aside target: `same(t, snapshot)` tests that t still holds the snapshot's pointers
// and sizes.  After a failure at any N: unchanged, and only its allocations are live.
template <class T, class Make, class Snap, class Same>
void built_case(const char* name, int n_allocs, Make make, Snap snap, Same same) {
    T t;
    fq::replace_built(t, [&] { return make(10); });
    const auto old = snap(t);
    for (int n = 1; n <= n_allocs; ++n) {
        CHECK(fails_at(n, [&] { fq::replace_built(t, [&] { return make(20); }); }));
        CHECK(same(t, old) && (int)Heap::live.size() == n_allocs);
    }
    // a successful replacement releases the old value only after the new one exists
    Heap::live_at_request.clear();
    const long r0 = Heap::releases;
    fq::replace_built(t, [&] { return make(20); });
    CHECK((int)Heap::live_at_request.front() == n_allocs && (int)Heap::live_at_request.back() == 2 * n_allocs - 1);
    CHECK(!same(t, old) && (int)Heap::live.size() == n_allocs && Heap::releases == r0 + n_allocs);
    t = T{};
    CHECK(Heap::live.empty() && Heap::double_frees == 0);
    std::printf("  %s: %d allocations per build\n", name, n_allocs);
}

void test_released() {
    released_case<Dataset>(
        "dataset", 5, [](long long rows) { return Dataset::make(rows, D, A); },
        [](const Dataset& d) { return d.rows == 0 && !d.obs && !d.act && !d.rew && !d.mask && !d.nobs; });
    released_case<Workspace>(
        "collect workspace", 1, [](long long n) { return Workspace::make(n); },
        [](const Workspace& w) { return w.floats == 0 && !w.buf; });
    released_case<Stage>(
        "start-row stage", kStage, [](long long n) { return Stage::make(n, 0u); }, [](const Stage& s) {
            bool none = s.cap == 0;
            for (int i = 0; i < kStage; ++i) none = none && !s.host[i] && !s.used[i];
            return none;
        });
    Stage s = Stage::make(7, 0u);  // a growth forgets the readers of the buffers that went
    s.used[2] = true;
    fq::replace_released(s, [] { return Stage::make(9, 0u); });
    CHECK(s.cap == 9 && !s.used[2]);
}

void test_built() {
    Layout lay;
    lay.dims[1] = 16;
    fqlpop_envmodel_config cfg{};
    cfg.obs_dim = D;
    struct EmSnap { const float *sp, *tp; int dim, obs; };
    built_case<EnvModel>(
        "env model", 2,
        [&](long long n) {
            Layout l = lay;
            l.dims[1] = (int)n;
            return EnvModel::make(l, cfg, n * 3, n);
        },
        [](const EnvModel& m) { return EmSnap{m.sp, m.tp, m.args.dims[1], m.cfg.obs_dim}; },
        [](const EnvModel& m, const EmSnap& o) {
            return bool(m) && m.sp.get() == o.sp && m.tp.get() == o.tp && m.args.dims[1] == o.dim && m.cfg.obs_dim == o.obs;
        });
    CHECK(!EnvModel{});

    struct EnsSnap { const float *sp, *tp; const ModelNet* nets; int n, dim; };
    built_case<Ensemble>(
        "env-model ensemble", 3,
        [&](long long n) {
            Layout l = lay;
            l.dims[1] = (int)n;
            Ensemble e = Ensemble::make(l, (int)n / 5, n * 3, n);
            // the per-model pointers are taken before the move into the target: moving keeps them
            e.nets[0] = ModelNet{e.sp, e.tp};
            return e;
        },
        [](const Ensemble& e) { return EnsSnap{e.sp, e.tp, e.nets, e.n, e.args.dims[1]}; },
        [](const Ensemble& e, const EnsSnap& o) {
            return e.sp.get() == o.sp && e.tp.get() == o.tp && e.nets.get() == o.nets && e.n == o.n &&
                   e.args.dims[1] == o.dim && e.nets[0].sp == o.sp && e.nets[0].tp == o.tp;
        });
    CHECK(Ensemble{}.n == 0);

    struct RingSnap { const float *obs, *act, *rew, *mask, *nobs; const long long* ctr; long long cap; };
    built_case<Rings>(
        "synthetic-transition rings", 6, [](long long cap) { return Rings::make(2, cap, D, A, kCtr); },
        [](const Rings& r) { return RingSnap{r.obs, r.act, r.rew, r.mask, r.nobs, r.ctr, r.cap}; },
        [](const Rings& r, const RingSnap& o) {
            return r.obs.get() == o.obs && r.act.get() == o.act && r.rew.get() == o.rew && r.mask.get() == o.mask &&
                   r.nobs.get() == o.nobs && r.ctr.get() == o.ctr && r.cap == o.cap;
        });
    // the rings report a failed allocation as a whole: members x rows and their bytes
    Heap::fail_at = 3;
    CHECK(fq::guard([] { Rings::make(2, 50, D, A, kCtr); }) == FQLPOP_E_HIP);
    const std::string want = "synthetic-transition rings: allocating " + std::to_string(4 * 2 * 50 * (2 * D + A + 2)) +
                             " bytes (2 members x 50 rows) failed";
    CHECK(fq::g_last_error == want);
    CHECK(Rings{}.cap == 0 && !Rings{}.obs && Heap::live.empty());
}

void test_streams() {
    const long r0 = Heap::releases;
    {
        Streams one;  // the step on one stream: three views of the main stream, one owner
        one.make_streams(1);
        CHECK(one.sM && one.sF == one.sM && one.sB == one.sM && one.sX == one.sM && Heap::live.size() == 1);
    }
    CHECK(Heap::live.empty() && Heap::releases == r0 + 1 && Heap::double_frees == 0);
    {
        Streams four;
        four.make_streams(4);
        const std::set<void*> distinct = {four.sM, four.sF, four.sB, four.sX};
        CHECK(distinct.size() == 4 && Heap::live == distinct);
    }
    CHECK(Heap::live.empty() && Heap::releases == r0 + 5 && Heap::double_frees == 0);
    for (int n = 1; n <= 4; ++n) {
        CHECK(fails_at(n, [] {
            Streams s;
            s.make_streams(4);
        }));
        CHECK(Heap::live.empty());
    }
}

}  // namespace

int main() {
    test_released();
    test_built();
    test_streams();
    std::printf("popmem_test: %d failed checks, %zu live allocations, %ld allocations, %ld double frees\n", failures,
                Heap::live.size(), Heap::allocs, Heap::double_frees);
    return failures + (int)Heap::live.size() + (int)Heap::double_frees;
}
