// Host-only test of csrc/emlayout.h: the plan fqlpop_emtrain_create makes (em_plan) and the
// layouts the env-model kernels address with, over the shapes tests/test_emtrain_cpu.py lists.
// No HIP runtime, no GPU; built with -fsanitize=address,undefined by that test.
//
//   emlayout_test <shapes.txt> <plans.bin>
//
// shapes.txt, one item per line (all integers but tw):
//   shape kind D A nh h.. ntp t.. tw T B option      (kind: FQLPOP_EM_*)
//   grid T B nobs obs.. nact act.. nw w.. ntp {len t..}..
//     the shapes (obs, act, hid, tph, tw) for act, for n in 1..3, for hid in w^n (the last width
//     fastest), for (tw 0 without a frozen predictor, then tw 1 with each of the ntp), for obs
// plans.bin: per shape, in order, FIELDS int32: refused (em_plan_try's text; the rest 0), lds_bytes,
// sweep, sweep_lds, tchunks, blocks, seq_stride, nin, rec_floats, sweep_need.
// For every admitted shape the layouts are checked here: regions contiguous from 0 to total, the
// sweep's LDS within a CU's beside the static arrays, the record ending at its stride and its
// loaded part within SW_RQ floats per thread.  Exit status: the number of failed checks.
#define FQ_HOSTMEM_NO_HIP
#include "../../flow-q-learning_amd/csrc/emlayout.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace fq::em;

namespace {

int failures = 0;
bool bad_input = false;  // shapes.txt does not parse: the walk stops
#define CHECK(c)                                                                                  \
    do {                                                                                          \
        if (!(c)) {                                                                               \
            if (failures < 20) std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            ++failures;                                                                           \
        }                                                                                         \
    } while (0)

constexpr int FIELDS = 10;
long shapes = 0, admitted = 0, refused = 0;

// plans.bin, written in blocks of records
struct Out {
    FILE* f;
    size_t n = 0;
    int32_t buf[FIELDS * 8192];
    void put(const int32_t* rec) {
        for (int i = 0; i < FIELDS; ++i) buf[n++] = rec[i];
        if (n == sizeof(buf) / sizeof(buf[0])) flush();
    }
    void flush() {
        if (std::fwrite(buf, sizeof(int32_t), n, f) != n) ++failures;
        n = 0;
    }
};

// a cursor over consecutive regions: each starts where the one before ended
struct Walk {
    int at = 0;
    bool ok = true;
    void region(int off, int width) {
        ok = ok && off == at && width >= 0;
        at = off + width;
    }
};

void check_layouts(const EmPlan& p, int D, bool ms) {
    const Net &n = p.net, &t = p.tpn;
    const int K0 = n.dims[0];
    int maxd = 0;
    for (int i = 0; i <= n.n; ++i) maxd = std::max(maxd, n.dims[i]);
    for (int i = 0; i <= t.n; ++i) maxd = std::max(maxd, t.dims[i]);
    for (int sweep = 0; sweep <= (p.sweep ? 1 : 0); ++sweep) {
        const EmLds l = em_lds(n, t, D, ms, sweep != 0);
        Walk w;
        w.region(l.x0, K0 * R);
        w.region(l.xhat, K0 * R);
        for (int i = 0; i <= n.n; ++i) w.region(em_acts(l, n, i), n.dims[i] * R);
        w.region(l.gA, maxd * R);
        w.region(l.gB, maxd * R);
        w.region(l.gC, maxd * R);
        w.region(l.nobs, D * R);
        if (t.n > 0)
            for (int i = 0; i <= t.n; ++i) w.region(em_tacts(l, t, i), t.dims[i] * R);
        else
            w.region(l.tacts0, ms ? D * R : 0);  // pred (a single step without the frozen predictor: none)
        w.region(l.carry, ms ? D * R : 0);
        if (sweep) {
            w.region(l.scr, SW_SCR);
            w.region(l.lnacc, 2 * K0);
            w.region(l.lnp, 2 * K0);
        }
        CHECK(w.ok && w.at == l.total);
        CHECK(4LL * l.total == (sweep ? p.sweep_need : p.lds_bytes));
        if (sweep) CHECK(4LL * l.total + SW_STATIC_LDS <= CU_LDS_BYTES);
        else CHECK(4LL * l.total <= EM_LDS_BUDGET && 4LL * l.total + SW_STATIC_LDS <= CU_LDS_BYTES);
    }
    if (!ms) {
        CHECK(!p.sweep && p.seq_stride == 0 && p.sweep_need == 0 && p.tchunks == 1);
        return;
    }
    const EmRec r = em_rec(n, D, p.sweep);
    Walk w;
    w.region(r.xhat, K0 * R);
    w.region(r.rstd, R);
    for (int i = 0; i < n.n; ++i) w.region(em_rec_acts(r, n, i), n.dims[i] * R);
    w.region(r.own, D * R);
    CHECK(w.ok && w.at == r.g0 && r.g0 == p.rec_floats);
    if (p.sweep) {
        for (int i = n.n - 1; i >= 0; --i) w.region(em_rec_g(r, n, i), n.dims[i + 1] * R);
        CHECK(r.g0 <= SW_RQ * SW_NT && p.nin <= SW_NT);
        // every op of the sweep's programs, both directions: one unit per wave, SW_FM fragments
        for (const Net* q : {&n, &t})
            for (int i = 0; i < q->n; ++i)
                for (int dir = 0; dir < 2; ++dir) {
                    int ntile, S, cks;
                    sw_plan(q->dims[i + dir], q->dims[i + 1 - dir], ntile, S, cks);
                    CHECK(ntile * S <= SW_NW && cks <= SW_FM);
                }
    }
    CHECK(w.ok && w.at == r.stride && r.stride == p.seq_stride);
}

// a config of everything but the observation width
fqlpop_emtrain_config config(int kind, int A, const std::vector<int>& hid, const std::vector<int>& tph, float tw, int T,
                             int B) {
    fqlpop_emtrain_config c{};
    c.kind = kind;
    c.action_dim = A;
    c.num_hidden = (int)hid.size();
    for (size_t i = 0; i < hid.size(); ++i) c.hidden_dims[i] = hid[i];
    c.tp_num_hidden = (int)tph.size();
    for (size_t i = 0; i < tph.size(); ++i) c.tp_hidden_dims[i] = tph[i];
    c.batch_size = B;
    c.steps = 100;
    c.termination_weight = tw;
    c.sequence_length = T;
    c.episode_length = 1000;
    return c;
}

void run_shape(fqlpop_emtrain_config& c, int D, int option, Out& out) {
    c.obs_dim = D;
    int32_t f[FIELDS] = {0};
    ++shapes;
    EmPlan p;
    if (!em_plan_try(&c, option != 0, -1, 1, &p)) {
        const int32_t g[FIELDS] = {0, p.lds_bytes, p.sweep ? 1 : 0, p.sweep_lds, p.tchunks, p.blocks,
                                   (int32_t)p.seq_stride, p.nin, p.rec_floats, (int32_t)p.sweep_need};
        for (int i = 0; i < FIELDS; ++i) f[i] = g[i];
        CHECK(p.seq_stride < (1LL << 31) && p.sweep_need < (1LL << 31));
        check_layouts(p, D, c.kind == FQLPOP_EM_MULTISTEP);
        admitted += p.sweep ? 1 : 0;
    } else {
        f[0] = 1;
        ++refused;
    }
    out.put(f);
}

std::vector<int> read_list(FILE* in) {
    int n = 0;
    if (std::fscanf(in, "%d", &n) != 1 || n < 0 || n > 4096) {
        bad_input = true;
        return {};
    }
    std::vector<int> v((size_t)n);
    for (int& x : v)
        if (std::fscanf(in, "%d", &x) != 1) bad_input = true;
    return v;
}

void run_grid(FILE* in, Out& out) {
    int T = 0, B = 0;
    if (std::fscanf(in, "%d %d", &T, &B) != 2) bad_input = true;
    const std::vector<int> obs = read_list(in), act = read_list(in), w = read_list(in);
    int ntp = 0;
    if (std::fscanf(in, "%d", &ntp) != 1) bad_input = true;
    std::vector<std::vector<int>> tps;
    for (int i = 0; i < ntp; ++i) tps.push_back(read_list(in));
    if (bad_input || w.empty()) return;
    for (int A : act)
        for (int n = 1; n <= 3; ++n) {
            std::vector<size_t> ix((size_t)n, 0);
            for (bool more = true; more;) {
                std::vector<int> hid;
                for (size_t i : ix) hid.push_back(w[i]);
                fqlpop_emtrain_config c = config(FQLPOP_EM_MULTISTEP, A, hid, {}, 0.f, T, B);
                for (int D : obs) run_shape(c, D, 1, out);
                for (const auto& tp : tps) {
                    c = config(FQLPOP_EM_MULTISTEP, A, hid, tp, 1.f, T, B);
                    for (int D : obs) run_shape(c, D, 1, out);
                }
                int k = n - 1;  // the next index tuple, the last position fastest
                while (k >= 0 && ++ix[(size_t)k] == w.size()) ix[(size_t)k--] = 0;
                more = k >= 0;
            }
        }
}

// the VAE pair at a few shapes: regions contiguous, totals as the widths add up
void check_vae() {
    const int shapes_[][5] = {{3, 2, 1, 20, 0}, {17, 5, 2, 50, 36}, {42, 8, 2, 96, 48}, {4096, 64, 2, 512, 512}};
    for (const auto& s : shapes_) {
        const int D = s[0], L = s[1], nh = s[2];
        VaeDense enc[VMAXH]{}, dec[VMAXH + 1]{};
        int k = L, sumh = 0, maxd = std::max(D, L);
        for (int i = 0; i < nh; ++i) {
            dec[i].K = k;
            dec[i].N = k = s[3 + nh - 1 - i];
            sumh += k;
            maxd = std::max(maxd, k);
        }
        dec[nh].K = k;
        dec[nh].N = D;
        k = D;
        for (int i = 0; i < nh; ++i) {
            enc[i].K = k;
            enc[i].N = k = s[3 + i];
        }
        const VaeLds l = vae_lds(enc, dec, nh, D, L, maxd);
        Walk w;
        w.region(l.x, D * R);
        for (int i = 1; i <= nh; ++i) w.region(vae_hidden(l.e1, enc, i), enc[i - 1].N * R);
        for (int o : {l.mu, l.lv, l.eps, l.z}) w.region(o, L * R);
        for (int i = 1; i <= nh; ++i) w.region(vae_hidden(l.d1, dec, i), dec[i - 1].N * R);
        w.region(l.xhat, D * R);
        w.region(l.gmu, L * R);
        w.region(l.glv, L * R);
        w.region(l.gA, maxd * R);
        w.region(l.gB, maxd * R);
        CHECK(w.ok && w.at == l.total && l.total == R * (2 * D + 2 * sumh + 6 * L + 2 * maxd));
        const VaeDecLds d = vae_dec_lds(dec, nh, L);
        Walk v;
        v.region(d.z, L * R);
        for (int i = 1; i <= nh + 1; ++i) v.region(vae_hidden(d.d1, dec, i), dec[i - 1].N * R);
        CHECK(v.ok && v.at == d.total && d.total == R * (L + sumh + D));
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::printf("usage: %s shapes.txt plans.bin\n", argv[0]);
        return 2;
    }
    FILE* in = std::fopen(argv[1], "r");
    if (!in) return 2;
    FILE* of = std::fopen(argv[2], "wb");
    if (!of) return 2;
    static Out out;
    out.f = of;
    char word[16];
    while (std::fscanf(in, "%15s", word) == 1 && !bad_input) {
        if (word[0] == 'g') {
            run_grid(in, out);
            continue;
        }
        int kind = 0, D = 0, A = 0, T = 0, B = 0, option = 0;
        float tw = 0.f;
        if (std::fscanf(in, "%d %d %d", &kind, &D, &A) != 3) bad_input = true;
        const std::vector<int> hid = read_list(in), tph = read_list(in);
        if (std::fscanf(in, "%f %d %d %d", &tw, &T, &B, &option) != 4) bad_input = true;
        if (!bad_input) {
            fqlpop_emtrain_config c = config(kind, A, hid, tph, tw, T, B);
            run_shape(c, D, option, out);
        }
    }
    std::fclose(in);
    if (bad_input) ++failures;
    check_vae();
    out.flush();
    if (std::fclose(of) != 0) ++failures;
    std::printf("%ld shapes, %ld on the sweep path, %ld refused, %d failed checks\n", shapes, admitted, refused, failures);
    return failures > 255 ? 255 : failures;
}
