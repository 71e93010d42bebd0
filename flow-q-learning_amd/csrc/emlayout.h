// The env-model trainers' layouts (emtrain.hip), each written once: the kernels address with
// these functions and the host sizes with them, so a shape cannot be admitted with a size the
// kernels do not use.
//   em_lds      the dynamic LDS of em_grad_kernel, em_seq_grad_kernel and em_sweep_kernel
//   em_rec      the per-(block, step) record of the multistep store (both sequence kernels,
//               em_seq_dw_kernel, the store's size)
//   sw_plan     the unit split of a sweep op (sw_load, sw_compute, the admission rule)
//   em_plan     everything fqlpop_emtrain_create decides before its first GPU call
//   vae_lds, vae_dec_lds   the dynamic LDS of em_vae_grad_kernel / em_vae_decode_kernel
// Pure integer arithmetic with no GPU call and no HIP type: tests/cpp/emlayout_test.cpp
// defines FQ_HOSTMEM_NO_HIP and runs the plan over a grid of shapes with a plain host compiler.
// All offsets and totals are in floats unless a name says bytes.
#pragma once

#include <algorithm>

#include "hostmem.h"

#ifdef __HIPCC__
#define EM_HD __host__ __device__ __forceinline__
#else
#define EM_HD inline
#endif

namespace fq {
namespace em {

constexpr int R = 16;      // minibatch rows per block
constexpr int NT = 512;    // threads per block
constexpr int MAXL = 8;    // Dense layers per net
constexpr int NLOG = 16;   // per-block log sums

// The sweep path (em_sweep_kernel): threads and waves per block, A fragments per wave and op,
// the split-K scratch [SW_NW][16][R], and the floats per thread of a step's record loaded a
// step ahead
constexpr int SW_NT = 1024, SW_NW = SW_NT / 64, SW_FM = 32, SW_SCR = SW_NW * 16 * R;
constexpr int SW_RQ = 10;
constexpr int EM_PH_N = 32;  // diagnostic phase slots (FQ_DIAG)
// em_sweep_kernel's static LDS: the __shared__ arrays it declares (the diagnostic build's ph
// too), pinned there by a static_assert; em_seq_grad_kernel declares the same ones but ph.  A
// CU's LDS holds them beside the dynamic part.
#ifdef FQ_DIAG
constexpr int SW_PH_LDS = (int)sizeof(unsigned long long[EM_PH_N]);
#else
constexpr int SW_PH_LDS = 0;
#endif
constexpr int SW_STATIC_LDS = (int)(sizeof(float[NLOG][R]) + sizeof(float[R]) + sizeof(long long[R]) +
                                    2 * sizeof(float[R]) + sizeof(float[2][R])) + SW_PH_LDS;
constexpr int CU_LDS_BYTES = 160 * 1024;
constexpr int EM_LDS_BUDGET = 150 * 1024;  // dynamic LDS of the fused step (em_grad_kernel, em_seq_grad_kernel)

struct Net {
    int n;                              // Dense layers (hidden + output)
    int dims[MAXL + 1];                 // dims[0] = input, dims[n] = output
    long long w[MAXL], b[MAXL];         // flat offsets (flax leaf order)
    long long ln_scale, ln_bias;        // state predictor LayerNorm_0 (-1: none)

    // flax leaf order (path-sorted): Dense_i/bias, Dense_i/kernel ..., LayerNorm_0/bias, LayerNorm_0/scale
    static Net layout(int in, int nh, const int* hid, int out, bool ln, long long* total) {
        Net n{};
        n.n = nh + 1;
        ARGCHK(n.n <= MAXL, "too many layers");
        n.dims[0] = in;
        for (int i = 0; i < nh; ++i) n.dims[i + 1] = hid[i];
        n.dims[nh + 1] = out;
        long long o = 0;
        for (int i = 0; i < n.n; ++i) {
            n.b[i] = o;
            o += n.dims[i + 1];
            n.w[i] = o;
            o += (long long)n.dims[i] * n.dims[i + 1];
        }
        n.ln_scale = n.ln_bias = -1;
        if (ln) {
            n.ln_bias = o;
            o += in;
            n.ln_scale = o;
            o += in;
        }
        *total = o;
        return n;
    }
    static Net none() {  // no net: n = 0, every width 0
        Net n{};
        n.ln_scale = n.ln_bias = -1;
        return n;
    }
};

// R * (dims[0] + .. + dims[count - 1])
EM_HD int em_rows(const Net& n, int count) {
    int s = 0;
    for (int i = 0; i < count; ++i) s += n.dims[i] * R;
    return s;
}

// Units of a sweep op with Kc contracted rows and No outputs: ntile output tiles x S k-chunks of
// cks k-steps (4 rows each), at most one unit per wave
EM_HD void sw_plan(int Kc, int No, int& ntile, int& S, int& cks) {
    ntile = (No + 15) >> 4;
    const int nks = (Kc + 3) >> 2;
    S = 1;
    while (S < SW_NW && ntile * S * 2 <= SW_NW && S * 2 <= nks) S *= 2;
    cks = (nks + S - 1) / S;
}
// ... within the block's waves and a wave's fragment registers
inline bool sw_op_fits(int Kc, int No) {
    int ntile, S, cks;
    sw_plan(Kc, No, ntile, S, cks);
    return ntile * S <= SW_NW && cks <= SW_FM;
}

// Dynamic LDS of the three grad kernels, every buffer feature-major [width][R]:
//   x0, xhat [K0] | acts(0..n) [dims[i]] (acts(n): the output) | gA, gB, gC [maxd] | nobs [D] |
//   tacts(0..m) [tpn.dims[i]], or pred [D] in their place when a multistep step has no frozen
//   predictor (pred == tacts(0) either way) | multistep: carry [D] |
//   sweep: scr [SW_SCR floats] | lnacc [2][K0] floats | lnp [2][K0] floats
// m = tpn.n: the host passes Net::none() for tpn when termination_weight == 0 (and for the
// termination kind), so no kernel asks tw for the depth of the frozen stack.
// A single-step launch with m == 0 has no pred buffer (pred == total).
struct EmLds {
    int x0, xhat, acts0, gA, gB, gC, nobs, tacts0, carry, scr, lnacc, lnp, total;
};
EM_HD EmLds em_lds(const Net& net, const Net& tpn, int D, bool multistep, bool sweep) {
    const int K0 = net.dims[0], m = tpn.n;
    int maxd = 0;
    for (int i = 0; i <= net.n; ++i) maxd = maxd > net.dims[i] ? maxd : net.dims[i];
    for (int i = 0; i <= m; ++i) maxd = maxd > tpn.dims[i] ? maxd : tpn.dims[i];
    EmLds l;
    l.x0 = 0;
    l.xhat = l.x0 + K0 * R;
    l.acts0 = l.xhat + K0 * R;
    l.gA = l.acts0 + em_rows(net, net.n + 1);
    l.gB = l.gA + maxd * R;
    l.gC = l.gB + maxd * R;
    l.nobs = l.gC + maxd * R;
    l.tacts0 = l.nobs + D * R;
    l.carry = l.tacts0 + (m > 0 ? em_rows(tpn, m + 1) : multistep ? D * R : 0);
    l.scr = l.carry + (multistep ? D * R : 0);
    l.lnacc = l.scr + (sweep ? SW_SCR : 0);
    l.lnp = l.lnacc + (sweep ? 2 * K0 : 0);
    l.total = l.lnp + (sweep ? 2 * K0 : 0);
    return l;
}
// Layer buffers by summed widths: buffer i of a net's stack that starts at `first`, an offset
// (the host, the 512-thread kernels' pointer arrays) or an LDS pointer (em_sweep_kernel, where a
// stored pointer array went to scratch and an offset added to the base at every use measured
// 1.2 % slower: profiles/emlayout/sweep_variants.txt)
template <class P>
EM_HD P em_layer(P first, const Net& net, int i) {
    for (int j = 0; j < i; ++j) first += net.dims[j] * R;
    return first;
}
EM_HD int em_acts(const EmLds& l, const Net& net, int i) { return em_layer(l.acts0, net, i); }
EM_HD int em_tacts(const EmLds& l, const Net& tpn, int i) { return em_layer(l.tacts0, tpn, i); }

// Record of one (block, step) in the multistep store:
//   xhat [K0][R] | rstd [R] | acts(0..n-1) | own [D][R], the step's own output gradient |
//   sweep: g(i) [dims[i + 1]][R], g(n-1) first (each layer's output gradient after the ReLU
//   mask: the dW operands)
// The backward loads [0, g0) a step ahead.
struct EmRec {
    int xhat, rstd, acts0, own, g0, stride;
};
EM_HD EmRec em_rec(const Net& net, int D, bool sweep) {
    EmRec r;
    r.xhat = 0;
    r.rstd = net.dims[0] * R;
    r.acts0 = r.rstd + R;
    r.own = r.acts0 + em_rows(net, net.n);
    r.g0 = r.own + D * R;
    r.stride = r.g0 + (sweep ? em_rows(net, net.n + 1) - net.dims[0] * R : 0);
    return r;
}
EM_HD int em_rec_acts(const EmRec& r, const Net& net, int i) { return r.acts0 + em_rows(net, i); }
EM_HD int em_rec_g(const EmRec& r, const Net& net, int i) {
    int o = r.g0;
    for (int j = net.n - 1; j > i; --j) o += net.dims[j + 1] * R;
    return o;
}

// What fqlpop_emtrain_create decides for a config and the em_seq_sweep engine option
// (em_plan_try: null and *out, or the refusal, in fqlpop_emtrain_create's order; em_plan throws
// it as FQLPOP_E_ARG).  n_params >= 0: also checked against K models' parameters, where
// fqlpop_emtrain_create checks it.
struct EmPlan {
    Net net, tpn;                // trained net; frozen termination predictor (Net::none() without one)
    long long P, PT;             // their parameter counts
    int T;                       // rows per sequence (1 off the multistep kind)
    int lds_bytes;               // dynamic LDS of em_grad_kernel / em_seq_grad_kernel
    bool sweep;                  // multistep through em_sweep_kernel + em_seq_dw_kernel
    int sweep_lds;               // its dynamic LDS bytes (0 off the sweep path)
    int tchunks;                 // sweep: T chunks of the dW GEMM (partial sets per block)
    int blocks;                  // 16-row blocks per model
    long long seq_stride;        // floats per (block, step) record (0 off the multistep kind)
    // the sizes the sweep's admission bounds: a step's inputs (one per thread), the floats of a
    // record the backward loads (SW_RQ per thread), the dynamic LDS bytes the sweep would ask for
    int nin, rec_floats;
    long long sweep_need;
};

// A refusal of em_nets / em_plan_try: the function returns the text, fqlpop_emtrain_create throws it
#define EM_REFUSE(c, m)     \
    do {                    \
        if (!(c)) return m; \
    } while (0)

// The nets of a config; null, or the refusal (FQLPOP_E_ARG)
inline const char* em_nets(const fqlpop_emtrain_config* c, Net* net, long long* P, Net* tpn, long long* PT) {
    EM_REFUSE(c->obs_dim > 0 && c->action_dim >= 0, "bad obs/action dims");
    EM_REFUSE(c->num_hidden >= 0 && c->num_hidden < MAXL, "bad num_hidden");
    for (int i = 0; i < c->num_hidden; ++i) EM_REFUSE(c->hidden_dims[i] > 0 && c->hidden_dims[i] <= 1024, "bad hidden dim");
    *tpn = Net::none();
    *PT = 0;
    if (c->kind == FQLPOP_EM_STATE_PREDICTOR || c->kind == FQLPOP_EM_MULTISTEP) {
        *net = Net::layout(c->obs_dim + c->action_dim, c->num_hidden, c->hidden_dims, c->obs_dim, true, P);
        if (c->termination_weight > 0.f) {
            EM_REFUSE(c->tp_num_hidden >= 0 && c->tp_num_hidden < MAXL, "bad tp_num_hidden");
            *tpn = Net::layout(c->obs_dim, c->tp_num_hidden, c->tp_hidden_dims, 1, false, PT);
        }
    } else {
        EM_REFUSE(c->kind == FQLPOP_EM_TERMINATION,
                  "kind must be FQLPOP_EM_STATE_PREDICTOR, FQLPOP_EM_TERMINATION or FQLPOP_EM_MULTISTEP");
        *net = Net::layout(c->obs_dim, c->num_hidden, c->hidden_dims, 1, false, P);
    }
    return nullptr;
}

// The sweep path takes every Dense op (both directions, the frozen termination predictor's
// too) as one unit per wave, a step's inputs (actions, next observations, rewards: in_load) as
// one value per thread, a step's record in SW_RQ loads per thread, and its dynamic LDS beside
// em_sweep_kernel's static arrays within a CU's.
inline bool sw_fits(const EmPlan& p) {
    if (p.nin > SW_NT) return false;
    for (const Net* n : {&p.net, &p.tpn})
        for (int i = 0; i < n->n; ++i)
            if (!sw_op_fits(n->dims[i], n->dims[i + 1]) || !sw_op_fits(n->dims[i + 1], n->dims[i])) return false;
    if (p.rec_floats > SW_RQ * SW_NT) return false;
    return p.sweep_need + SW_STATIC_LDS <= CU_LDS_BYTES;
}

inline const char* em_plan_try(const fqlpop_emtrain_config* c, bool sweep_option, long long n_params, int K, EmPlan* out) {
    EM_REFUSE(c->batch_size > 0 && c->batch_size % R == 0, "batch_size must be a positive multiple of 16");
    EM_REFUSE(c->steps > 0, "steps must be > 0");
    EmPlan p{};
    if (const char* why = em_nets(c, &p.net, &p.P, &p.tpn, &p.PT)) return why;
    if (n_params >= 0) EM_REFUSE(n_params == p.P * K, "params size mismatch");
    const bool ms = c->kind == FQLPOP_EM_MULTISTEP;
    p.T = 1;
    if (ms) {
        EM_REFUSE(c->sequence_length >= 1, "sequence_length must be >= 1");
        EM_REFUSE(c->episode_length > c->sequence_length, "episode_length must exceed sequence_length");
        p.T = c->sequence_length;
    }
    const int D = c->obs_dim, A = c->action_dim;
    const long long fl = em_lds(p.net, p.tpn, D, ms, false).total;
    EM_REFUSE(fl * 4 <= EM_LDS_BUDGET, "env-model layer widths exceed the LDS budget of the fused step");
    p.lds_bytes = (int)(fl * 4);
    p.blocks = c->batch_size / R;
    p.tchunks = 1;
    p.nin = R * (A + D + 1);
    p.rec_floats = em_rec(p.net, D, false).g0;
    p.sweep_need = ms ? 4LL * em_lds(p.net, p.tpn, D, true, true).total : 0;
    if (ms && sweep_option && sw_fits(p)) {
        p.sweep = true;
        p.sweep_lds = (int)p.sweep_need;
        // dW GEMM blocks: 16-step chunks at least, at most 4 chunks per sequence block
        p.tchunks = std::max(1, std::min(4, p.T / 16));
    }
    p.seq_stride = ms ? em_rec(p.net, D, p.sweep).stride : 0;
    *out = p;
    return nullptr;
}
#undef EM_REFUSE
inline EmPlan em_plan(const fqlpop_emtrain_config* c, bool sweep_option, long long n_params = -1, int K = 1) {
    EmPlan p;
    const char* why = em_plan_try(c, sweep_option, n_params, K, &p);
    ARGCHK(!why, why);
    return p;
}

// ------------------------------------------------------ initial-observation VAE --
constexpr int VMAXH = 6;   // hidden layers per side

struct VaeDense {
    int K, N, seg;          // in, out, Adam segment
    long long w, b;         // flat offsets
};

// Dynamic LDS of em_vae_grad_kernel ([width][R] each):
//   x [D] | encoder hidden e(1..nh) (e(0) == x) | mu, lv, eps, z [L] | decoder hidden d(1..nh)
//   (d(0) == z) | xhat [D] | gmu, glv [L] | gA, gB [maxd]
struct VaeLds {
    int x, e1, mu, lv, eps, z, d1, xhat, gmu, glv, gA, gB, total;
};
EM_HD VaeLds vae_lds(const VaeDense* enc, const VaeDense* dec, int nh, int D, int L, int maxd) {
    VaeLds l;
    l.x = 0;
    l.e1 = l.x + D * R;
    l.mu = l.e1;
    for (int i = 0; i < nh; ++i) l.mu += enc[i].N * R;
    l.lv = l.mu + L * R;
    l.eps = l.lv + L * R;
    l.z = l.eps + L * R;
    l.d1 = l.z + L * R;
    l.xhat = l.d1;
    for (int i = 0; i < nh; ++i) l.xhat += dec[i].N * R;
    l.gmu = l.xhat + D * R;
    l.glv = l.gmu + L * R;
    l.gA = l.glv + L * R;
    l.gB = l.gA + maxd * R;
    l.total = l.gB + maxd * R;
    return l;
}
// e(i), d(i) for i >= 1: ds = enc with first = e1, or dec with first = d1 (d(i) is dec[i - 1]'s output)
EM_HD int vae_hidden(int first, const VaeDense* ds, int i) {
    for (int j = 0; j + 1 < i; ++j) first += ds[j].N * R;
    return first;
}
// Dynamic LDS of em_vae_decode_kernel: z [L] | d(1..nh) | out [D] (= d(nh + 1), dec[nh]'s output);
// d(i) = vae_hidden(d1, dec, i)
struct VaeDecLds {
    int z, d1, total;
};
EM_HD VaeDecLds vae_dec_lds(const VaeDense* dec, int nh, int L) {
    VaeDecLds l;
    l.z = 0;
    l.d1 = L * R;
    l.total = vae_hidden(l.d1, dec, nh + 2);
    return l;
}

}  // namespace em
}  // namespace fq
