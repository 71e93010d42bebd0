// Env-model trainer: one training step of the
// reference's world-model trainers on the GPU.
//
//   state predictor       envmodel/state_predictor_trainer.py:67-95 on
//                         BaselineStatePredictor (envmodel/baseline.py:25-37),
//                         state_prediction_loss (envmodel/loss.py:80-111) as bound
//                         by train_env_model.py:37-44 (reconstruction weight 0;
//                         a frozen termination predictor scores the predicted next
//                         observation when termination_weight > 0)
//   termination predictor envmodel/termination_predictor_trainer.py:55-76 on
//                         TerminationPredictor (envmodel/termination_predictor.py:
//                         14-21; input dropout while training), focal_loss
//                         (envmodel/loss.py:33-66; train_env_model.py:79)
//   optimiser             optax.adam(cosine_decay_schedule(init_lr, steps))
//
// The nets are small (obs 28-42 -> 128 -> 256 -> 128 -> obs), so one step is
// two launches: em_grad_kernel (block = 16 minibatch rows: forward, loss,
// backward, per-block partial parameter grads, per-block log sums; activations
// in LDS, feature-major [feature][row]; the weights stream from L2) and
// em_adam_kernel (fixed-order sum of the block partials + Adam, which also
// refreshes the W^T copy the dX products read).  Every Dense product (forward,
// dX, dW) runs on v_mfma_f32_16x16x4_f32 with the block's 16 rows as the MFMA
// width; odd widths (33, 28, 1) are padded by the buffer loads' range check.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/fqlpop.h"
#include "emboot.h"
#include "emlayout.h"
#include "hostmem.h"
#include "kernels.h"

#define DEV __device__ __forceinline__

namespace fq {
namespace em {

// (R, NT, the sweep's constants, struct Net and every LDS / record layout: emlayout.h)

// The model axis of an ensemble launch (fqlpop_emtrain_create_ensemble): K models that share
// the dataset, the frozen termination predictor, the config and the update count, each with
// its own parameters, moments, partials, logs, record store, seed and (when injected per
// model) batch, at a fixed stride from model 0's.  A single-model handle is n_models = 1,
// xcd = 0: block == blockIdx.x and every offset 0.
constexpr int ENS_MAX = FQLPOP_EM_ENS_MAX_MODELS;
constexpr int ENS_XCDS = 8;
struct EnsAxis {
    int n_models, bpm, xcd;             // models, blocks per model, placement (ens_block_map)
    long long par;                      // floats between two models' params / wt / m / v
    long long part, logs, seq;          // ... partial sets, block log sums, record stores
    long long obs, act, rew, keep;      // ... injected batches ([B][D], [B][A], [B], mask bytes); 0: one
                                        // shared batch, or the dataset
    uint64_t seeds[ENS_MAX];            // sampling / dropout seed of each model
};

// Linear block id -> (model, block within the model) of a launch of n_models x bpm blocks.
//   xcd = 0: model-major, grid = n_models bpm, no padding.
//   xcd = 1: blocks are dealt round-robin over the 8 XCDs (ids l and l + 8 share one; observed,
//   not promised), so id l sits on XCD x = l % 8 in slot j = l / 8.  With K >= 8 models XCD x
//   holds the models x, x + 8, .. (at most ceil(K / 8)), one after the other in its slots;
//   with K < 8 a model owns S = 8 / K neighbouring XCDs and deals its blocks over them.
//   Either way an XCD's L2 sees the W and W^T of at most ceil(K / 8) models.  Ids that fall
//   outside (model >= K, block >= bpm) are padding: *model = -1, the block exits at once.
// Returns the grid size.  The results of a launch do not depend on the mapping: every
// per-block quantity (sampling index, dropout position, partial slot) uses the block within
// the model.
__host__ __device__ inline int ens_block_map(int n_models, int bpm, int xcd, int lin, int* model, int* block) {
    if (!xcd) {
        *model = lin / bpm;
        *block = lin - *model * bpm;
        return n_models * bpm;
    }
    const int S = n_models >= ENS_XCDS ? 1 : ENS_XCDS / n_models;  // XCDs per model
    const int G = (n_models + ENS_XCDS - 1) / ENS_XCDS;            // models per XCD
    const int cb = (bpm + S - 1) / S;                              // slots of one model on one XCD
    const int x = lin % ENS_XCDS, j = lin / ENS_XCDS;
    const int g = j / cb, r = j - g * cb;
    const int mdl = x / S + ENS_XCDS * g, blk = r * S + x % S;
    const bool pad = mdl >= n_models || blk >= bpm || g >= G;
    *model = pad ? -1 : mdl;
    *block = pad ? -1 : blk;
    return ENS_XCDS * G * cb;
}

struct StepArgs {
    EnsAxis ens;
    int kind;                           // FQLPOP_EM_STATE_PREDICTOR / FQLPOP_EM_TERMINATION
    int train;                          // 1: grads + dropout; 0: eval logs only
    Net net, tpn;                       // trained net; frozen termination predictor (kind 0, tw > 0)
    // params, wt, part, logs, seq (and an injected batch) are model 0's: a block reads its own
    // model's through ModelView (ens_enter); tp / tpt and the dataset are shared
    const float* params;
    const float* tp;
    const float *wt, *tpt;              // W^T copies of params / tp (Dense kernels [out][in], same offsets)
    float* part;                        // [blocks][P] partial grads
    long long P;
    float* logs;                        // [blocks][NLOG]
    // rows: injected [B][..] arrays, or gathered from the dataset by Philox indices
    const float *obs, *act, *rew, *nobs;
    long long n_rows;
    int injected;
    const unsigned char* keep;          // injected dropout keep mask [B][obs] or null
    long long step;                   // update count (sampling counter)
    int B, D, A;
    float tw, ttw, alpha, gamma, rate;
    // multistep (FQLPOP_EM_MULTISTEP): sequence length, rows per dataset episode, and the
    // per-(block, step) activation store of the backpropagation through time
    int T, ep_len;
    float* seq;
    long long seq_stride;
    int tchunks;                        // sweep path: T chunks of the dW GEMM (partials per block)
    unsigned long long* probe;          // diagnostic builds only (FQLPOP_EM_PROBE): sweep phase times
    // device-sampled launches only (em_unit): null, or model 0's table of units, tab_stride
    // entries (n_units) per model.  Training: the bootstrap table.  oob_eval
    // (fqlpop_emtrain_eval_oob): the out-of-bag list, n_oob[model] long, for batch oob_batch of
    // the call's draw oob_draw.  (Behind every earlier field, whose offsets the kernels keep.)
    const long long* tab;
    long long tab_stride;
    const long long* n_oob;
    int oob_eval;
    uint32_t oob_batch, oob_draw;
};

// ----------------------------------------------------------------- Philox
DEV void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
// uniform [0, 1) from (seed, a, b, c)
DEV float urand(uint64_t seed, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t x[4] = {a, b, c, 0x3E7u};
    philox(x, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (x[0] >> 8) * (1.0f / 16777216.0f);
}

// Counter word 2 of the unit draws: a minibatch row, a multistep episode (the VAE section lists
// its own); a bootstrap table entry and an out-of-bag unit (include/fqlpop.h)
constexpr uint32_t SALT_ROW = 0xE7u, SALT_EP = 0xE5u;
constexpr uint32_t SALT_BOOT = FQLPOP_EM_SALT_BOOT, SALT_OOB = FQLPOP_EM_SALT_OOB;

DEV float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// Dense layers on v_mfma_f32_16x16x4_f32: out[m][c] = act(sum_k A[k][m] x[k][c] + bias[m])
// for m < M, c < R = 16 (LDS, feature-major [m][R]); A is k-major [Kr][M] (m contiguous).
// A block's 8 waves take 16-feature output tiles round-robin; a wave loads the A
// fragments of KS k-steps (4 k each, up to 32) into registers at once (all in flight: the loop is
// L2-latency bound otherwise), then runs the MFMAs with x from LDS.  Forward: A = W
// [K][N]; dX: A = W^T [N][K] with mask = relu'(the layer input).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;
// An LDS activation pointer that went through a runtime-indexed pointer array (acts[i]) is
// generic again: its accesses compile to flat instructions, which count in both vmcnt and
// lgkmcnt, so every LDS read behind them also waited for the global loads and stores in
// flight.  The assumption lets the compiler address LDS directly.
template <typename T>
DEV T* lds_ptr(T* p) {
#if __HIP_DEVICE_COMPILE__  // (the builtin exists for the device pass only)
    __builtin_assume(__builtin_amdgcn_is_shared((const void*)p));
#endif
    return p;
}
template <int KS>
DEV void em_mfma_t(const float* __restrict__ A, const float* __restrict__ bias, const float* x, int Kr, int M,
                   float* y, bool relu, const float* mask) {
    x = lds_ptr(x);
    y = lds_ptr(y);
    if (mask) mask = lds_ptr(mask);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int ntile = (M + 15) / 16, nks = (Kr + 3) / 4;
    // unguarded buffer loads (a guarded load compiles to a branch + vmcnt(0) wait): k >= Kr
    // falls past the range and reads 0; a lane's o >= M only feeds its own discarded row
    const rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)A, (short)0, Kr * M * 4, 0x00020000);
    for (int t = w; t < ntile; t += NT / 64) {
        const int o = 16 * t + li;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < nks; s0 += KS) {
            float av[KS];
#pragma unroll
            for (int u = 0; u < KS; ++u)
                av[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                      rA, ((4 * (s0 + u) + lk) * M + o) * 4, 0, 0));
#pragma unroll
            for (int u = 0; u < KS; ++u) {
                if (s0 + u < nks) {
                    const int k = 4 * (s0 + u) + lk;
                    const float xv = x[min(k, Kr - 1) * R + li];
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], k < Kr ? xv : 0.f, acc, 0, 0, 0);
                }
            }
        }
        // acc[r]: output m = 16t + 4lk + r, column li
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 16 * t + 4 * lk + r;
            if (m < M) {
                float v = acc[r] + (bias ? bias[m] : 0.f);
                if (relu) v = fmaxf(v, 0.f);
                if (mask && !(mask[m * R + li] > 0.f)) v = 0.f;  // relu' (0 at 0)
                y[m * R + li] = v;
            }
        }
    }
    __syncthreads();
}
// KSMAX: the most k-steps a wave keeps in flight (32 = 32 VGPRs of fragments; the multistep
// kernel, at its register limit, takes 16)
template <int KSMAX = 32>
DEV void em_mfma(const float* A, const float* bias, const float* x, int Kr, int M, float* y, bool relu,
                 const float* mask) {
    if (Kr <= 32) em_mfma_t<8>(A, bias, x, Kr, M, y, relu, mask);
    else if (Kr <= 64 || KSMAX < 32) em_mfma_t<16>(A, bias, x, Kr, M, y, relu, mask);
    else em_mfma_t<32>(A, bias, x, Kr, M, y, relu, mask);
}
// out[f][r] = act(sum_k W[k][f] in[k][r] + b[f])
template <int KSMAX = 32>
DEV void dense_fwd(const float* W, const float* b, const float* in, int K, int N, float* out, bool relu) {
    em_mfma<KSMAX>(W, b, in, K, N, out, relu, nullptr);
}
// g_in[k][r] = sum_f W[k][f] g[f][r] (times relu'(in) when mask_in), from WT = W^T [N][K]
// (the transposed copy the optimiser keeps)
template <int KSMAX = 32>
DEV void dense_dx(const float* WT, const float* g, int K, int N, float* g_in, const float* mask_in) {
    em_mfma<KSMAX>(WT, nullptr, g, N, K, g_in, false, mask_in);
}

// Partial parameter grads of one Dense over the block's rows (MFMA over the 16 rows):
// dW[k][f] = sum_r in[k][r] g[f][r], db[f] = sum_r g[f][r]
// (acc: added to the partials already there -- the sum over the steps of a sequence).
// A wave's tiles go in batches of DW_MT: with acc, the batch's old partials are loaded
// first, all in flight together (one dependent read per tile cost one L2 round trip each,
// 16 of them per wave in a 128 x 256 layer, at every step of a multistep sequence)
constexpr int DW_MT = 8;
DEV void dense_dw(const float* in, const float* g, int K, int N, float* __restrict__ pW, float* __restrict__ pb,
                  bool acc = false) {
    in = lds_ptr(in);
    g = lds_ptr(g);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int tf = (N + 15) / 16, nt = (K + 15) / 16 * tf;
    constexpr int NW = NT / 64;
    for (int t0 = w; t0 < nt; t0 += NW * DW_MT) {
        float old[DW_MT][4];
        if (acc) {
#pragma unroll
            for (int j = 0; j < DW_MT; ++j) {
                const int t = min(t0 + NW * j, nt - 1);  // past the wave's last tile: a re-read
                const int k0 = 16 * (t / tf), f0 = 16 * (t % tf);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = min(k0 + 4 * lk + q, K - 1), f = min(f0 + li, N - 1);  // in range
                    old[j][q] = pW[(long long)k * N + f];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < DW_MT; ++j) {
            const int t = t0 + NW * j;
            if (t >= nt) break;
            const int k0 = 16 * (t / tf), f0 = 16 * (t % tf);
            f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < R / 4; ++s) {
                const float av = k0 + li < K ? in[(k0 + li) * R + 4 * s + lk] : 0.f;  // A[k][r]
                const float bv = f0 + li < N ? g[(f0 + li) * R + 4 * s + lk] : 0.f;   // B[r][f]
                d = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, d, 0, 0, 0);
            }
            // d[q]: k = k0 + 4lk + q, f = f0 + li
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + 4 * lk + q, f = f0 + li;
                if (k < K && f < N) pW[(long long)k * N + f] = acc ? old[j][q] + d[q] : d[q];
            }
        }
    }
    for (int f = threadIdx.x; f < N; f += NT) {
        const float* b = g + f * R;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) s += b[r];
        pb[f] = acc ? pb[f] + s : s;
    }
}

// Frozen termination predictor on pred = tacts[0] [D][R]: weighted BCE of its logit
// (envmodel/loss.py:14-30) into the log sums 1..5, and its input gradient, scaled by
// tw / norm, added to gA [D][R].  inv_n: 1 / (number of scored predictions).
template <int KSMAX = 32>
DEV void tp_score(const StepArgs& a, float* const* tacts, float* gA, float* gB, float* gC, const float* lab,
                  float (*lsum)[R], float inv_n, float norm) {
    const Net& T = a.tpn;
    const int tid = threadIdx.x;
    for (int i = 0; i < T.n; ++i)
        dense_fwd<KSMAX>(a.tp + T.w[i], a.tp + T.b[i], tacts[i], T.dims[i], T.dims[i + 1], tacts[i + 1], i < T.n - 1);
    if (tid < R) {
        const float x = lds_ptr(tacts[T.n])[tid], z = lab[tid], w = a.ttw;
        const float ce = softplus(x) - x * z;
        lsum[1][tid] += (z > 0.f ? w * ce : ce) / (w + 1.f);
        lsum[2][tid] += z > 0.f ? ce : 0.f;
        lsum[3][tid] += z > 0.f ? 0.f : ce;
        lsum[4][tid] += z;
        lsum[5][tid] += 1.f - z;
        const float p = 1.0f / (1.0f + expf(-x));
        gB[tid] = (z > 0.f ? w : 1.f) / (w + 1.f) * (p - z) * inv_n;  // d bce / d logit
    }
    __syncthreads();
    // dX down the frozen stack (relu' of each hidden input), gB <-> gC
    float* src = gB;
    float* dst = gC;
    for (int i = T.n - 1; i >= 0; --i) {
        dense_dx<KSMAX>(a.tpt + T.w[i], src, T.dims[i], T.dims[i + 1], dst, i > 0 ? tacts[i] : nullptr);
        float* tmp = src;
        src = dst;
        dst = tmp;
    }
    src = lds_ptr(src);
    for (int t = tid; t < a.D * R; t += NT) gA[t] += a.tw / norm * src[t];
    __syncthreads();
}

// Squared-error log sums of the block's R rows over the D features, in a fixed order: the
// block's last wave, lane = r + 16 g, sums d^2 of row r over the features k = g (mod 4) in
// ascending k, then (s0 + s1) + (s2 + s3), and adds that to lsum0[r].  (An LDS atomicAdd per
// element left the order of the sum, and with it the last bit of the logged loss, to the wave
// scheduling: a model's logs must not depend on what runs beside it.)  d is computed as the
// loss does, (out + x0) - nobs; out, x0 and nobs are final on entry and the barrier that
// follows the caller's own loop over the elements publishes lsum0.
template <int NTHREADS>
DEV void sq_err_rows(const float* out, const float* x0, const float* nobs, int D, float* lsum0) {
    const int l = (int)threadIdx.x - (NTHREADS - 64);
    if (l < 0) return;
    const int r = l & 15, g = l >> 4;
    float s = 0.f;
    for (int k = g; k < D; k += 4) {
        const float p = out[k * R + r] + x0[k * R + r];
        const float d = p - nobs[k * R + r];
        s += d * d;
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (g == 0) lsum0[r] += s;
}

// The state predictor's loss on out [D][R]: pred = out + obs (x0 rows k < D are the
// observations), kept when keep_pred (the frozen termination predictor's input, the next step's
// observation); gA = d MSE / d pred scaled by gscale; squared errors into lsum0; a barrier.
template <int NTHREADS>
DEV void pred_loss(const float* out, const float* x0, const float* nobs, float* pred, bool keep_pred, float* gA, int D,
                   float gscale, float* lsum0, int tid) {
    for (int q = tid; q < D * R; q += NTHREADS) {
        const float p = out[q] + x0[q];
        const float d = p - nobs[q];
        if (keep_pred) pred[q] = p;
        gA[q] = gscale * d;
    }
    sq_err_rows<NTHREADS>(out, x0, nobs, D, lsum0);
    __syncthreads();
}

// A block's model: the per-model pointers and seed of StepArgs moved to the block's model, and
// the block's index within it.  Derived once at kernel entry; the model index and every offset
// are wave-uniform (blockIdx and kernel arguments only; readfirstlane pins the quotients of
// the block map, whose division expands to vector instructions, back into scalar registers,
// so that no buffer resource built from these pointers ends up in a waterfall loop).
struct ModelView {
    const float *params, *wt;
    float *part, *logs, *seq;
    const float *obs, *act, *rew, *nobs;
    const unsigned char* keep;
    const long long* tab;
    uint64_t seed;
    int blk, model;
};
DEV bool ens_enter(const StepArgs& a, ModelView& m) {
    const EnsAxis& e = a.ens;
    {
        // One word of every 64-byte line of the kernel arguments, requested together ahead of the
        // branches below.  The arguments of a launch are cold, and the loads behind a branch that
        // itself waits for arguments start only once it is taken: a second round trip to memory
        // (measured: + 0.5 us per single-model launch without this).
        // (Separate operands of one empty asm: an OR over the words was scheduled as two rounds.)
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&a);
        constexpr int LAST = (int)(sizeof(StepArgs) / 4) - 1;
        static_assert(LAST < 16 * 16, "StepArgs outgrew the 16 lines touched here");
#define EM_W(i) "s"(w[(i) * 16 < LAST ? (i) * 16 : LAST])
        asm volatile("" ::EM_W(0), EM_W(1), EM_W(2), EM_W(3), EM_W(4), EM_W(5), EM_W(6), EM_W(7), EM_W(8), EM_W(9),
                     EM_W(10), EM_W(11), EM_W(12), EM_W(13), EM_W(14), EM_W(15));
#undef EM_W
    }
    int model = 0, blk = (int)blockIdx.x;
    if (e.n_models > 1 || e.xcd) {  // (one model, no remap: the single-model launch as it was)
        ens_block_map(e.n_models, e.bpm, e.xcd, (int)blockIdx.x, &model, &blk);
        model = __builtin_amdgcn_readfirstlane(model);
        blk = __builtin_amdgcn_readfirstlane(blk);
        if (model < 0) return false;  // padding of the XCD placement
    }
    m.blk = blk;
    m.model = model;
    m.tab = a.tab ? a.tab + model * a.tab_stride : nullptr;
    m.params = a.params + model * e.par;
    m.wt = a.wt + model * e.par;
    m.part = a.part + model * e.part;
    m.logs = a.logs + model * e.logs;
    m.seq = a.seq + model * e.seq;
    m.obs = a.obs + model * e.obs;
    m.act = a.act + model * e.act;
    m.rew = a.rew + model * e.rew;
    m.nobs = a.nobs + model * e.obs;
    m.keep = a.keep ? a.keep + model * e.keep : nullptr;
    m.seed = e.seeds[0];  // (with the other arguments; a later model's is one more scalar load)
    if (model > 0) m.seed = e.seeds[model];
    return true;
}

// The unit (dataset row, or episode of the multistep model) of batch position gr in a
// device-sampled launch; *c2: the counter's third word (the multistep window start).  The index
// u = (x1 << 32 | x0) mod n_units is the unit itself without a table (a handle without
// bootstrap: the draw as it always was), else the table's entry u.  An out-of-bag evaluation
// draws from its own counter, over the model's list.  Every condition is block-uniform.
DEV long long em_unit(const StepArgs& a, const ModelView& m, int gr, uint32_t salt, long long n_units, uint32_t* c2) {
    const bool ev = a.oob_eval != 0;
    uint32_t c[4] = {(uint32_t)gr, ev ? a.oob_batch : (uint32_t)a.step, ev ? SALT_OOB : salt, ev ? a.oob_draw : 0u};
    philox(c, (uint32_t)m.seed, (uint32_t)(m.seed >> 32));
    *c2 = c[2];
    const uint64_t v = ((uint64_t)c[1] << 32) | c[0];
    if (!m.tab) return (long long)(v % (uint64_t)n_units);
    const long long n = ev ? a.n_oob[m.model] : n_units;
    return m.tab[v % (uint64_t)n];
}

// First dataset row of batch position gr's sequence: injected [B][T] rows, or a MultistepLoader
// window of T steps inside a Philox-drawn episode
DEV long long em_window(const StepArgs& a, const ModelView& mv, int gr) {
    if (a.injected) return (long long)gr * a.T;
    uint32_t c2;
    const long long ep = em_unit(a, mv, gr, SALT_EP, a.n_rows / a.ep_len, &c2);
    const long long st = (long long)(c2 % (uint32_t)(a.ep_len - a.T));
    return ep * a.ep_len + st;
}

// flax LayerNorm statistics of row r of x0 [K0][R] (eps 1e-6, E[x^2] - mu^2 clipped)
DEV void ln_stats(const float* x0, int K0, int r, float* mu_s, float* rs_s) {
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < K0; ++k) {
        const float v = x0[k * R + r];
        s1 += v;
        s2 += v * v;
    }
    const float mu = s1 / K0;
    mu_s[r] = mu;
    rs_s[r] = 1.0f / sqrtf(fmaxf(s2 / K0 - mu * mu, 0.f) + 1e-6f);
}

__global__ __launch_bounds__(NT) void em_grad_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float lsum[NLOG][R];
    __shared__ float lab[R];
    __shared__ long long rowid[R];
    ModelView mv;
    if (!ens_enter(a, mv)) return;
    const int tid = threadIdx.x, blk = mv.blk;
    const Net& N = a.net;
    const int D = a.D, A = a.A;
    const int K0 = N.dims[0];
    const EmLds L = em_lds(N, a.tpn, D, false, false);
    float* x0 = lds + L.x0;
    float* xhat = lds + L.xhat;
    float* acts[MAXL + 1];
    float* tacts[MAXL + 1];
    for (int i = 0; i <= N.n; ++i) acts[i] = lds + em_acts(L, N, i);
    for (int i = 0; i <= a.tpn.n; ++i) tacts[i] = lds + em_tacts(L, a.tpn, i);
    float* gA = lds + L.gA;
    float* gB = lds + L.gB;
    float* gC = lds + L.gC;
    float* nobs = lds + L.nobs;

    // ---- rows: injected batch rows, or Philox-drawn dataset rows ([EXT] Dataset.sample)
    if (tid < R) {
        const int gr = blk * R + tid;
        long long id = gr;
        if (!a.injected) {
            uint32_t c2;
            id = em_unit(a, mv, gr, SALT_ROW, a.n_rows, &c2);
        }
        rowid[tid] = id;
        lab[tid] = mv.rew[id] == 0.f ? 1.f : 0.f;
    }
    for (int q = tid; q < NLOG * R; q += NT) lsum[q / R][q % R] = 0.f;
    __syncthreads();
    for (int t = tid; t < D * R; t += NT) {
        const int k = t / R, r = t % R;
        nobs[t] = mv.nobs[rowid[r] * D + k];
    }
    if (a.kind == FQLPOP_EM_STATE_PREDICTOR) {
        for (int t = tid; t < K0 * R; t += NT) {
            const int k = t / R, r = t % R;
            x0[t] = k < D ? mv.obs[rowid[r] * D + k] : mv.act[rowid[r] * A + (k - D)];
        }
    } else {
        // termination predictor: dropout on the input while training; the keep mask is fixed
        // per (batch position, feature), as the reference's constant dropout rng
        for (int t = tid; t < K0 * R; t += NT) {
            const int k = t / R, r = t % R;
            float v = mv.nobs[rowid[r] * D + k];
            if (a.train) {
                const int pos = blk * R + r;
                const bool keep = mv.keep ? mv.keep[(long long)pos * D + k] != 0
                                          : urand(mv.seed, (uint32_t)pos, (uint32_t)k, 0xD20u) >= a.rate;
                v = keep ? v / (1.0f - a.rate) : 0.f;
            }
            x0[t] = v;
        }
    }
    __syncthreads();

    // ---- forward
    const float* P = mv.params;
    if (N.ln_scale >= 0) {
        // flax LayerNorm over the K0 input features of each row
        __shared__ float mu_s[R], rs_s[R];
        if (tid < R) ln_stats(x0, K0, tid, mu_s, rs_s);
        __syncthreads();
        for (int t = tid; t < K0 * R; t += NT) {
            const int k = t / R, r = t % R;
            const float xh = (x0[t] - mu_s[r]) * rs_s[r];
            xhat[t] = xh;
            lds_ptr(acts[0])[t] = xh * P[N.ln_scale + k] + P[N.ln_bias + k];
        }
    } else {
        for (int t = tid; t < K0 * R; t += NT) lds_ptr(acts[0])[t] = x0[t];
    }
    __syncthreads();
    for (int i = 0; i < N.n; ++i)
        dense_fwd(P + N.w[i], P + N.b[i], acts[i], N.dims[i], N.dims[i + 1], acts[i + 1], i < N.n - 1);
    const float* out = lds_ptr(acts[N.n]);

    // ---- loss, output gradient (gA [dout][R]) and log sums
    const float invB = 1.0f / (float)a.B;
    if (a.kind == FQLPOP_EM_STATE_PREDICTOR) {
        // pred = out + obs; MSE(pred, next) over B x D; grads / (1 + tw)
        const float norm = 1.0f + a.tw;
        const float gscale = 2.0f / ((float)a.B * D) / norm;
        // (without a frozen termination predictor a single step has no pred buffer: em_lds)
        pred_loss<NT>(out, x0, nobs, lds_ptr(tacts[0]), a.tpn.n > 0, gA, D, gscale, lsum[0], tid);
        if (a.tw > 0.f) tp_score(a, tacts, gA, gB, gC, lab, lsum, invB, norm);
    } else {
        // focal loss (alpha, gamma) on the logit
        if (tid < R) {
            const float x = out[tid], z = lab[tid];
            const float p = 1.0f / (1.0f + expf(-x));
            const float ce = softplus(x) - x * z;
            const float pt = z > 0.f ? p : 1.f - p;
            const float af = z > 0.f ? a.alpha : 1.f - a.alpha;
            const float li = af * powf(1.f - pt, a.gamma) * ce;
            const float logp = -softplus(-x), log1mp = -softplus(x);
            const float d = z > 0.f ? powf(1.f - p, a.gamma) * (a.gamma * p * logp - (1.f - p))
                                    : powf(p, a.gamma) * (-a.gamma * (1.f - p) * log1mp + p);
            gA[tid] = af * d * invB;
            lsum[1][tid] = li;
            lsum[2][tid] = z > 0.f ? li : 0.f;
            lsum[3][tid] = z > 0.f ? 0.f : li;
            lsum[4][tid] = z;
            lsum[5][tid] = 1.f - z;
            const bool pr = x > 0.f;
            lsum[6][tid] = (pr == (z > 0.f)) ? 1.f : 0.f;
            lsum[7][tid] = (pr && z > 0.f) ? 1.f : 0.f;
            lsum[8][tid] = pr ? 1.f : 0.f;
        }
        __syncthreads();
    }

    // ---- block log sums
    if (tid < NLOG) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += lsum[tid][r];
        mv.logs[(long long)blk * NLOG + tid] = s;
    }
    if (!a.train) return;

    // ---- backward: partial grads of every Dense (and LayerNorm_0)
    float* pg = mv.part + (long long)blk * a.P;
    float* g = gA;
    float* gn = gB;
    for (int i = N.n - 1; i >= 0; --i) {
        dense_dw(acts[i], g, N.dims[i], N.dims[i + 1], pg + N.w[i], pg + N.b[i]);
        if (i > 0 || N.ln_scale >= 0) dense_dx(mv.wt + N.w[i], g, N.dims[i], N.dims[i + 1], gn, i > 0 ? acts[i] : nullptr);
        else __syncthreads();
        float* tmp = g;
        g = gn;
        gn = tmp;
    }
    if (N.ln_scale >= 0) {
        // g = grad wrt the LayerNorm output [K0][R]
        g = lds_ptr(g);
        for (int k = tid; k < K0; k += NT) {
            float ss = 0.f, sb = 0.f;
            for (int r = 0; r < R; ++r) {
                ss += g[k * R + r] * xhat[k * R + r];
                sb += g[k * R + r];
            }
            pg[N.ln_scale + k] = ss;
            pg[N.ln_bias + k] = sb;
        }
    }
}

// Multistep state predictor (envmodel/multistep.py:31-54): block = 16 sequences, the
// baseline cell stepped T times from observations[:, 0] (each step's prediction is the
// next step's observation), the loss of every step as in em_grad_kernel (normalised over
// B x T), then backpropagation through time: the step's activations go to a per-block
// store in HBM on the way forward and come back in reverse; the gradient w.r.t. the
// carried observation (the residual plus the LayerNorm input gradient of its D
// features) flows from step t + 1 into step t.  Partial grads accumulate over the steps.
#ifndef EM_SEQ_KS
#define EM_SEQ_KS 16
#endif
__global__ __launch_bounds__(NT) void em_seq_grad_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float lsum[NLOG][R];
    __shared__ float lab[R];
    __shared__ long long rowbase[R];
    __shared__ float mu_s[R], rs_s[R], cs[2][R];
    static_assert(sizeof(lsum) + sizeof(lab) + sizeof(rowbase) + sizeof(mu_s) + sizeof(rs_s) + sizeof(cs) + SW_PH_LDS ==
                      SW_STATIC_LDS, "em_seq_grad_kernel's __shared__ arrays are em_sweep_kernel's (SW_STATIC_LDS)");
    ModelView mv;
    if (!ens_enter(a, mv)) return;
    const int tid = threadIdx.x, blk = mv.blk;
    const Net& N = a.net;
    const int D = a.D, A = a.A, T = a.T;
    const int K0 = N.dims[0];
    const EmLds L = em_lds(N, a.tpn, D, true, false);  // carry: the gradient w.r.t. the carried observation
    const EmRec rc = em_rec(N, D, false);
    float* x0 = lds + L.x0;
    float* xhat = lds + L.xhat;
    float* acts[MAXL + 1];
    float* tacts[MAXL + 1];
    for (int i = 0; i <= N.n; ++i) acts[i] = lds + em_acts(L, N, i);
    for (int i = 0; i <= a.tpn.n; ++i) tacts[i] = lds + em_tacts(L, a.tpn, i);
    float* gA = lds + L.gA;
    float* gB = lds + L.gB;
    float* gC = lds + L.gC;
    float* nobs = lds + L.nobs;
    float* carry = lds + L.carry;

    // ---- sequences: injected [B][T] rows, or MultistepLoader windows drawn by Philox
    if (tid < R) rowbase[tid] = em_window(a, mv, blk * R + tid);
    for (int q = tid; q < NLOG * R; q += NT) lsum[q / R][q % R] = 0.f;
    __syncthreads();

    const float* P = mv.params;
    const float norm = 1.0f + a.tw;
    const float inv_n = 1.0f / ((float)a.B * (float)T);
    const float gscale = 2.0f / ((float)a.B * (float)T * D) / norm;
    float* const sq = mv.seq + (long long)blk * T * a.seq_stride;  // this block's store (records: em_rec)
    const int act_floats = rc.own - rc.acts0;

    // ---- forward through the sequence
    for (int t = 0; t < T; ++t) {
        for (int q = tid; q < K0 * R; q += NT) {
            const int k = q / R, r = q % R;
            const long long row = rowbase[r] + t;
            if (k >= D) x0[q] = mv.act[row * A + (k - D)];
            else if (t == 0) x0[q] = mv.obs[row * D + k];  // later steps: the previous prediction
        }
        for (int q = tid; q < D * R; q += NT) {
            const int k = q / R, r = q % R;
            nobs[q] = mv.nobs[(rowbase[r] + t) * D + k];
        }
        if (tid < R) lab[tid] = mv.rew[rowbase[tid] + t] == 0.f ? 1.f : 0.f;
        __syncthreads();
        if (tid < R) ln_stats(x0, K0, tid, mu_s, rs_s);
        __syncthreads();
        for (int q = tid; q < K0 * R; q += NT) {
            const int k = q / R, r = q % R;
            const float xh = (x0[q] - mu_s[r]) * rs_s[r];
            xhat[q] = xh;
            lds_ptr(acts[0])[q] = xh * P[N.ln_scale + k] + P[N.ln_bias + k];
        }
        __syncthreads();
        for (int i = 0; i < N.n; ++i)
            dense_fwd<EM_SEQ_KS>(P + N.w[i], P + N.b[i], acts[i], N.dims[i], N.dims[i + 1], acts[i + 1], i < N.n - 1);
        const float* out = lds_ptr(acts[N.n]);
        float* pred = lds_ptr(tacts[0]);
        pred_loss<NT>(out, x0, nobs, pred, true, gA, D, gscale, lsum[0], tid);
        if (a.tw > 0.f) tp_score<EM_SEQ_KS>(a, tacts, gA, gB, gC, lab, lsum, inv_n, norm);
        if (a.train) {
            float* st = sq + (long long)t * a.seq_stride;
            for (int q = tid; q < K0 * R; q += NT) st[rc.xhat + q] = xhat[q];
            if (tid < R) st[rc.rstd + tid] = rs_s[tid];
            float* sa = st + rc.acts0;
            for (int q = tid; q < act_floats; q += NT) sa[q] = lds_ptr(acts[0])[q];  // acts[0..n-1] are contiguous
            float* sg = st + rc.own;
            for (int q = tid; q < D * R; q += NT) sg[q] = gA[q];
        }
        for (int q = tid; q < D * R; q += NT) x0[q] = pred[q];  // the next step's observation
        __syncthreads();
    }
    if (tid < NLOG) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += lsum[tid][r];
        mv.logs[(long long)blk * NLOG + tid] = s;
    }
    if (!a.train) return;

    // ---- backward through time
    float* pg = mv.part + (long long)blk * a.P;
    for (int t = T - 1; t >= 0; --t) {
        const bool acc = t < T - 1;
        const float* st = sq + (long long)t * a.seq_stride;
        {
            // the step's record (xhat | rstd | acts[0..n-1]) in batches of 8 loads per thread,
            // all in flight before their LDS stores (one HBM round trip per element otherwise)
            constexpr int BQ = 8;
            const int n1 = rc.rstd, n2 = rc.acts0, n3 = rc.own;
            float* const a0 = lds_ptr(acts[0]);
            for (int q0 = tid; q0 < n3; q0 += BQ * NT) {
                float v[BQ];
#pragma unroll
                for (int j = 0; j < BQ; ++j) v[j] = st[min(q0 + j * NT, n3 - 1)];  // unguarded
#pragma unroll
                for (int j = 0; j < BQ; ++j) {
                    const int q = q0 + j * NT;
                    if (q < n1) xhat[q] = v[j];
                    else if (q < n2) rs_s[q - n1] = v[j];
                    else if (q < n3) a0[q - n2] = v[j];
                }
            }
        }
        const float* sg = st + rc.own;
        // total gradient w.r.t. this step's prediction: its own loss terms + the next step's
        for (int q = tid; q < D * R; q += NT) {
            const float gv = sg[q] + (acc ? carry[q] : 0.f);
            gA[q] = gv;
            carry[q] = gv;  // the residual path: pred_t = out_t + obs_t
        }
        __syncthreads();
        float* g = gA;
        float* gn = gB;
        for (int i = N.n - 1; i >= 0; --i) {
            dense_dw(acts[i], g, N.dims[i], N.dims[i + 1], pg + N.w[i], pg + N.b[i], acc);
            dense_dx<EM_SEQ_KS>(mv.wt + N.w[i], g, N.dims[i], N.dims[i + 1], gn, i > 0 ? acts[i] : nullptr);
            float* tmp = g;
            g = gn;
            gn = tmp;
        }
        // g = grad w.r.t. the LayerNorm output [K0][R]
        g = lds_ptr(g);
        for (int k = tid; k < K0; k += NT) {
            float ss = 0.f, sb = 0.f;
            for (int r = 0; r < R; ++r) {
                ss += g[k * R + r] * xhat[k * R + r];
                sb += g[k * R + r];
            }
            pg[N.ln_scale + k] = acc ? pg[N.ln_scale + k] + ss : ss;
            pg[N.ln_bias + k] = acc ? pg[N.ln_bias + k] + sb : sb;
        }
        if (tid < R) {
            float c1 = 0.f, c2 = 0.f;
            for (int k = 0; k < K0; ++k) {
                const float gy = g[k * R + tid] * P[N.ln_scale + k];
                c1 += gy;
                c2 += gy * xhat[k * R + tid];
            }
            cs[0][tid] = c1 / K0;
            cs[1][tid] = c2 / K0;
        }
        __syncthreads();
        // LayerNorm input gradient of the observation features: into the carry
        for (int q = tid; q < D * R; q += NT) {
            const int k = q / R, r = q % R;
            carry[q] += rs_s[r] * (g[q] * P[N.ln_scale + k] - cs[0][r] - xhat[q] * cs[1][r]);
        }
        __syncthreads();
    }
}

// ====================================== multistep BPTT as sweeps (round 6, 1024 threads) ==
// em_seq_grad_kernel at the reference defaults (B = 256, T = 256) is 16 blocks of 512 threads
// whose every Dense product is a chain of L2 round trips (A fragments in batches of 16
// k-steps, up to 8 batches per wave and layer), and whose backward read-modify-writes the
// block's partial dW in L2 at every one of the T steps: 18 ms per train step (VERDICT r5
// item 6).  This path splits the work where the dependencies allow:
//   * em_sweep_kernel (16 waves per block, the same 16 sequences per block): every Dense op
//     of a step is at most ONE unit per wave, a 16-wide output tile x a chunk of <= 32
//     k-steps (split-K partials summed in a fixed order through LDS), and the A fragments of
//     the NEXT op are loaded while the current op's MFMAs run (weights do not depend on the
//     data; the barriers wait for LDS only), so an op costs about one MFMA chain and one or
//     two barriers instead of 2-8 dependent L2 round trips;
//   * its backward sweep runs only what is sequential in t: the dX chain, the LayerNorm
//     backward and the carried observation gradient; it stores each layer's output gradient
//     g_i beside the forward record, and sums the LayerNorm grads over t in LDS;
//   * em_seq_dw_kernel: dW_i = sum over the (t, row) pairs of acts_i g_i^T and db_i, one GEMM
//     per (block, T chunk, 64 x 64 tile) over the stored records, into the per-chunk partials
//     that em_adam_kernel folds in a fixed order.
// Taken when the plan admits the shape (emlayout.h: sw_fits); otherwise, and under engine option
// em_seq_sweep = 0, em_seq_grad_kernel runs.
// diagnostic phase slots (FQ_DIAG, FQLPOP_EM_PROBE): 0 inputs, 26 LayerNorm statistics, 1
// normalise, 2-5 forward ops, 6-13 termination-predictor ops, 27 record stores, 14 next
// observation; backward: 28 record to LDS, 29 next record's loads, 15 barrier, 16 carry,
// 17-20 dX ops, 30 LayerNorm backward sums, 25 carry update

struct SwOp {
    const float* A;  // k-major [Kc][No] (No contiguous): W for a forward op, W^T for a dX op
    int Kc, No;      // contracted rows, outputs
};
// (the units of an op: sw_plan, emlayout.h)
// the wave's A fragments of op o: fr[j] = A[4 (ch cks + j) + lk][16 tile + li] (unguarded buffer
// loads: rows >= Kc read 0, a lane's column >= No feeds only its own discarded output row)
// wave-uniform values through readfirstlane: an op descriptor picked by run-time branches is
// not known to be uniform, and a buffer resource built from VGPRs puts every load of the
// chain in a waterfall loop
DEV int sw_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
DEV const float* sw_uniptr(const float* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (const float*)(((unsigned long long)hi << 32) | lo);
}
DEV void sw_load(SwOp o, float (&fr)[SW_FM]) {
    o.A = sw_uniptr(o.A);
    o.Kc = sw_uni(o.Kc);
    o.No = sw_uni(o.No);
    int ntile, S, cks;
    sw_plan(o.Kc, o.No, ntile, S, cks);
    const int w = sw_uni(threadIdx.x >> 6), lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    if (w >= ntile * S) return;  // (a wave without a unit loads nothing: see sw_chain)
    const int tile = w % ntile, ch = w / ntile;
    const rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)o.A, (short)0, o.Kc * o.No * 4, 0x00020000);
    const int voff = ((4 * ch * cks + lk) * o.No + 16 * tile + li) * 4, sstep = 16 * o.No;
#pragma unroll
    for (int j = 0; j < SW_FM; ++j)
        fr[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rA, voff, j < cks ? j * sstep : 0x40000000, 0));
}
// One unit's MFMA chain (C) over all SW_FM slots, with slot j refilled with the next op's
// fragment right behind the MFMA that consumed it (L).  All or nothing, on both sides: a wave
// with a unit in the next op loads every slot and then reads every slot, a wave without one
// does neither.  (A load whose result is never read leaves its register free for the
// allocator while the load is in flight, and the next value put there must first wait for it
// (vmcnt counts in order): with per-op slot counts the chain ran at L2 latency per few MFMAs,
// and per-count code paths were merged by the compiler into one with the slots in scratch.)
// No branch around a load: slots j >= ck2 of the next op are loaded from past the buffer's
// range (an SGPR offset beyond num_records: they read exact zeros) and then read by an empty
// asm instead of an MFMA; rows >= Kc read zeros the same way, and x is read unconditionally
// (past the operand: other, initialised LDS buffers, times a zero fragment).  Even and odd
// slots are two independent chains, summed at the end.
template <bool C, bool L>
DEV void sw_chain(float (&fr)[SW_FM], f32x4& acc, const float* xl, int cks, rsrc_t rN, int voff, int sstep, int ck2) {
    f32x4 odd = f32x4{0.f, 0.f, 0.f, 0.f};
    // groups of 4 slots: one wave-uniform branch per group (past the chunk: no MFMA), the group's
    // 4 x reads issued together (a branch per slot kept every x read in front of its own MFMA,
    // one exposed LDS latency each); slots j >= cks inside a live group hold zero fragments
#pragma unroll
    for (int g = 0; g < SW_FM / 4; ++g) {
        if (C) {
            if (4 * g < cks) {
                float xv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) xv[q] = xl[4 * (4 * g + q) * R];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q & 1) odd = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[4 * g + q], xv[q], odd, 0, 0, 0);
                    else acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[4 * g + q], xv[q], acc, 0, 0, 0);
                }
            } else {  // the slots' (zero) loads are read: see above
                asm volatile("" ::"v"(fr[4 * g]), "v"(fr[4 * g + 1]), "v"(fr[4 * g + 2]), "v"(fr[4 * g + 3]));
            }
        }
        if (L) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = 4 * g + q;
                fr[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                      rN, voff, j < ck2 ? j * sstep : 0x40000000, 0));
            }
        }
    }
    if (C) acc = acc + odd;
}
// y[m][c] = act(sum_k A[k][m] x[k][c] + bias[m]), m < No, c < R; mode 0 linear, 1 ReLU, 2 zero
// where mask[m][c] <= 0 (relu' of a hidden layer's output); x, y, mask, scr in LDS.  fr holds
// this op's fragments on entry and the next op's (nx) on exit, so the next op's L2 latency
// hides under this op's chain
DEV void sw_compute(SwOp o, SwOp nx, float (&fr)[SW_FM], const float* bias, const float* x, float* y, int mode,
                    const float* mask, float* scr) {
    o.A = sw_uniptr(o.A);
    o.Kc = sw_uni(o.Kc);
    o.No = sw_uni(o.No);
    nx.A = sw_uniptr(nx.A);
    nx.Kc = sw_uni(nx.Kc);
    nx.No = sw_uni(nx.No);
    if (bias) bias = sw_uniptr(bias);
    x = lds_ptr(x);
    y = lds_ptr(y);
    scr = lds_ptr(scr);
    if (mask) mask = lds_ptr(mask);
    int ntile, S, cks, nt2, S2, ck2;
    sw_plan(o.Kc, o.No, ntile, S, cks);
    sw_plan(nx.Kc, nx.No, nt2, S2, ck2);
    const int tid = threadIdx.x, w = sw_uni(tid >> 6), lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const bool mine = w < ntile * S;
    const int tile = mine ? w % ntile : 0, ch = mine ? w / ntile : 0;
    const int u2 = w < nt2 * S2 ? w : 0;
    const int tile2 = u2 % nt2, chn = u2 / nt2;
    const rsrc_t rN = __builtin_amdgcn_make_buffer_rsrc((void*)nx.A, (short)0, nx.Kc * nx.No * 4, 0x00020000);
    // the bias values this thread adds, loaded before the refills: a wait for a load issued
    // after them would also wait for every refill in flight (vmcnt counts in order)
    // (S == 1: the lane's 4 outputs 16 tile + 4 lk + r; S > 1: output (tid + i SW_NT) / R of the
    // reduction pass; outputs >= No read 0)
    float bq[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias) {
        const rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)bias, (short)0, o.No * 4, 0x00020000);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            bq[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                  rB, (S == 1 ? 16 * tile + 4 * lk + i : (tid + i * SW_NT) / R) * 4, 0, 0));
    }
    // one address VGPR per operand: the k-step part of every offset is wave-uniform (the load's
    // SGPR offset; the LDS read's immediate)
    const int voff = ((4 * chn * ck2 + lk) * nx.No + 16 * tile2 + li) * 4, sstep = 16 * nx.No;
    const float* xl = x + (4 * ch * cks + lk) * R + li;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool mine2 = w < nt2 * S2;
    if (mine && mine2) sw_chain<true, true>(fr, acc, xl, cks, rN, voff, sstep, ck2);
    else if (mine) sw_chain<true, false>(fr, acc, xl, cks, rN, voff, sstep, ck2);
    else if (mine2) sw_chain<false, true>(fr, acc, xl, cks, rN, voff, sstep, ck2);
    if (mine) {
        // acc[r]: output m = 16 tile + 4 lk + r, column li
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 16 * tile + 4 * lk + r;
            if (S == 1) {
                if (m < o.No) {
                    float v = acc[r] + bq[r];
                    if (mode == 1) v = fmaxf(v, 0.f);
                    if (mode == 2 && !(mask[m * R + li] > 0.f)) v = 0.f;
                    y[m * R + li] = v;
                }
            } else {
                scr[(ch * ntile * 16 + m) * R + li] = acc[r];
            }
        }
    }
    __syncthreads();
    if (S > 1) {  // (No <= 128 here: ntile S <= 16 with S >= 2; q < 4 SW_NT)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + i * SW_NT;
            if (q < o.No * R) {
                const int m = q / R, c = q % R;
                float v = scr[m * R + c];
                for (int c2 = 1; c2 < S; ++c2) v += scr[(c2 * ntile * 16 + m) * R + c];
                v += bq[i];
                if (mode == 1) v = fmaxf(v, 0.f);
                if (mode == 2 && !(mask[q] > 0.f)) v = 0.f;
                y[q] = v;
            }
        }
        __syncthreads();
    }
    // every bias value is read (no load result left dead in flight: see sw_chain)
    asm volatile("" ::"v"(bq[0]), "v"(bq[1]), "v"(bq[2]), "v"(bq[3]));
}

// threadIdx.x through an opaque copy: per-thread addresses derived from it inside a time loop
// are recomputed where used instead of hoisted out of the loop and spilled (each spill reload
// was a vmcnt(0) that also waited for the next op's fragment refills)
DEV int opaque_tid() {
    int v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "v"((int)threadIdx.x));
    return v;
}

// LDS: em_lds, with SW_STATIC_LDS pinned to the __shared__ arrays below; records: em_rec.  Two
// forms are kept for speed (profiles/emlayout/sweep_variants.txt): layer buffers step an LDS
// pointer through em_layer (an offset added to the base at every use: + 1.2 %), and the backward
// walks g(n-1) .. g(0) with a running pointer from rec.g0 (em_rec_g per op: + 1.5 %).
__global__ __launch_bounds__(SW_NT) void em_sweep_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float lsum[NLOG][R];
    __shared__ float lab[R];
    __shared__ long long rowbase[R];
    __shared__ float mu_s[R], rs_s[R], cs[2][R];
    static_assert(sizeof(lsum) + sizeof(lab) + sizeof(rowbase) + sizeof(mu_s) + sizeof(rs_s) + sizeof(cs) + SW_PH_LDS ==
                      SW_STATIC_LDS, "SW_STATIC_LDS sums em_sweep_kernel's __shared__ arrays");
    ModelView mv;
    if (!ens_enter(a, mv)) return;
    const int tid = threadIdx.x, blk = mv.blk;
#ifdef FQ_DIAG  // phase times of block 0 (s_memrealtime, 100 MHz), summed over the steps
    __shared__ unsigned long long ph[EM_PH_N];
    static_assert(sizeof(ph) == SW_PH_LDS, "SW_PH_LDS is ph");
    unsigned long long ph_prev = 0;
    const bool ph_on = a.probe != nullptr && blockIdx.x == 0;
    if (ph_on && tid < EM_PH_N) ph[tid] = 0;
    auto stamp = [&](int i) {
        if (ph_on && threadIdx.x == 0) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (i >= 0) ph[i] += now - ph_prev;
            ph_prev = now;
        }
    };
#else
    auto stamp = [](int) {};
#endif
    const Net& N = a.net;
    const Net& TP = a.tpn;
    const int D = a.D, A = a.A, T = a.T, n = N.n, m = TP.n;  // (m == 0 when tw == 0: em_lds)
    const int K0 = N.dims[0];
    const EmLds L = em_lds(N, TP, D, true, true);
    const EmRec rc = em_rec(N, D, true);
    float* x0 = lds + L.x0;
    float* xhat = lds + L.xhat;
    // (layer buffers by summed widths: a runtime-indexed array of LDS pointers went to scratch)
    float* const acts0 = lds + L.acts0;
    float* const tacts0 = lds + L.tacts0;
    auto acts = [&](int i) { return lds_ptr(em_layer(acts0, N, i)); };
    auto tacts = [&](int i) { return lds_ptr(em_layer(tacts0, TP, i)); };
    float* gA = lds + L.gA;
    float* gB = lds + L.gB;
    float* gC = lds + L.gC;
    float* nobs = lds + L.nobs;
    float* carry = lds + L.carry;
    float* scr = lds + L.scr;
    float* lnacc = lds + L.lnacc;  // [2][K0] LayerNorm grad sums over t
    float* lnp = lds + L.lnp;      // [2][K0] LayerNorm scale, bias (no global load inside the sweeps)

    if (tid < R) rowbase[tid] = em_window(a, mv, blk * R + tid);
    // every LDS float finite before the first op: a chain reads x past its operand (times zeros)
    for (int q = tid; q < L.lnp; q += SW_NT) lds[q] = 0.f;
    for (int q = tid; q < NLOG * R; q += SW_NT) lsum[q / R][q % R] = 0.f;
    for (int q = tid; q < 2 * K0; q += SW_NT) {
        lnacc[q] = 0.f;
        lnp[q] = q < K0 ? mv.params[a.net.ln_scale + q] : mv.params[a.net.ln_bias + q - K0];
    }
    __syncthreads();

    const float* P = mv.params;
    const float norm = 1.0f + a.tw;
    const float inv_n = 1.0f / ((float)a.B * (float)T);
    const float gscale = 2.0f / ((float)a.B * (float)T * D) / norm;
    float* const sq = mv.seq + (long long)blk * T * a.seq_stride;
    const int act_floats = rc.own - rc.acts0;

    // ---- the forward sweep's op program: n layers, then (tw > 0) the frozen termination
    // predictor's m layers and its m dX ops
    const int nfw = n + 2 * m;
    auto fw_op = [&](int j) -> SwOp {
        if (j < n) return SwOp{P + N.w[j], N.dims[j], N.dims[j + 1]};
        if (j < n + m) return SwOp{a.tp + TP.w[j - n], TP.dims[j - n], TP.dims[j - n + 1]};
        const int i = m - 1 - (j - n - m);
        return SwOp{a.tpt + TP.w[i], TP.dims[i + 1], TP.dims[i]};
    };
    float fr[SW_FM];
    sw_load(fw_op(0), fr);
    // the next step's input rows (actions; observations at t = 0 only; next observations; rewards),
    // one value per thread, loaded a step ahead
    const int nin = (A + D + 1) * R;  // <= SW_NT: sw_fits admits no shape that needs a second value per thread
    auto in_load = [&](int t, int tid) -> float {
        if (tid >= nin || t >= T) return 0.f;
        const int r = tid % R, f = tid / R;
        const long long row = rowbase[r] + t;
        if (f < A) return mv.act[row * A + f];
        if (f < A + D) return mv.nobs[row * D + (f - A)];
        return mv.rew[row];
    };
    float inx = in_load(0, tid);
    for (int q = tid; q < D * R; q += SW_NT) x0[q] = mv.obs[rowbase[q % R] * D + q / R];  // observations[:, 0]

    stamp(-1);
    for (int t = 0; t < T; ++t) {
        const int tid = opaque_tid();
        if (tid < nin) {
            const int r = tid % R, f = tid / R;
            if (f < A) x0[(D + f) * R + r] = inx;
            else if (f < A + D) nobs[(f - A) * R + r] = inx;
            else lab[r] = inx == 0.f ? 1.f : 0.f;
        }
        inx = in_load(t + 1, tid);
        __syncthreads();
        stamp(0);
        if (tid < R) ln_stats(x0, K0, tid, mu_s, rs_s);
        __syncthreads();
        stamp(26);
        for (int q = tid; q < K0 * R; q += SW_NT) {
            const int k = q / R, r = q % R;
            const float xh = (x0[q] - mu_s[r]) * rs_s[r];
            xhat[q] = xh;
            acts0[q] = xh * lnp[k] + lnp[K0 + k];
        }
        __syncthreads();
        stamp(1);
        float* src = gB;  // the termination predictor's backward ping-pong
        float* dst = gC;
        for (int j = 0; j < nfw; ++j) {
            const SwOp o = fw_op(j), on = fw_op(j + 1 < nfw ? j + 1 : 0);  // (past the last op: the next step's first)
            if (j < n) {
                sw_compute(o, on, fr, P + N.b[j], acts(j), acts(j + 1), j < n - 1 ? 1 : 0, nullptr, scr);
                if (j == n - 1) {
                    // pred = out + obs; MSE; d loss / d pred (gA); the termination predictor's input
                    pred_loss<SW_NT>(acts(n), x0, nobs, tacts(0), true, gA, D, gscale, lsum[0], tid);
                }
            } else if (j < n + m) {
                const int i = j - n;
                sw_compute(o, on, fr, a.tp + TP.b[i], tacts(i), tacts(i + 1), i < m - 1 ? 1 : 0, nullptr, scr);
                if (i == m - 1) {  // weighted BCE of the logit (tp_score)
                    if (tid < R) {
                        const float x = tacts(m)[tid], z = lab[tid], w = a.ttw;
                        const float ce = softplus(x) - x * z;
                        lsum[1][tid] += (z > 0.f ? w * ce : ce) / (w + 1.f);
                        lsum[2][tid] += z > 0.f ? ce : 0.f;
                        lsum[3][tid] += z > 0.f ? 0.f : ce;
                        lsum[4][tid] += z;
                        lsum[5][tid] += 1.f - z;
                        const float p = 1.0f / (1.0f + expf(-x));
                        src[tid] = (z > 0.f ? w : 1.f) / (w + 1.f) * (p - z) * inv_n;
                    }
                    __syncthreads();
                }
            } else {
                const int i = m - 1 - (j - n - m);
                sw_compute(o, on, fr, nullptr, src, dst, i > 0 ? 2 : 0, i > 0 ? tacts(i) : nullptr, scr);
                float* tmp = src;
                src = dst;
                dst = tmp;
                if (i == 0) {
                    const float* sp = lds_ptr(src);
                    for (int q = tid; q < D * R; q += SW_NT) gA[q] += a.tw / norm * sp[q];
                    __syncthreads();
                }
            }
            stamp(2 + min(j, 11));
        }
        if (a.train) {
            float* st = sq + (long long)t * a.seq_stride;
            for (int q = tid; q < K0 * R; q += SW_NT) st[rc.xhat + q] = xhat[q];
            if (tid < R) st[rc.rstd + tid] = rs_s[tid];
            float* sa = st + rc.acts0;
            for (int q = tid; q < act_floats; q += SW_NT) sa[q] = acts0[q];  // acts[0..n-1] contiguous
            float* sg = st + rc.own;
            for (int q = tid; q < D * R; q += SW_NT) sg[q] = gA[q];
        }
        stamp(27);
        const float* pred = tacts(0);
        for (int q = tid; q < D * R; q += SW_NT) x0[q] = pred[q];  // the next step's observation
        __syncthreads();
        stamp(14);
    }
    if (tid < NLOG) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += lsum[tid][r];
        mv.logs[(long long)blk * NLOG + tid] = s;
    }
    if (!a.train) return;
    // the backward reads records other threads stored (the last one just now): every store of
    // the forward sweep complete before any wave goes on (__syncthreads waits for LDS only)
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();

    // ---- the backward sweep: dX chain, LayerNorm backward and carry, t = T-1 .. 0
    auto bw_op = [&](int j) -> SwOp {  // j = 0..n-1: layer n-1-j's dX from W^T
        const int i = n - 1 - j;
        return SwOp{mv.wt + N.w[i], N.dims[i + 1], N.dims[i]};
    };
    sw_load(bw_op(0), fr);
    // the step's record (xhat | rstd | acts[1..n-1] for the masks | own output gradient), a step
    // ahead in registers (RQ per thread), then into LDS at the step's start
    constexpr int RQ = SW_RQ;
    const int n_rec = rc.g0;
    float rec[RQ];
    auto rec_load = [&](int t, int tid) {
        const float* st = sq + (long long)max(t, 0) * a.seq_stride;
#pragma unroll
        for (int j = 0; j < RQ; ++j) rec[j] = st[min(tid + j * SW_NT, n_rec - 1)];
    };
    rec_load(T - 1, tid);
    for (int t = T - 1; t >= 0; --t) {
        const int tid = opaque_tid();
        float* st = sq + (long long)t * a.seq_stride;
        {
            float* const a0 = acts0;
            const int n1 = rc.rstd, n2 = rc.acts0, n3 = rc.own;
#pragma unroll
            for (int j = 0; j < RQ; ++j) {
                const int q = tid + j * SW_NT;
                if (q < n1) xhat[q] = rec[j];
                else if (q < n2) rs_s[q - n1] = rec[j];
                else if (q < n3) a0[q - n2] = rec[j];
                else if (q < n_rec) gA[q - n3] = rec[j];
            }
        }
        stamp(28);
        rec_load(t - 1, tid);
        stamp(29);
        __syncthreads();
        stamp(15);
        for (int q = tid; q < D * R; q += SW_NT) {
            const float gv = gA[q] + (t < T - 1 ? carry[q] : 0.f);
            gA[q] = gv;
            carry[q] = gv;  // the residual path: pred_t = out_t + obs_t
        }
        __syncthreads();
        stamp(16);
        float* g = gA;
        float* gn = gB;
        float* sgi = st + rc.g0;  // g(n-1) first, then each layer below it: em_rec_g
        for (int j = 0; j < n; ++j) {
            const int i = n - 1 - j;
            for (int q = tid; q < N.dims[i + 1] * R; q += SW_NT) sgi[q] = lds_ptr(g)[q];  // g_i for dW
            sgi += N.dims[i + 1] * R;
            sw_compute(bw_op(j), bw_op(j + 1 < n ? j + 1 : 0), fr, nullptr, g, gn, i > 0 ? 2 : 0,
                       i > 0 ? acts(i) : nullptr, scr);
            float* tmp = g;
            g = gn;
            gn = tmp;
            stamp(17 + min(j, 7));
        }
        // g = grad w.r.t. the LayerNorm output [K0][R]
        g = lds_ptr(g);
        if (tid < K0) {
            float ss = 0.f, sb = 0.f;
            for (int r = 0; r < R; ++r) {
                ss += g[tid * R + r] * xhat[tid * R + r];
                sb += g[tid * R + r];
            }
            lnacc[tid] += ss;
            lnacc[K0 + tid] += sb;
        }
        if (tid < R) {
            float c1 = 0.f, c2 = 0.f;
            for (int k = 0; k < K0; ++k) {
                const float gy = g[k * R + tid] * lnp[k];
                c1 += gy;
                c2 += gy * xhat[k * R + tid];
            }
            cs[0][tid] = c1 / K0;
            cs[1][tid] = c2 / K0;
        }
        __syncthreads();
        stamp(30);
        for (int q = tid; q < D * R; q += SW_NT) {
            const int k = q / R, r = q % R;
            carry[q] += rs_s[r] * (g[q] * lnp[k] - cs[0][r] - xhat[q] * cs[1][r]);
        }
        __syncthreads();
        stamp(25);
    }
#ifdef FQ_DIAG
    if (ph_on && tid < EM_PH_N) a.probe[tid] += ph[tid];
#endif
    // LayerNorm grads into T chunk 0's partials (the other chunks' are zero: em_seq_dw_kernel
    // writes the Dense leaves of every chunk)
    for (int c = 0; c < a.tchunks; ++c) {
        float* pg = mv.part + (long long)(blk * a.tchunks + c) * a.P;
        for (int k = tid; k < K0; k += SW_NT) {
            pg[N.ln_scale + k] = c == 0 ? lnacc[k] : 0.f;
            pg[N.ln_bias + k] = c == 0 ? lnacc[K0 + k] : 0.f;
        }
    }
}

// dW_i[k][f] = sum over the chunk's steps t and rows r of acts_i[t][k][r] g_i[t][f][r], db_i[f] =
// sum of g_i[t][f][r]; block = (sequence block b, T chunk c, layer i, 64 x 64 tile); 4 waves of
// 2 x 2 16 x 16 tiles (v_mfma_f32_16x16x4_f32, the contraction over the 16 rows of a step);
// each step's [64][R] operand slices staged through LDS, double-buffered
struct SeqDwArgs {
    const float* seq;
    long long seq_stride;
    float* part;
    long long P;
    Net net;
    int T, tchunks, D;
    int first[MAXL + 1];  // prefix of per-layer tile counts
    long long ens_seq, ens_part;  // floats between two models' record stores / partial sets
};
// grid: (blocks x tchunks x tiles, models); the model is blockIdx.y (wave-uniform by construction)
__global__ __launch_bounds__(256) void em_seq_dw_kernel(const SeqDwArgs a) {
    __shared__ __attribute__((aligned(16))) float As[2][64 * R], Bs[2][64 * R];
    const float* const mseq = a.seq + blockIdx.y * a.ens_seq;
    float* const mpart = a.part + blockIdx.y * a.ens_part;
    const int per = a.first[a.net.n];
    const int bc = blockIdx.x / per, tl = blockIdx.x % per;  // bc = b tchunks + c
    const int b = bc / a.tchunks, c = bc % a.tchunks;
    int i = 0;
    while (i + 1 < a.net.n && tl >= a.first[i + 1]) ++i;
    const int K = a.net.dims[i], Nn = a.net.dims[i + 1];
    const int tf = (Nn + 63) / 64, lt = tl - a.first[i];
    const int k0 = 64 * (lt / tf), f0 = 64 * (lt % tf);
    // offsets of acts_i and g_i inside a record
    const EmRec rc = em_rec(a.net, a.D, true);
    const int oa = em_rec_acts(rc, a.net, i), og = em_rec_g(rc, a.net, i);
    const int t0 = a.T * c / a.tchunks, t1 = a.T * (c + 1) / a.tchunks;
    const float* sq = mseq + (long long)b * a.T * a.seq_stride;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int wk = (w >> 1) * 32, wf = (w & 1) * 32;
    // staging: thread -> one float4 of each slice ([64][R] = 256 float4); rows past K / N read as 0
    const int sr = tid >> 2, sc = (tid & 3) * 4;
    auto ld = [&](int t, float4& va, float4& vb) {
        const float* st = sq + (long long)t * a.seq_stride;
        va = k0 + sr < K ? *reinterpret_cast<const float4*>(st + oa + (k0 + sr) * R + sc) : float4{0.f, 0.f, 0.f, 0.f};
        vb = f0 + sr < Nn ? *reinterpret_cast<const float4*>(st + og + (f0 + sr) * R + sc) : float4{0.f, 0.f, 0.f, 0.f};
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    float4 va, vb;
    ld(t0, va, vb);
    *reinterpret_cast<float4*>(&As[0][sr * R + sc]) = va;
    *reinterpret_cast<float4*>(&Bs[0][sr * R + sc]) = vb;
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const int cur = (t - t0) & 1;
        if (t + 1 < t1) ld(t + 1, va, vb);
        const float* Ac = As[cur];
        const float* Bc = Bs[cur];
#pragma unroll
        for (int s = 0; s < R / 4; ++s) {
            float av[2], bv[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) av[x] = Ac[(wk + 16 * x + li) * R + 4 * s + lk];
#pragma unroll
            for (int y = 0; y < 2; ++y) bv[y] = Bc[(wf + 16 * y + li) * R + 4 * s + lk];
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[x], bv[y], acc[x][y], 0, 0, 0);
        }
        if (k0 == 0 && tid < 64) {
            const float4* row = reinterpret_cast<const float4*>(&Bc[tid * R]);
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < R / 4; ++q) s += row[q].x + row[q].y + row[q].z + row[q].w;
            bsum += s;
        }
        if (t + 1 < t1) {
            *reinterpret_cast<float4*>(&As[cur ^ 1][sr * R + sc]) = va;
            *reinterpret_cast<float4*>(&Bs[cur ^ 1][sr * R + sc]) = vb;
        }
        __syncthreads();
    }
    float* pg = mpart + (long long)bc * a.P;
    // acc[x][y][r]: k = k0 + wk + 16 x + 4 lk + r, f = f0 + wf + 16 y + li
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0 + wk + 16 * x + 4 * lk + r, f = f0 + wf + 16 * y + li;
                if (k < K && f < Nn) pg[a.net.w[i] + (long long)k * Nn + f] = acc[x][y][r];
            }
    if (k0 == 0 && tid < 64 && f0 + tid < Nn) pg[a.net.b[i] + f0 + tid] = bsum;
}

struct AdamArgsEm {
    float* params;
    float* wt;                          // W^T copy, refreshed with the update
    Net net;
    float *m, *v;
    const float* part;
    long long P;
    int blocks;
    float lr, bc1, bc2;
    long long ens_par, ens_part;        // floats between two models' params / wt / m / v, partial sets
};

// Fixed-order sum of the block partials + optax.adam.  grid: (P / 256, models); the model is
// blockIdx.y, and a model's partials fold in the same block order whatever runs beside it.
__global__ __launch_bounds__(256) void em_adam_kernel(const AdamArgsEm a) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.P) return;
    const long long mo = blockIdx.y * a.ens_par;
    const float* part = a.part + blockIdx.y * a.ens_part;
    float* params = a.params + mo;
    float* wt = a.wt + mo;
    float* am = a.m + mo;
    float* av = a.v + mo;
    float g = 0.f;
    for (int b = 0; b < a.blocks; ++b) g += part[(long long)b * a.P + p];
    const float m = 0.1f * g + 0.9f * am[p];
    const float v = 0.001f * (g * g) + 0.999f * av[p];
    am[p] = m;
    av[p] = v;
    const float np = params[p] + (-a.lr) * ((m / a.bc1) / (sqrtf(v / a.bc2) + 1e-8f));
    params[p] = np;
    for (int i = 0; i < a.net.n; ++i) {
        const long long o = p - a.net.w[i];
        const int K = a.net.dims[i], N = a.net.dims[i + 1];
        if (o >= 0 && o < (long long)K * N) wt[a.net.w[i] + (o % N) * K + o / N] = np;
    }
}

// ------------------------------------------------ bootstrap tables (set-up) --
// Once per fqlpop_emtrain_set_bootstrap*, for all K models at a time: fill (grid.y = model),
// mark (likewise), compact (one block per model).  Nothing here is on the step's path.
struct BootArgs {
    long long* table;                   // [K][n]
    unsigned char* seen;                // [K][n]
    long long n;                        // n_units
    uint64_t seeds[ENS_MAX];
};

// table[k][i] = (x1 << 32 | x0) mod n of Philox(key seeds[k], counter (lo32 i, hi32 i, SALT_BOOT, 0))
__global__ __launch_bounds__(256) void em_boot_fill_kernel(const BootArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t seed = a.seeds[blockIdx.y];
    uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), SALT_BOOT, 0u};
    philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    a.table[blockIdx.y * a.n + i] = (long long)((((uint64_t)c[1] << 32) | c[0]) % (uint64_t)a.n);
}

// seen[k][table[k][i]] = 1 (seen starts zeroed).  Every writer of a byte stores the same value,
// so the stores need no order among themselves.  Table entries are in [0, n): drawn mod n, or
// checked by the host before the upload.
__global__ __launch_bounds__(256) void em_oob_mark_kernel(const BootArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const long long base = blockIdx.y * a.n;
    a.seen[base + a.table[base + i]] = 1;
}

// oob[k] = the units with seen[k][.] == 0, ascending; n_oob[k] = how many.  One block per model
// walks the units in chunks of OOB_NT x OOB_PER; a thread owns OOB_PER neighbours, and a
// block-wide exclusive scan of the threads' counts (wave scan, then the wave totals) places
// them.  At most n entries are written: the list cannot be longer than the units.
constexpr int OOB_NT = 1024, OOB_PER = 4;
__global__ __launch_bounds__(OOB_NT) void em_oob_compact_kernel(const unsigned char* seen, long long* oob,
                                                                 long long* n_oob, long long n) {
    __shared__ int wsum[OOB_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    seen += blockIdx.x * n;
    oob += blockIdx.x * n;
    long long base = 0;  // (every thread keeps the same count)
    for (long long c0 = 0; c0 < n; c0 += OOB_NT * OOB_PER) {
        const long long i0 = c0 + (long long)tid * OOB_PER;
        bool out[OOB_PER];
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < OOB_PER; ++q) {
            out[q] = i0 + q < n && seen[i0 + q] == 0;
            cnt += out[q] ? 1 : 0;
        }
        int inc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int before = 0, total = 0;
        for (int j = 0; j < OOB_NT / 64; ++j) {
            const int s = wsum[j];
            if (j < w) before += s;
            total += s;
        }
        long long o = base + before + inc - cnt;
#pragma unroll
        for (int q = 0; q < OOB_PER; ++q)
            if (out[q]) oob[o++] = i0 + q;
        base += total;
        __syncthreads();  // wsum is rewritten by the next chunk
    }
    if (tid == 0) n_oob[blockIdx.x] = base;
}

// One model's logs [FQLPOP_EM_LOG_STRIDE] from its per-block sums lg (layout: include/fqlpop.h).
// On the host for the log reads, on the device for fqlpop_emtrain_eval_oob: the same double
// arithmetic, every product and sum rounded on its own, so the two agree to the bit.
struct LogShape {
    int blocks, kind;
    double B, D, tw;                    // scored predictions, obs_dim, termination_weight
};
__host__ __device__ inline void em_logs_calc(const LogShape& h, const float* lg, float* out) {
#pragma clang fp contract(off)
    double s[NLOG] = {0};
    for (int b = 0; b < h.blocks; ++b)
        for (int k = 0; k < NLOG; ++k) s[k] += lg[(size_t)b * NLOG + k];
    const double B = h.B, D = h.D;
    for (int k = 0; k < FQLPOP_EM_LOG_STRIDE; ++k) out[k] = 0.f;
    if (h.kind != FQLPOP_EM_TERMINATION) {
        const double mse = s[0] / (B * D), tw = h.tw;
        const double tl = tw > 0 ? s[1] / B : 0.0;
        out[0] = (float)((mse + tw * tl) / (1.0 + tw));
        out[1] = (float)mse;
        out[2] = (float)tl;
        out[3] = (float)(s[4] > 0 ? s[2] / s[4] : NAN);
        out[4] = (float)(s[5] > 0 ? s[3] / s[5] : NAN);
    } else {
        out[0] = (float)(s[1] / B);
        out[1] = (float)(s[2] / (s[4] + 1e-8));
        out[2] = (float)(s[3] / (s[5] + 1e-8));
        out[3] = (float)(s[6] / B);
        out[4] = (float)(s[8] > 0 ? s[7] / s[8] : 1.0);
        out[5] = (float)(s[4] > 0 ? s[7] / s[4] : 1.0);
    }
}

// fqlpop_emtrain_eval_oob, after batch j of n: thread k adds model k's logs of that batch to
// acc[k] (float32, in batch order) and divides by n after the last.
struct OobAccArgs {
    LogShape shape;
    const float* logs;                  // [K][blocks][NLOG] block sums of the batch just run
    long long ens_logs;
    float* acc;                         // [K][FQLPOP_EM_LOG_STRIDE]
    int K, j, n;
};
__global__ __launch_bounds__(64) void em_oob_acc_kernel(const OobAccArgs a) {
    const int k = threadIdx.x;
    if (k >= a.K) return;
    float out[FQLPOP_EM_LOG_STRIDE];
    em_logs_calc(a.shape, a.logs + k * a.ens_logs, out);
    float* acc = a.acc + k * FQLPOP_EM_LOG_STRIDE;
    for (int i = 0; i < FQLPOP_EM_LOG_STRIDE; ++i) {
        float v = a.j == 0 ? out[i] : acc[i] + out[i];
        if (a.j == a.n - 1) v /= (float)a.n;
        acc[i] = v;
    }
}

}  // namespace em
}  // namespace fq

// ===================================================================== ABI ==
using namespace fq;
using namespace fq::em;

namespace {
// Flat params with every Dense kernel [in][out] replaced by its transpose [out][in]
std::vector<float> transposed(const Net& n, const float* p, long long P) {
    std::vector<float> t(p, p + P);
    for (int i = 0; i < n.n; ++i) {
        const int K = n.dims[i], N = n.dims[i + 1];
        for (int k = 0; k < K; ++k)
            for (int f = 0; f < N; ++f) t[n.w[i] + (long long)f * K + k] = p[n.w[i] + (long long)k * N + f];
    }
    return t;
}
}  // namespace

struct fqlpop_emtrain {
    fqlpop_emtrain_config cfg{};
    int device = 0;
    Net net{}, tpn{};
    long long P = 0, PT = 0;
    DevBuf<float> params, m, v, part, logs;
    DevBuf<float> wt;                     // W^T copies (the backward's dX reads)
    struct Frozen {                       // the frozen termination predictor and its W^T copies
        DevBuf<float> tp, tpt;
    } frozen;
    struct Data {                         // the dataset (rows == 0, null pointers: none)
        DevBuf<float> obs, act, rew, nobs;
        long long rows = 0;
    } data;
    EmBootTables<> boot;                  // bootstrap tables over the dataset's units (empty: off)
    DevBuf<float> i_obs, i_act, i_rew, i_nobs;
    DevBuf<unsigned char> i_keep;
    long long count = 0;
    int blocks = 0;
    int lds_bytes = 0;
    int T = 1;                   // rows per sequence of a batch (FQLPOP_EM_MULTISTEP: sequence_length)
    DevBuf<float> seq;           // multistep: per-(block, step) activation store
    long long seq_stride = 0;
    HostBuf<unsigned long long> probe;    // diagnostic builds: sweep phase sums (mapped host memory)
    long long probe_launches = 0;
    bool sweep = false;          // multistep through em_sweep_kernel + em_seq_dw_kernel (sw_fits)
    int tchunks = 1;             // sweep: T chunks of the dW GEMM (partial sets per block)
    int sweep_lds = 0;
    // the model axis (fqlpop_emtrain_create_ensemble; 1 model, no remap for fqlpop_emtrain_create):
    // every per-model buffer above is [K] slices at these strides (floats; keep: bytes)
    int K = 1;
    int xcd = 0;                 // engine option em_ens_xcd at creation
    uint64_t seeds[ENS_MAX] = {};
    long long s_par = 0, s_part = 0, s_logs = 0, s_seq = 0, s_obs = 0, s_act = 0, s_rew = 0, s_keep = 0;
    Stream<> s;
};

extern "C" {

int fqlpop_emtrain_param_count(const fqlpop_emtrain_config* cfg, int64_t* n_params) {
    return guard([&] {
        ARGCHK(cfg && n_params, "null argument");
        Net a, b;
        long long P, PT;
        const char* why = em_nets(cfg, &a, &P, &b, &PT);
        ARGCHK(!why, why);
        *n_params = P;
    });
}

}  // extern "C"

// K models ([K][P] params, K seeds) behind one handle; K = 1, xcd = 0 is fqlpop_emtrain_create.
// Every refusal comes before the first GPU call.
static void em_create(const fqlpop_emtrain_config* cfg, int K, const float* params, int64_t n_params,
                      const uint64_t* seeds, int xcd, int device, fqlpop_emtrain_t** out) {
    {
        const EmPlan plan = em_plan(cfg, fq::engine_option_em_seq_sweep(), n_params, K);
        auto h = std::make_unique<fqlpop_emtrain>();
        h->cfg = *cfg;
        h->device = device;
        h->K = K;
        h->xcd = xcd;
        for (int k = 0; k < K; ++k) h->seeds[k] = seeds[k];
        h->cfg.seed = seeds[0];
        h->net = plan.net; h->tpn = plan.tpn; h->P = plan.P; h->PT = plan.PT;
        h->T = plan.T;
        h->lds_bytes = plan.lds_bytes;
        h->blocks = plan.blocks;
        h->sweep = plan.sweep; h->sweep_lds = plan.sweep_lds; h->tchunks = plan.tchunks;
        h->seq_stride = plan.seq_stride;
        const bool ms = cfg->kind == FQLPOP_EM_MULTISTEP;
        const long long P = h->P;
        const long long B = cfg->batch_size * (long long)h->T, D = cfg->obs_dim, A = cfg->action_dim;
        // per-model strides (a model's parameter block starts on a 256-byte boundary)
        h->s_par = K > 1 ? (P + 63) / 64 * 64 : P;
        h->s_part = P * h->blocks * h->tchunks;
        h->s_logs = (long long)NLOG * h->blocks;
        h->s_obs = B * D;
        h->s_act = B * A;
        h->s_rew = B;
        h->s_keep = B * D;
        h->s_seq = h->seq_stride * h->T * h->blocks;
        HIPCHK(hipSetDevice(device));
        h->s = Stream<>::create();
        const long long PK = h->s_par * K;
        h->params = DevBuf<float>(PK, "env-model parameters");
        h->m = DevBuf<float>(PK, "env-model Adam moments");
        h->v = DevBuf<float>(PK, "env-model Adam moments");
        h->part = DevBuf<float>(h->s_part * K, "env-model partial grads");
        h->logs = DevBuf<float>(h->s_logs * K);
        h->wt = DevBuf<float>(PK, "env-model parameters");
        HIPCHK(hipMemset(h->params, 0, 4 * PK));
        HIPCHK(hipMemset(h->wt, 0, 4 * PK));
        for (int k = 0; k < K; ++k) {
            const float* pk = params + (long long)k * P;
            HIPCHK(hipMemcpy(h->params + k * h->s_par, pk, 4 * P, hipMemcpyHostToDevice));
            const std::vector<float> wt = transposed(h->net, pk, P);
            HIPCHK(hipMemcpy(h->wt + k * h->s_par, wt.data(), 4 * P, hipMemcpyHostToDevice));
        }
        HIPCHK(hipMemset(h->m, 0, 4 * PK));
        HIPCHK(hipMemset(h->v, 0, 4 * PK));
        HIPCHK(hipMemset(h->logs, 0, 4 * h->s_logs * K));
        if (ms) {
            // the record store of every model (about 300 MB per model at B = T = 256, default widths)
            const std::string what = "multistep record store (" + std::to_string(K) + " models x " +
                                     std::to_string(4 * h->s_seq) + " bytes)";
            h->seq = DevBuf<float>(h->s_seq * K, what.c_str());
        }
        h->i_obs = DevBuf<float>(h->s_obs * K);
        h->i_act = DevBuf<float>(std::max(1LL, h->s_act * K));
        h->i_rew = DevBuf<float>(h->s_rew * K);
        h->i_nobs = DevBuf<float>(h->s_obs * K);
        h->i_keep = DevBuf<unsigned char>(h->s_keep * K);
        HIPCHK(hipFuncSetAttribute((const void*)em_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_bytes));
        HIPCHK(hipFuncSetAttribute((const void*)em_seq_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   h->lds_bytes));
        if (h->sweep)
            HIPCHK(hipFuncSetAttribute((const void*)em_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       h->sweep_lds));
#ifdef FQ_DIAG
        if (h->sweep && std::getenv("FQLPOP_EM_PROBE")) {
            h->probe = HostBuf<unsigned long long>(EM_PH_N, hipHostMallocMapped | hipHostMallocCoherent);
            std::memset(h->probe, 0, 8 * EM_PH_N);
        }
#endif
        *out = h.release();
    }
}

extern "C" {

int fqlpop_emtrain_create(const fqlpop_emtrain_config* cfg, const float* params, int64_t n_params, int device,
                          fqlpop_emtrain_t** out) {
    return guard([&] {
        ARGCHK(cfg && params && out, "null argument");
        em_create(cfg, 1, params, n_params, &cfg->seed, 0, device, out);
    });
}

int fqlpop_emtrain_create_ensemble(const fqlpop_emtrain_config* cfg, int n_models, const float* params,
                                   int64_t n_params, const uint64_t* seeds, int device, fqlpop_emtrain_t** out) {
    return guard([&] {
        ARGCHK(cfg && params && out, "null argument");
        ARGCHK(seeds, "null seeds: an ensemble takes one seed per model");
        ARGCHK(n_models >= 1 && n_models <= ENS_MAX, "n_models must be 1..16");
        em_create(cfg, n_models, params, n_params, seeds, fq::engine_option_em_ens_xcd(), device, out);
    });
}

int fqlpop_emtrain_num_models(fqlpop_emtrain_t* h, int* n_models) {
    return guard([&] {
        ARGCHK(h && n_models, "null argument");
        *n_models = h->K;
    });
}

int fqlpop_emtrain_ensemble_block_map(int n_models, int blocks_per_model, int xcd_mode, int linear_block,
                                      int* grid_blocks, int* model, int* block) {
    return guard([&] {
        ARGCHK(grid_blocks && model && block, "null argument");
        ARGCHK(n_models >= 1 && n_models <= ENS_MAX, "n_models must be 1..16");
        ARGCHK(blocks_per_model >= 1 && blocks_per_model <= (1 << 20), "blocks_per_model must be 1..2^20");
        ARGCHK(xcd_mode == 0 || xcd_mode == 1, "xcd_mode must be 0 or 1");
        int m = -1, b = -1;
        const int grid = ens_block_map(n_models, blocks_per_model, xcd_mode, 0, &m, &b);
        ARGCHK(linear_block >= 0 && linear_block < grid, "linear_block outside the grid");
        ens_block_map(n_models, blocks_per_model, xcd_mode, linear_block, &m, &b);
        *grid_blocks = grid;
        *model = m;
        *block = b;
    });
}

int fqlpop_emtrain_destroy(fqlpop_emtrain_t* h) {
    return guard([&] {
        if (!h) return;
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        if (h->probe) {  // diagnostic builds: mean phase times per step of the sweep (block 0)
            std::fprintf(stderr, "[em sweep phases, us per step, %lld launches, T %d]", h->probe_launches, h->T);
            for (int i = 0; i < EM_PH_N; ++i)
                if (h->probe[i])
                    std::fprintf(stderr, " %d:%.2f", i, h->probe[i] * 0.01 / ((double)h->probe_launches * h->T));
            std::fprintf(stderr, "\n");
        }
        delete h;
    });
}

int fqlpop_emtrain_set_frozen_termination(fqlpop_emtrain_t* h, const float* tp_params, int64_t n) {
    return guard([&] {
        ARGCHK(h && tp_params, "null argument");
        ARGCHK(h->PT > 0, "no frozen termination predictor in this config (termination_weight == 0)");
        ARGCHK(n == h->PT, "termination predictor size mismatch");
        HIPCHK(hipSetDevice(h->device));
        replace_built(h->frozen, [&] {
            fqlpop_emtrain::Frozen f{DevBuf<float>(h->PT), DevBuf<float>(h->PT)};
            HIPCHK(hipMemcpy(f.tp, tp_params, 4 * h->PT, hipMemcpyHostToDevice));
            const std::vector<float> tt = transposed(h->tpn, tp_params, h->PT);
            HIPCHK(hipMemcpy(f.tpt, tt.data(), 4 * h->PT, hipMemcpyHostToDevice));
            HIPCHK(hipStreamSynchronize(h->s));  // the current predictor's last reader has run
            return f;
        });
    });
}

int fqlpop_emtrain_set_dataset(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                               const float* next_obs, int64_t n_rows) {
    return guard([&] {
        ARGCHK(h && obs && rew && next_obs && (act || h->cfg.action_dim == 0), "null argument");
        ARGCHK(n_rows > 0, "n_rows must be > 0");
        if (h->cfg.kind == FQLPOP_EM_MULTISTEP)  // MultistepLoader reshapes to [n / episode_length][episode_length]
            ARGCHK(n_rows % h->cfg.episode_length == 0, "multistep: n_rows must be a multiple of episode_length");
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->s));
        const long long D = h->cfg.obs_dim, A = h->cfg.action_dim;
        replace_dataset(h->data, h->boot, [&] {
            fqlpop_emtrain::Data d;
            d.obs = DevBuf<float>(n_rows * D, "env-model dataset");
            d.act = DevBuf<float>(std::max(1LL, n_rows * A), "env-model dataset");
            d.rew = DevBuf<float>(n_rows, "env-model dataset");
            d.nobs = DevBuf<float>(n_rows * D, "env-model dataset");
            HIPCHK(hipMemcpy(d.obs, obs, 4 * n_rows * D, hipMemcpyHostToDevice));
            if (A) HIPCHK(hipMemcpy(d.act, act, 4 * n_rows * A, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d.rew, rew, 4 * n_rows, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d.nobs, next_obs, 4 * n_rows * D, hipMemcpyHostToDevice));
            d.rows = n_rows;
            return d;
        });
    });
}

// shared: an injected batch is one [B..] batch for every model (model stride 0)
static StepArgs em_args(fqlpop_emtrain* h, bool train, bool injected, bool shared = false) {
    const auto& c = h->cfg;
    StepArgs a{};
    a.ens.n_models = h->K;
    a.ens.bpm = h->blocks;
    a.ens.xcd = h->xcd;
    a.ens.par = h->s_par; a.ens.part = h->s_part; a.ens.logs = h->s_logs; a.ens.seq = h->s_seq;
    if (injected && !shared && h->K > 1) {
        a.ens.obs = h->s_obs; a.ens.act = h->s_act; a.ens.rew = h->s_rew; a.ens.keep = h->s_keep;
    }
    for (int k = 0; k < h->K; ++k) a.ens.seeds[k] = h->seeds[k];
    a.kind = c.kind;
    a.train = train ? 1 : 0;
    a.net = h->net;
    a.tpn = h->tpn;
    a.params = h->params;
    a.tp = h->frozen.tp;
    a.wt = h->wt;
    a.tpt = h->frozen.tpt;
    a.part = h->part;
    a.P = h->P;
    a.logs = h->logs;
    a.injected = injected ? 1 : 0;
    if (injected) {
        a.obs = h->i_obs; a.act = h->i_act; a.rew = h->i_rew; a.nobs = h->i_nobs;
        a.n_rows = (long long)c.batch_size * h->T;
    } else {
        a.obs = h->data.obs; a.act = h->data.act; a.rew = h->data.rew; a.nobs = h->data.nobs;
        a.n_rows = h->data.rows;
        if (h->boot) {
            a.tab = h->boot.table;
            a.tab_stride = h->boot.n_units;
        }
    }
    a.step = h->count;
    a.B = c.batch_size; a.D = c.obs_dim; a.A = c.action_dim;
    a.tw = c.kind != FQLPOP_EM_TERMINATION ? c.termination_weight : 0.f;
    a.T = h->T;
    a.ep_len = c.episode_length;
    a.seq = h->seq;
    a.seq_stride = h->seq_stride;
    a.tchunks = h->tchunks;
    if (h->probe && train) {
        unsigned long long* dp = nullptr;
        HIPCHK(hipHostGetDevicePointer((void**)&dp, h->probe, 0));
        a.probe = dp;
        ++h->probe_launches;
    }
    a.ttw = c.true_termination_weight;
    a.alpha = c.focal_alpha; a.gamma = c.focal_gamma; a.rate = c.dropout_rate;
    return a;
}

static void em_launch_step(fqlpop_emtrain* h, const StepArgs& a) {
    // K x blocks blocks through the block map (one model, no remap: the blocks themselves)
    int m0, b0;
    const unsigned grid = (unsigned)ens_block_map(h->K, h->blocks, h->xcd, 0, &m0, &b0);
    const unsigned K = (unsigned)h->K;
    if (h->sweep) {
        hipLaunchKernelGGL(em_sweep_kernel, dim3(grid), dim3(SW_NT), h->sweep_lds, h->s, a);
        HIPCHK(hipGetLastError());
        if (a.train) {
            SeqDwArgs d{};
            d.seq = h->seq; d.seq_stride = h->seq_stride; d.part = h->part; d.P = h->P; d.net = h->net;
            d.T = h->T; d.tchunks = h->tchunks; d.D = h->cfg.obs_dim;
            d.ens_seq = h->s_seq; d.ens_part = h->s_part;
            int tot = 0;
            for (int i = 0; i < h->net.n; ++i) {
                d.first[i] = tot;
                tot += ((h->net.dims[i] + 63) / 64) * ((h->net.dims[i + 1] + 63) / 64);
            }
            d.first[h->net.n] = tot;
            hipLaunchKernelGGL(em_seq_dw_kernel, dim3(h->blocks * h->tchunks * tot, K), dim3(256), 0, h->s, d);
        }
    } else if (h->cfg.kind == FQLPOP_EM_MULTISTEP) {
        hipLaunchKernelGGL(em_seq_grad_kernel, dim3(grid), dim3(NT), h->lds_bytes, h->s, a);
    } else {
        hipLaunchKernelGGL(em_grad_kernel, dim3(grid), dim3(NT), h->lds_bytes, h->s, a);
    }
    HIPCHK(hipGetLastError());
    if (!a.train) return;
    // optax.cosine_decay_schedule(init, steps)(count), adam bias correction with count + 1
    const auto& c = h->cfg;
    const double cc = (double)std::min<long long>(h->count, c.steps);
    AdamArgsEm ad{};
    ad.params = h->params; ad.wt = h->wt; ad.net = h->net; ad.m = h->m; ad.v = h->v; ad.part = h->part;
    ad.P = h->P; ad.blocks = h->blocks * h->tchunks;
    ad.ens_par = h->s_par; ad.ens_part = h->s_part;
    ad.lr = (float)(c.init_lr * 0.5 * (1.0 + std::cos(3.14159265358979323846 * cc / c.steps)));
    ad.bc1 = (float)(1.0 - std::pow(0.9, (double)(h->count + 1)));
    ad.bc2 = (float)(1.0 - std::pow(0.999, (double)(h->count + 1)));
    hipLaunchKernelGGL(em_adam_kernel, dim3((unsigned)((h->P + 255) / 256), K), dim3(256), 0, h->s, ad);
    HIPCHK(hipGetLastError());
    ++h->count;
}

static void em_check_ready(fqlpop_emtrain* h) {
    if (h->cfg.kind != FQLPOP_EM_TERMINATION && h->cfg.termination_weight > 0.f && !h->frozen.tp)
        throw Err{FQLPOP_E_STATE, "termination_weight > 0 needs fqlpop_emtrain_set_frozen_termination"};
}

int fqlpop_emtrain_step(fqlpop_emtrain_t* h, int n_steps) {
    return guard([&] {
        ARGCHK(h && n_steps >= 0, "bad argument");
        ARGCHK(h->data.rows > 0, "no dataset: call fqlpop_emtrain_set_dataset");
        em_check_ready(h);
        HIPCHK(hipSetDevice(h->device));
        for (int i = 0; i < n_steps; ++i) em_launch_step(h, em_args(h, true, false));
    });
}

// the single-model entry points refuse an ensemble handle, naming the call that serves it
#define EM_SINGLE(h, call) \
    ARGCHK((h)->K == 1, "this handle holds an ensemble of models: use " call)

// nb batches ([nb][B..] host arrays; 1: the one batch of a single model or a shared one) into
// the injected slots 0..nb-1
static void em_upload_batch(fqlpop_emtrain* h, const float* obs, const float* act, const float* rew,
                            const float* next_obs, int nb = 1) {
    ARGCHK(obs && rew && next_obs && (act || h->cfg.action_dim == 0), "null batch array");
    const long long B = (long long)h->cfg.batch_size * h->T * nb, D = h->cfg.obs_dim, A = h->cfg.action_dim;
    HIPCHK(hipMemcpyAsync(h->i_obs, obs, 4 * B * D, hipMemcpyHostToDevice, h->s));
    if (A) HIPCHK(hipMemcpyAsync(h->i_act, act, 4 * B * A, hipMemcpyHostToDevice, h->s));
    HIPCHK(hipMemcpyAsync(h->i_rew, rew, 4 * B, hipMemcpyHostToDevice, h->s));
    HIPCHK(hipMemcpyAsync(h->i_nobs, next_obs, 4 * B * D, hipMemcpyHostToDevice, h->s));
}

int fqlpop_emtrain_step_injected(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                                 const float* next_obs, const uint8_t* keep_mask) {
    return guard([&] {
        ARGCHK(h, "null handle");
        EM_SINGLE(h, "fqlpop_emtrain_step_injected_ensemble");
        em_check_ready(h);
        HIPCHK(hipSetDevice(h->device));
        em_upload_batch(h, obs, act, rew, next_obs);
        StepArgs a = em_args(h, true, true);
        if (keep_mask) {
            HIPCHK(hipMemcpyAsync(h->i_keep, keep_mask, (size_t)h->cfg.batch_size * h->cfg.obs_dim,
                                 hipMemcpyHostToDevice, h->s));
            a.keep = h->i_keep;
        }
        em_launch_step(h, a);
        HIPCHK(hipStreamSynchronize(h->s));  // host batch buffers are reused
    });
}

int fqlpop_emtrain_step_injected_ensemble(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                                          const float* next_obs, const uint8_t* keep_mask, int shared) {
    return guard([&] {
        ARGCHK(h, "null handle");
        ARGCHK(shared == 0 || shared == 1, "shared must be 0 or 1");
        em_check_ready(h);
        HIPCHK(hipSetDevice(h->device));
        const int nb = shared ? 1 : h->K;
        em_upload_batch(h, obs, act, rew, next_obs, nb);
        StepArgs a = em_args(h, true, true, shared != 0);
        if (keep_mask) {
            HIPCHK(hipMemcpyAsync(h->i_keep, keep_mask, (size_t)h->cfg.batch_size * h->cfg.obs_dim * nb,
                                 hipMemcpyHostToDevice, h->s));
            a.keep = h->i_keep;
        }
        em_launch_step(h, a);
        HIPCHK(hipStreamSynchronize(h->s));  // host batch buffers are reused
    });
}

// one model's logs [FQLPOP_EM_LOG_STRIDE] from its per-block sums lg (layout: include/fqlpop.h)
static LogShape em_log_shape(const fqlpop_emtrain* h) {
    return LogShape{h->blocks, h->cfg.kind, (double)h->cfg.batch_size * h->T, (double)h->cfg.obs_dim,
                    (double)h->cfg.termination_weight};
}
static void em_logs_model(const fqlpop_emtrain* h, const float* lg, float* out) {
    em_logs_calc(em_log_shape(h), lg, out);
}
// logs [K][FQLPOP_EM_LOG_STRIDE]: one copy and one synchronisation for all K models
static void em_logs(fqlpop_emtrain* h, float* out) {
    std::vector<float> lg((size_t)h->s_logs * h->K);
    HIPCHK(hipMemcpyAsync(lg.data(), h->logs, 4 * lg.size(), hipMemcpyDeviceToHost, h->s));
    HIPCHK(hipStreamSynchronize(h->s));
    for (int k = 0; k < h->K; ++k)
        em_logs_model(h, lg.data() + (size_t)k * h->s_logs, out + (size_t)k * FQLPOP_EM_LOG_STRIDE);
}

int fqlpop_emtrain_read_logs(fqlpop_emtrain_t* h, float* logs) {
    return guard([&] {
        ARGCHK(h && logs, "null argument");
        EM_SINGLE(h, "fqlpop_emtrain_read_logs_ensemble");
        HIPCHK(hipSetDevice(h->device));
        em_logs(h, logs);
    });
}

int fqlpop_emtrain_read_logs_ensemble(fqlpop_emtrain_t* h, float* logs) {
    return guard([&] {
        ARGCHK(h && logs, "null argument");
        HIPCHK(hipSetDevice(h->device));
        em_logs(h, logs);
    });
}

int fqlpop_emtrain_eval(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                        const float* next_obs, float* logs) {
    return guard([&] {
        ARGCHK(h && logs, "null argument");
        EM_SINGLE(h, "fqlpop_emtrain_eval_ensemble");
        em_check_ready(h);
        HIPCHK(hipSetDevice(h->device));
        em_upload_batch(h, obs, act, rew, next_obs);
        em_launch_step(h, em_args(h, false, true));
        em_logs(h, logs);
    });
}

int fqlpop_emtrain_eval_ensemble(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                                 const float* next_obs, int shared, float* logs) {
    return guard([&] {
        ARGCHK(h && logs, "null argument");
        ARGCHK(shared == 0 || shared == 1, "shared must be 0 or 1");
        em_check_ready(h);
        HIPCHK(hipSetDevice(h->device));
        em_upload_batch(h, obs, act, rew, next_obs, shared ? 1 : h->K);
        em_launch_step(h, em_args(h, false, true, shared != 0));
        em_logs(h, logs);
    });
}

static void em_get_params(fqlpop_emtrain* h, int model, int which, float* out, int64_t n) {
    ARGCHK(n == h->P, "params size mismatch");
    ARGCHK(which >= 0 && which <= 2, "which must be FQLPOP_STATE_PARAMS/ADAM_M/ADAM_V");
    HIPCHK(hipSetDevice(h->device));
    const float* src = (which == 0 ? h->params : which == 1 ? h->m : h->v) + model * h->s_par;
    HIPCHK(hipMemcpyAsync(out, src, 4 * n, hipMemcpyDeviceToHost, h->s));
    HIPCHK(hipStreamSynchronize(h->s));
}

int fqlpop_emtrain_get_params(fqlpop_emtrain_t* h, int which, float* out, int64_t n) {
    return guard([&] {
        ARGCHK(h && out, "null argument");
        EM_SINGLE(h, "fqlpop_emtrain_get_params_model");
        em_get_params(h, 0, which, out, n);
    });
}

int fqlpop_emtrain_get_params_model(fqlpop_emtrain_t* h, int model, int which, float* out, int64_t n) {
    return guard([&] {
        ARGCHK(h && out, "null argument");
        ARGCHK(model >= 0 && model < h->K, "model index out of range");
        em_get_params(h, model, which, out, n);
    });
}

int fqlpop_emtrain_get_count(fqlpop_emtrain_t* h, int64_t* count) {
    return guard([&] {
        ARGCHK(h && count, "null argument");
        *count = h->count;
    });
}

int fqlpop_emtrain_get_plan(fqlpop_emtrain_t* h, int* sweep, int* tchunks, int* blocks) {
    return guard([&] {
        ARGCHK(h, "null handle");
        if (sweep) *sweep = h->sweep ? 1 : 0;
        if (tchunks) *tchunks = h->tchunks;
        if (blocks) *blocks = h->blocks;
    });
}

int fqlpop_emtrain_sync(fqlpop_emtrain_t* h) {
    return guard([&] {
        ARGCHK(h, "null handle");
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->s));
    });
}

}  // extern "C"

// ------------------------------------------------------------- bootstrap ABI --
static long long em_n_units(const fqlpop_emtrain* h) {
    return h->cfg.kind == FQLPOP_EM_MULTISTEP ? h->data.rows / h->cfg.episode_length : h->data.rows;
}

// Fresh tables for the handle's dataset: `table` ([K][n_units], checked by the caller) uploaded,
// or drawn on the device when null; then the out-of-bag lists and their host-side counts.
static EmBootTables<> em_boot_build(fqlpop_emtrain* h, const int64_t* table) {
    static_assert(sizeof(int64_t) == sizeof(long long), "the tables are int64 on both sides of the ABI");
    const long long n = em_n_units(h);
    const int K = h->K;
    EmBootTables<> b = EmBootTables<>::make(K, n);
    BootArgs a{};
    a.table = b.table;
    a.seen = b.seen;
    a.n = n;
    for (int k = 0; k < K; ++k) a.seeds[k] = h->seeds[k];
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)K);
    if (table) {
        HIPCHK(hipMemcpyAsync(b.table, table, 8 * (size_t)K * n, hipMemcpyHostToDevice, h->s));
    } else {
        hipLaunchKernelGGL(em_boot_fill_kernel, grid, dim3(256), 0, h->s, a);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(b.seen, 0, (size_t)K * n, h->s));
    HIPCHK(hipMemsetAsync(b.oob, 0, 8 * (size_t)K * n, h->s));
    hipLaunchKernelGGL(em_oob_mark_kernel, grid, dim3(256), 0, h->s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(em_oob_compact_kernel, dim3((unsigned)K), dim3(OOB_NT), 0, h->s, b.seen.get(), b.oob.get(),
                       b.n_oob.get(), n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b.n_oob_h, b.n_oob, 8 * (size_t)K, hipMemcpyDeviceToHost, h->s));
    HIPCHK(hipStreamSynchronize(h->s));  // (also: the caller's table may be reused)
    return b;
}

extern "C" {

int fqlpop_emtrain_set_bootstrap(fqlpop_emtrain_t* h, int enable) {
    return guard([&] {
        ARGCHK(h, "null handle");
        ARGCHK(enable == 0 || enable == 1, "enable must be 0 or 1");
        if (h->data.rows <= 0) throw Err{FQLPOP_E_STATE, "no dataset: call fqlpop_emtrain_set_dataset"};
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->s));  // the current tables' last reader has run
        if (!enable) {
            h->boot = EmBootTables<>{};
            return;
        }
        replace_built(h->boot, [&] { return em_boot_build(h, nullptr); });
    });
}

int fqlpop_emtrain_set_bootstrap_table(fqlpop_emtrain_t* h, const int64_t* table, int64_t n) {
    return guard([&] {
        ARGCHK(h && table, "null argument");
        if (h->data.rows <= 0) throw Err{FQLPOP_E_STATE, "no dataset: call fqlpop_emtrain_set_dataset"};
        const long long nu = em_n_units(h);
        ARGCHK(n == nu * h->K, "bootstrap table size mismatch: n must be n_models * n_units");
        for (int64_t i = 0; i < n; ++i)
            if (table[i] < 0 || table[i] >= nu)
                throw Err{FQLPOP_E_ARG, "bootstrap table entry " + std::to_string(i) + " (" + std::to_string(table[i]) +
                                            ") is outside [0, " + std::to_string(nu) + ")"};
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->s));
        replace_built(h->boot, [&] { return em_boot_build(h, table); });
    });
}

int fqlpop_emtrain_get_bootstrap(fqlpop_emtrain_t* h, int model, int64_t* table, int64_t n_units, int64_t* oob,
                                 int64_t oob_cap, int64_t* n_oob) {
    return guard([&] {
        ARGCHK(h && table && n_oob, "null argument");
        if (!h->boot) throw Err{FQLPOP_E_STATE, "no bootstrap tables: call fqlpop_emtrain_set_bootstrap"};
        ARGCHK(model >= 0 && model < h->K, "model index out of range");
        ARGCHK(n_units == h->boot.n_units, "n_units mismatch");
        const long long no = h->boot.n_oob_h[model];
        ARGCHK(!oob || oob_cap >= no, "oob_cap is smaller than the model's out-of-bag list");
        HIPCHK(hipSetDevice(h->device));
        const long long off = (long long)model * n_units;
        HIPCHK(hipMemcpyAsync(table, h->boot.table + off, 8 * (size_t)n_units, hipMemcpyDeviceToHost, h->s));
        if (oob && no > 0) HIPCHK(hipMemcpyAsync(oob, h->boot.oob + off, 8 * (size_t)no, hipMemcpyDeviceToHost, h->s));
        HIPCHK(hipStreamSynchronize(h->s));
        *n_oob = no;
    });
}

int fqlpop_emtrain_eval_oob(fqlpop_emtrain_t* h, int n_batches, uint64_t draw, float* logs) {
    return guard([&] {
        ARGCHK(h && logs, "null argument");
        ARGCHK(n_batches >= 1, "n_batches must be >= 1");
        if (h->data.rows <= 0) throw Err{FQLPOP_E_STATE, "no dataset: call fqlpop_emtrain_set_dataset"};
        if (!h->boot) throw Err{FQLPOP_E_STATE, "no bootstrap tables: call fqlpop_emtrain_set_bootstrap"};
        for (int k = 0; k < h->K; ++k)
            if (h->boot.n_oob_h[k] == 0)
                throw Err{FQLPOP_E_STATE, "model " + std::to_string(k) + " has no out-of-bag unit: its table holds every one"};
        em_check_ready(h);
        HIPCHK(hipSetDevice(h->device));
        StepArgs a = em_args(h, false, false);
        a.tab = h->boot.oob;
        a.n_oob = h->boot.n_oob;
        a.oob_eval = 1;
        a.oob_draw = (uint32_t)draw;
        OobAccArgs r{};
        r.shape = em_log_shape(h);
        r.logs = h->logs;
        r.ens_logs = h->s_logs;
        r.acc = h->boot.acc;
        r.K = h->K;
        r.n = n_batches;
        for (int j = 0; j < n_batches; ++j) {
            a.oob_batch = (uint32_t)j;
            em_launch_step(h, a);
            r.j = j;
            hipLaunchKernelGGL(em_oob_acc_kernel, dim3(1), dim3(64), 0, h->s, r);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(logs, h->boot.acc, 4 * (size_t)h->K * FQLPOP_EM_LOG_STRIDE, hipMemcpyDeviceToHost, h->s));
        HIPCHK(hipStreamSynchronize(h->s));
    });
}

}  // extern "C"

// =================================================== initial-observation VAE ==
// The reference's InitialObservationEnvModel and vae_loss (envmodel/initial_observation.py:
// 8-78): encoder x -> relu Dense per hidden dim -> (mu, logvar), z = mu + eps exp(logvar / 2),
// decoder z -> relu Dense per reversed hidden dim -> Dense(obs_dim);
// loss = (w mean((x - xhat)^2) + kl) / (w + 1), kl = -0.5 mean(1 + logvar - mu^2 - exp(logvar)).
// A train step is em_vae_grad_kernel (block = 16 minibatch rows, as em_grad_kernel: forward,
// loss, backward, per-block partial grads, per-block log sums) and em_adam_kernel once per
// parameter segment (its W^T refresh walks one chain of Dense layers, and the two encoder
// heads both hang off the last hidden layer): decoder | encoder trunk + mu head | logvar
// head, contiguous in the flat order (flax path-sorted: decoder/Dense_i/{bias, kernel} ...,
// then encoder/Dense_i/{bias, kernel} with Dense_n = mu, Dense_{n+1} = logvar).
//
// Random numbers (Philox4x32-10, key = (seed lo, seed hi)):
//   minibatch row of batch position p at update count s  counter (p, s, 0xE7, 0):
//                                                        row = (x1 << 32 | x0) mod n_rows
//   eps of batch position p, latent index j, count s     counter (p, j, s, 0x1E5)
//   z of fqlpop_initobs_sample row r, latent index j     counter (r, j, 0, 0x5A3), key = the
//                                                        call's seed
//   normal from a counter's (x0, x1): u1 = ((x0 >> 8) + 1) / 2^24 in (0, 1],
//   u2 = (x1 >> 8) / 2^24, n = sqrt(-2 ln u1) cos(2 pi u2)   (Box-Muller)
namespace fq {
namespace em {

constexpr int VLOG = 2;    // per-block log sums: squared error, kl terms
constexpr int VAE_STATIC_LDS = VLOG * R * 4 + R * 8;  // lsum + rowid of em_vae_grad_kernel

// (VMAXH, VaeDense and the two kernels' LDS layouts: emlayout.h)
struct VaeArgs {
    int train;
    int nh, D, L, B, maxd;
    VaeDense enc[VMAXH], mu, lv, dec[VMAXH + 1];
    const float* params;
    const float* wt;                     // W^T copies (same offsets)
    float* part[3];                      // per segment [blocks][segP]
    long long segoff[3], segP[3];
    float* logs;                         // [blocks][VLOG]
    const float* obs;                    // injected [B][D] or the dataset [n_rows][D]
    long long n_rows;
    int injected;
    const float* eps;                    // injected [B][L] or null (device draw)
    uint64_t seed;
    long long step;
    float w;                             // reconstruction_weight
};
struct VaeDecArgs {
    int nh, D, L;
    VaeDense dec[VMAXH + 1];
    const float* params;
    const float* z;                      // [n][L] or null (device draw)
    float* out;                          // [n][D]
    long long n;
    uint64_t seed;
};

DEV float nrand(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t salt) {
    uint32_t x[4] = {c0, c1, c2, salt};
    philox(x, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u1 = (float)((x[0] >> 8) + 1u) * (1.0f / 16777216.0f);
    const float u2 = (float)(x[1] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

DEV float* vae_part(const VaeArgs& a, int seg, long long off) {
    return a.part[seg] + (long long)blockIdx.x * a.segP[seg] + (off - a.segoff[seg]);
}

__global__ __launch_bounds__(NT) void em_vae_grad_kernel(const VaeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float lsum[VLOG][R];
    __shared__ long long rowid[R];
    const int tid = threadIdx.x, blk = blockIdx.x;
    const int nh = a.nh, D = a.D, L = a.L;
    const VaeLds ly = vae_lds(a.enc, a.dec, nh, D, L, a.maxd);
    float* eact[VMAXH + 1];
    float* dact[VMAXH + 1];
    float* x = lds + ly.x;
    float* mu = lds + ly.mu;
    float* lv = lds + ly.lv;
    float* eps = lds + ly.eps;
    float* z = lds + ly.z;
    eact[0] = x;
    dact[0] = z;
    for (int i = 1; i <= nh; ++i) {
        eact[i] = lds + vae_hidden(ly.e1, a.enc, i);
        dact[i] = lds + vae_hidden(ly.d1, a.dec, i);
    }
    float* xhat = lds + ly.xhat;
    float* gmu = lds + ly.gmu;
    float* glv = lds + ly.glv;
    float* gA = lds + ly.gA;
    float* gB = lds + ly.gB;

    // ---- rows (injected, or Philox-drawn rows of the initial-observation set) and eps
    if (tid < R) {
        const int gr = blk * R + tid;
        long long id = gr;
        if (!a.injected) {
            uint32_t c[4] = {(uint32_t)gr, (uint32_t)a.step, 0xE7u, 0u};
            philox(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
            id = (long long)((((uint64_t)c[1] << 32) | c[0]) % (uint64_t)a.n_rows);
        }
        rowid[tid] = id;
    }
    __syncthreads();
    for (int t = tid; t < R * D; t += NT) {
        const int r = t / D, k = t % D;
        x[k * R + r] = a.obs[rowid[r] * D + k];
    }
    for (int t = tid; t < R * L; t += NT) {
        const int r = t / L, k = t % L;
        const long long pos = (long long)blk * R + r;
        eps[k * R + r] = a.eps ? a.eps[pos * L + k]
                               : nrand(a.seed, (uint32_t)pos, (uint32_t)k, (uint32_t)a.step, 0x1E5u);
    }
    __syncthreads();

    // ---- forward
    const float* P = a.params;
    for (int i = 0; i < nh; ++i)
        dense_fwd(P + a.enc[i].w, P + a.enc[i].b, eact[i], a.enc[i].K, a.enc[i].N, eact[i + 1], true);
    dense_fwd(P + a.mu.w, P + a.mu.b, eact[nh], a.mu.K, L, mu, false);
    dense_fwd(P + a.lv.w, P + a.lv.b, eact[nh], a.lv.K, L, lv, false);
    for (int t = tid; t < L * R; t += NT) z[t] = mu[t] + eps[t] * expf(0.5f * lv[t]);
    __syncthreads();
    for (int i = 0; i <= nh; ++i)
        dense_fwd(P + a.dec[i].w, P + a.dec[i].b, dact[i], a.dec[i].K, a.dec[i].N, i < nh ? dact[i + 1] : xhat, i < nh);

    // ---- loss: output gradient (gA [D][R]) and the log sums, one row per thread in a fixed order
    const float wn = 1.0f / (a.w + 1.0f);
    const float grec = a.w * wn * 2.0f / ((float)a.B * (float)D);
    const float gkl = wn / ((float)a.B * (float)L);
    for (int t = tid; t < D * R; t += NT) gA[t] = grec * (xhat[t] - x[t]);
    if (tid < R) {
        float s = 0.f, q = 0.f;
        for (int k = 0; k < D; ++k) {
            const float d = xhat[k * R + tid] - x[k * R + tid];
            s += d * d;
        }
        for (int k = 0; k < L; ++k) {
            const float m = mu[k * R + tid], l = lv[k * R + tid];
            q += 1.0f + l - m * m - expf(l);
        }
        lsum[0][tid] = s;
        lsum[1][tid] = q;
    }
    __syncthreads();
    if (tid < VLOG) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += lsum[tid][r];
        a.logs[(long long)blk * VLOG + tid] = s;
    }
    if (!a.train) return;

    // ---- backward: decoder, down to dz
    float* g = gA;
    float* gn = gB;
    for (int i = nh; i >= 0; --i) {
        const VaeDense& d = a.dec[i];
        dense_dw(dact[i], g, d.K, d.N, vae_part(a, d.seg, d.w), vae_part(a, d.seg, d.b));
        dense_dx(a.wt + d.w, g, d.K, d.N, gn, i > 0 ? dact[i] : nullptr);
        float* tmp = g;
        g = gn;
        gn = tmp;
    }
    // both heads: dmu = dz + kl', dlogvar = dz eps 0.5 exp(logvar / 2) + kl'
    g = lds_ptr(g);
    for (int t = tid; t < L * R; t += NT) {
        const float l = lv[t];
        gmu[t] = g[t] + gkl * mu[t];
        glv[t] = g[t] * eps[t] * 0.5f * expf(0.5f * l) - 0.5f * gkl * (1.0f - expf(l));
    }
    __syncthreads();
    dense_dw(eact[nh], gmu, a.mu.K, L, vae_part(a, a.mu.seg, a.mu.w), vae_part(a, a.mu.seg, a.mu.b));
    dense_dw(eact[nh], glv, a.lv.K, L, vae_part(a, a.lv.seg, a.lv.w), vae_part(a, a.lv.seg, a.lv.b));
    dense_dx(a.wt + a.mu.w, gmu, a.mu.K, L, gA, eact[nh]);
    dense_dx(a.wt + a.lv.w, glv, a.lv.K, L, gB, eact[nh]);
    for (int t = tid; t < a.mu.K * R; t += NT) gA[t] += gB[t];
    __syncthreads();
    // encoder trunk
    g = gA;
    gn = gB;
    for (int i = nh - 1; i >= 0; --i) {
        const VaeDense& d = a.enc[i];
        dense_dw(eact[i], g, d.K, d.N, vae_part(a, d.seg, d.w), vae_part(a, d.seg, d.b));
        if (i > 0) dense_dx(a.wt + d.w, g, d.K, d.N, gn, eact[i]);
        float* tmp = g;
        g = gn;
        gn = tmp;
    }
}

// out[r] = decoder(z[r]) for n rows, 16 per block (rows >= n: zero latents, nothing stored)
__global__ __launch_bounds__(NT) void em_vae_decode_kernel(const VaeDecArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, nh = a.nh, D = a.D, L = a.L;
    const long long row0 = (long long)blockIdx.x * R;
    const VaeDecLds ly = vae_dec_lds(a.dec, nh, L);
    float* dact[VMAXH + 2];
    dact[0] = lds + ly.z;
    for (int i = 1; i <= nh + 1; ++i) dact[i] = lds + vae_hidden(ly.d1, a.dec, i);
    for (int t = tid; t < R * L; t += NT) {
        const int r = t / L, k = t % L;
        const long long row = row0 + r;
        float v = 0.f;
        if (row < a.n) v = a.z ? a.z[row * L + k] : nrand(a.seed, (uint32_t)row, (uint32_t)k, 0u, 0x5A3u);
        lds[ly.z + k * R + r] = v;
    }
    __syncthreads();
    for (int i = 0; i <= nh; ++i)
        dense_fwd(a.params + a.dec[i].w, a.params + a.dec[i].b, dact[i], a.dec[i].K, a.dec[i].N, dact[i + 1], i < nh);
    const float* o = lds_ptr(dact[nh + 1]);
    for (int t = tid; t < R * D; t += NT) {
        const int r = t / D, k = t % D;
        if (row0 + r < a.n) a.out[(row0 + r) * D + k] = o[k * R + r];
    }
}

}  // namespace em
}  // namespace fq

struct fqlpop_initobs {
    fqlpop_initobs_config cfg{};
    int device = 0;
    VaeArgs proto{};                     // layer table and segments
    Net seg_net[3]{};                    // the segments as em_adam_kernel's Dense chains
    long long P = 0;
    DevBuf<float> params, wt, m, v, part, logs;
    DevBuf<float> i_obs, i_eps;
    struct Data {                        // the dataset (rows == 0, null pointer: none)
        DevBuf<float> obs;
        long long rows = 0;
    } data;
    struct Staging {                     // fqlpop_initobs_sample buffers (grown on demand)
        DevBuf<float> z, out;
        long long cap = 0;
    } stage;
    long long count = 0;
    int blocks = 0, lds_bytes = 0, dec_lds = 0;
    Stream<> s;
};

namespace {
// the layer table in flat (flax path-sorted) order; throws E_ARG on a bad shape
void vae_layout(const fqlpop_initobs_config* c, VaeArgs* a, long long* P) {
    ARGCHK(c->obs_dim >= 1 && c->obs_dim <= 4096, "obs_dim must be in 1..4096");
    ARGCHK(c->latent_dim >= 1 && c->latent_dim <= 64, "latent_dim must be in 1..64");
    ARGCHK(c->num_hidden >= 1 && c->num_hidden <= VMAXH, "num_hidden must be in 1..6");
    for (int i = 0; i < c->num_hidden; ++i)
        ARGCHK(c->hidden_dims[i] >= 1 && c->hidden_dims[i] <= 512, "hidden widths must be in 1..512");
    const int nh = c->num_hidden, D = c->obs_dim, L = c->latent_dim;
    *a = VaeArgs{};
    a->nh = nh; a->D = D; a->L = L;
    long long o = 0;
    auto put = [&](VaeDense& d, int K, int N, int seg) {
        d.K = K; d.N = N; d.seg = seg;
        d.b = o; o += N;
        d.w = o; o += (long long)K * N;
    };
    a->segoff[0] = 0;
    int k = L;
    for (int i = 0; i < nh; ++i) {  // decoder: hidden_dims reversed
        put(a->dec[i], k, c->hidden_dims[nh - 1 - i], 0);
        k = c->hidden_dims[nh - 1 - i];
    }
    put(a->dec[nh], k, D, 0);
    a->segP[0] = o;
    a->segoff[1] = o;
    k = D;
    for (int i = 0; i < nh; ++i) {
        put(a->enc[i], k, c->hidden_dims[i], 1);
        k = c->hidden_dims[i];
    }
    put(a->mu, k, L, 1);
    a->segP[1] = o - a->segoff[1];
    a->segoff[2] = o;
    put(a->lv, k, L, 2);
    a->segP[2] = o - a->segoff[2];
    int maxd = std::max(D, L);
    for (int i = 0; i < nh; ++i) maxd = std::max(maxd, c->hidden_dims[i]);
    a->maxd = maxd;
    *P = o;
}

Net vae_chain(const VaeDense* const* ds, int n, long long base) {
    Net net{};
    net.n = n;
    net.ln_scale = net.ln_bias = -1;
    for (int i = 0; i < n; ++i) {
        net.dims[i] = ds[i]->K;
        net.dims[i + 1] = ds[i]->N;
        net.w[i] = ds[i]->w - base;
        net.b[i] = ds[i]->b - base;
    }
    return net;
}

VaeArgs vae_args(fqlpop_initobs* h, bool train, bool injected, const float* eps) {
    VaeArgs a = h->proto;
    a.train = train ? 1 : 0;
    a.B = h->cfg.batch_size;
    a.params = h->params;
    a.wt = h->wt;
    for (int s = 0; s < 3; ++s) a.part[s] = h->part + (long long)h->blocks * a.segoff[s];
    a.logs = h->logs;
    a.injected = injected ? 1 : 0;
    a.obs = injected ? h->i_obs.get() : h->data.obs.get();
    a.n_rows = injected ? h->cfg.batch_size : h->data.rows;
    a.eps = eps;
    a.seed = h->cfg.seed;
    a.step = h->count;
    a.w = h->cfg.reconstruction_weight;
    return a;
}

void vae_launch(fqlpop_initobs* h, const VaeArgs& a) {
    hipLaunchKernelGGL(em_vae_grad_kernel, dim3(h->blocks), dim3(NT), h->lds_bytes, h->s, a);
    HIPCHK(hipGetLastError());
    if (!a.train) return;
    // optax.cosine_decay_schedule(init, steps)(count), adam bias correction with count + 1
    const auto& c = h->cfg;
    const double cc = (double)std::min<long long>(h->count, c.steps);
    const float lr = (float)(c.init_lr * 0.5 * (1.0 + std::cos(3.14159265358979323846 * cc / c.steps)));
    const float bc1 = (float)(1.0 - std::pow(0.9, (double)(h->count + 1)));
    const float bc2 = (float)(1.0 - std::pow(0.999, (double)(h->count + 1)));
    for (int s = 0; s < 3; ++s) {
        const long long off = a.segoff[s];
        AdamArgsEm ad{};
        ad.params = h->params + off; ad.wt = h->wt + off; ad.net = h->seg_net[s];
        ad.m = h->m + off; ad.v = h->v + off; ad.part = a.part[s];
        ad.P = a.segP[s]; ad.blocks = h->blocks;
        ad.lr = lr; ad.bc1 = bc1; ad.bc2 = bc2;
        hipLaunchKernelGGL(em_adam_kernel, dim3((unsigned)((ad.P + 255) / 256)), dim3(256), 0, h->s, ad);
        HIPCHK(hipGetLastError());
    }
    ++h->count;
}

// logs [FQLPOP_INITOBS_LOG_STRIDE] = reconstruction_loss, kl, loss (vae_loss's logs)
void vae_logs(fqlpop_initobs* h, float* out) {
    std::vector<float> lg((size_t)VLOG * h->blocks);
    HIPCHK(hipMemcpyAsync(lg.data(), h->logs, 4 * lg.size(), hipMemcpyDeviceToHost, h->s));
    HIPCHK(hipStreamSynchronize(h->s));
    double s[VLOG] = {0};
    for (int b = 0; b < h->blocks; ++b)
        for (int k = 0; k < VLOG; ++k) s[k] += lg[(size_t)b * VLOG + k];
    const double B = h->cfg.batch_size, w = h->cfg.reconstruction_weight;
    const double rec = s[0] / (B * h->cfg.obs_dim), kl = -0.5 * s[1] / (B * h->cfg.latent_dim);
    for (int k = 0; k < FQLPOP_INITOBS_LOG_STRIDE; ++k) out[k] = 0.f;
    out[0] = (float)rec;
    out[1] = (float)kl;
    out[2] = (float)((w * rec + kl) / (w + 1.0));
}

void vae_upload(fqlpop_initobs* h, const float* obs, const float* eps) {
    const long long B = h->cfg.batch_size;
    HIPCHK(hipMemcpyAsync(h->i_obs, obs, 4 * B * h->cfg.obs_dim, hipMemcpyHostToDevice, h->s));
    if (eps) HIPCHK(hipMemcpyAsync(h->i_eps, eps, 4 * B * h->cfg.latent_dim, hipMemcpyHostToDevice, h->s));
}
}  // namespace

extern "C" {

int fqlpop_initobs_param_count(const fqlpop_initobs_config* cfg, int64_t* n_params) {
    return guard([&] {
        ARGCHK(cfg && n_params, "null argument");
        VaeArgs a;
        long long P;
        vae_layout(cfg, &a, &P);
        *n_params = P;
    });
}

int fqlpop_initobs_create(const fqlpop_initobs_config* cfg, const float* params, int64_t n_params, int device,
                          fqlpop_initobs_t** out) {
    return guard([&] {
        ARGCHK(cfg && params && out, "null argument");
        auto h = std::make_unique<fqlpop_initobs>();
        h->cfg = *cfg;
        h->device = device;
        vae_layout(cfg, &h->proto, &h->P);
        ARGCHK(cfg->batch_size > 0 && cfg->batch_size % R == 0, "batch_size must be a positive multiple of 16");
        ARGCHK(cfg->steps > 0, "steps must be > 0");
        ARGCHK(cfg->reconstruction_weight >= 0.f, "reconstruction_weight must be >= 0");
        ARGCHK(n_params == h->P, "params size mismatch");
        const VaeArgs& a = h->proto;
        const int nh = a.nh, D = a.D, L = a.L;
        // dynamic + static LDS of em_vae_grad_kernel, before any GPU call
        const long long fl = vae_lds(a.enc, a.dec, nh, D, L, a.maxd).total;
        if (fl * 4 + VAE_STATIC_LDS > 160 * 1024)
            throw Err{FQLPOP_E_UNSUPPORTED,
                        "initial-observation VAE: layer widths need " + std::to_string(fl * 4 + VAE_STATIC_LDS) +
                            " bytes of LDS, the fused step has 163840"};
        h->lds_bytes = (int)(fl * 4);
        h->dec_lds = 4 * vae_dec_lds(a.dec, nh, L).total;
        h->blocks = cfg->batch_size / R;
        {
            const VaeDense* ch[VMAXH + 1];
            for (int i = 0; i <= nh; ++i) ch[i] = &a.dec[i];
            h->seg_net[0] = vae_chain(ch, nh + 1, a.segoff[0]);
            for (int i = 0; i < nh; ++i) ch[i] = &a.enc[i];
            ch[nh] = &a.mu;
            h->seg_net[1] = vae_chain(ch, nh + 1, a.segoff[1]);
            ch[0] = &a.lv;
            h->seg_net[2] = vae_chain(ch, 1, a.segoff[2]);
        }
        HIPCHK(hipSetDevice(device));
        const long long P = h->P, B = cfg->batch_size;
        h->s = Stream<>::create();
        h->params = DevBuf<float>(P, "VAE parameters");
        h->wt = DevBuf<float>(P, "VAE parameters");
        h->m = DevBuf<float>(P, "VAE Adam moments");
        h->v = DevBuf<float>(P, "VAE Adam moments");
        h->part = DevBuf<float>(P * h->blocks, "VAE partial grads");
        h->logs = DevBuf<float>((long long)VLOG * h->blocks);
        h->i_obs = DevBuf<float>(B * D);
        h->i_eps = DevBuf<float>(B * L);
        std::vector<float> wt(params, params + P);
        auto tr = [&](const VaeDense& d) {
            for (int k = 0; k < d.K; ++k)
                for (int f = 0; f < d.N; ++f) wt[d.w + (long long)f * d.K + k] = params[d.w + (long long)k * d.N + f];
        };
        for (int i = 0; i <= nh; ++i) tr(a.dec[i]);
        for (int i = 0; i < nh; ++i) tr(a.enc[i]);
        tr(a.mu);
        tr(a.lv);
        HIPCHK(hipMemcpy(h->params, params, 4 * P, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->wt, wt.data(), 4 * P, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(h->m, 0, 4 * P));
        HIPCHK(hipMemset(h->v, 0, 4 * P));
        HIPCHK(hipMemset(h->logs, 0, 4 * (long long)VLOG * h->blocks));
        // the limit is the kernel's, not the handle's: the largest any live handle may need
        static int grad_lds_max = 0, dec_lds_max = 0;
        grad_lds_max = std::max(grad_lds_max, h->lds_bytes);
        dec_lds_max = std::max(dec_lds_max, h->dec_lds);
        HIPCHK(hipFuncSetAttribute((const void*)em_vae_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  grad_lds_max));
        HIPCHK(hipFuncSetAttribute((const void*)em_vae_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  dec_lds_max));
        *out = h.release();
    });
}

int fqlpop_initobs_destroy(fqlpop_initobs_t* h) {
    return guard([&] {
        if (!h) return;
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        delete h;
    });
}

int fqlpop_initobs_set_dataset(fqlpop_initobs_t* h, const float* obs, int64_t n_rows) {
    return guard([&] {
        ARGCHK(h && obs, "null argument");
        ARGCHK(n_rows > 0, "n_rows must be > 0");
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->s));
        replace_released(h->data, [&] {
            fqlpop_initobs::Data d{DevBuf<float>(n_rows * h->cfg.obs_dim, "initial-observation dataset"), n_rows};
            HIPCHK(hipMemcpy(d.obs, obs, 4 * n_rows * h->cfg.obs_dim, hipMemcpyHostToDevice));
            return d;
        });
    });
}

int fqlpop_initobs_step(fqlpop_initobs_t* h, int n_steps) {
    return guard([&] {
        ARGCHK(h && n_steps >= 0, "bad argument");
        if (h->data.rows <= 0) throw Err{FQLPOP_E_STATE, "no dataset: call fqlpop_initobs_set_dataset first"};
        HIPCHK(hipSetDevice(h->device));
        for (int i = 0; i < n_steps; ++i) vae_launch(h, vae_args(h, true, false, nullptr));
    });
}

int fqlpop_initobs_step_injected(fqlpop_initobs_t* h, const float* obs, const float* eps) {
    return guard([&] {
        ARGCHK(h && obs, "null argument");
        HIPCHK(hipSetDevice(h->device));
        vae_upload(h, obs, eps);
        vae_launch(h, vae_args(h, true, true, eps ? h->i_eps : nullptr));
        HIPCHK(hipStreamSynchronize(h->s));  // host batch buffers are reused
    });
}

int fqlpop_initobs_eval(fqlpop_initobs_t* h, const float* obs, const float* eps, float* logs) {
    return guard([&] {
        ARGCHK(h && obs && logs, "null argument");
        ARGCHK(eps, "fqlpop_initobs_eval needs eps (an evaluation is a function of its inputs)");
        HIPCHK(hipSetDevice(h->device));
        vae_upload(h, obs, eps);
        vae_launch(h, vae_args(h, false, true, h->i_eps));
        vae_logs(h, logs);
    });
}

int fqlpop_initobs_read_logs(fqlpop_initobs_t* h, float* logs) {
    return guard([&] {
        ARGCHK(h && logs, "null argument");
        HIPCHK(hipSetDevice(h->device));
        vae_logs(h, logs);
    });
}

int fqlpop_initobs_get_params(fqlpop_initobs_t* h, int which, float* out, int64_t n) {
    return guard([&] {
        ARGCHK(h && out, "null argument");
        ARGCHK(n == h->P, "params size mismatch");
        ARGCHK(which >= 0 && which <= 2, "which must be FQLPOP_STATE_PARAMS/ADAM_M/ADAM_V");
        HIPCHK(hipSetDevice(h->device));
        const float* src = which == 0 ? h->params : which == 1 ? h->m : h->v;
        HIPCHK(hipMemcpyAsync(out, src, 4 * n, hipMemcpyDeviceToHost, h->s));
        HIPCHK(hipStreamSynchronize(h->s));
    });
}

int fqlpop_initobs_get_count(fqlpop_initobs_t* h, int64_t* count) {
    return guard([&] {
        ARGCHK(h && count, "null argument");
        *count = h->count;
    });
}

int fqlpop_initobs_sync(fqlpop_initobs_t* h) {
    return guard([&] {
        ARGCHK(h, "null handle");
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->s));
    });
}

int fqlpop_initobs_sample(fqlpop_initobs_t* h, int64_t n, uint64_t seed, const float* z, float* out) {
    return guard([&] {
        ARGCHK(h && out, "null argument");
        ARGCHK(n >= 1 && n <= (1LL << 31) - R, "n must be in 1..2^31 - 16");
        HIPCHK(hipSetDevice(h->device));
        const long long D = h->cfg.obs_dim, L = h->cfg.latent_dim;
        if (n > h->stage.cap) {
            HIPCHK(hipStreamSynchronize(h->s));
            replace_released(h->stage, [&] {
                return fqlpop_initobs::Staging{DevBuf<float>(n * L, "sample staging"), DevBuf<float>(n * D, "sample staging"), n};
            });
        }
        if (z) HIPCHK(hipMemcpyAsync(h->stage.z, z, 4 * n * L, hipMemcpyHostToDevice, h->s));
        VaeDecArgs a{};
        a.nh = h->proto.nh; a.D = (int)D; a.L = (int)L;
        for (int i = 0; i <= a.nh; ++i) a.dec[i] = h->proto.dec[i];
        a.params = h->params;
        a.z = z ? h->stage.z.get() : nullptr;
        a.out = h->stage.out;
        a.n = n;
        a.seed = seed;
        hipLaunchKernelGGL(em_vae_decode_kernel, dim3((unsigned)((n + R - 1) / R)), dim3(NT), h->dec_lds, h->s, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, h->stage.out, 4 * n * D, hipMemcpyDeviceToHost, h->s));
        HIPCHK(hipStreamSynchronize(h->s));
    });
}

}  // extern "C"
