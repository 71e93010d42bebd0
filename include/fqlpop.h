/*
 * fqlpop.h -- C ABI of the MI355X-native FQL population trainer (libfqlpop.so).
 *
 * The reference's boundary for this path is a Python object API, not an FFI
 * (SURVEY.md section 8b): the callers use FQLAgent.create / update /
 * total_loss / sample_actions / config and flax (to|from)_state_dict of the
 * un-vendored `fql` submodule [EXT].  Each entry point below cites the
 * reference call site it replaces.  The Python shim
 * `flow-q-learning_amd/fql/agents/fql.py` binds these with ctypes (see
 * INTEGRATION.md); nothing here uses torch or C++ types.
 *
 * Conventions
 *   - every function returns 0 on success or a negative FQLPOP_E* code; the
 *     message of the last failure on the calling thread is fqlpop_last_error();
 *   - the handle owns all device memory (params, Adam moments, target critic,
 *     dataset copy, activations, info); host pointers are borrowed for the
 *     duration of the call only;
 *   - calls are stream-ordered on the handle's streams; functions that return
 *     data to the host (read_info, get_state, sample_actions) synchronise;
 *   - one handle per host thread.
 *   - "member" indices are population slots 0..n_members-1.
 */
#ifndef FQLPOP_H
#define FQLPOP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FQLPOP_OK 0
#define FQLPOP_E_ARG (-1)      /* bad argument / shape */
#define FQLPOP_E_HIP (-2)      /* HIP runtime failure */
#define FQLPOP_E_STATE (-3)    /* call not valid in the current state */
#define FQLPOP_E_UNSUPPORTED (-4)

/* Number of float slots per member in the info buffers (13 used for train,
 * 10 for val, in the order of FQLPOP_INFO_*). */
#define FQLPOP_INFO_STRIDE 16
enum {
    FQLPOP_INFO_CRITIC_LOSS = 0, FQLPOP_INFO_Q_MEAN, FQLPOP_INFO_Q_MAX, FQLPOP_INFO_Q_MIN,
    FQLPOP_INFO_ACTOR_LOSS, FQLPOP_INFO_BC_FLOW_LOSS, FQLPOP_INFO_DISTILL_LOSS,
    FQLPOP_INFO_Q_LOSS, FQLPOP_INFO_Q, FQLPOP_INFO_MSE,
    FQLPOP_INFO_GRAD_MAX, FQLPOP_INFO_GRAD_MIN, FQLPOP_INFO_GRAD_NORM
};

/* Which state buffer get_state/set_state address. */
enum { FQLPOP_STATE_PARAMS = 0, FQLPOP_STATE_ADAM_M = 1, FQLPOP_STATE_ADAM_V = 2 };

/* Mirrors trainer/config.py:5-22 (AgentConfig) for the fields update() reads.
 *
 * Accepted ranges (fqlpop_create refuses everything else with FQLPOP_E_ARG) and the path that
 * serves each; every accepted configuration trains, and tests/test_gpu_config_space.py steps
 * the edges named here against the float64 oracle:
 *   hidden_dim   64, 128, 256, 512 or 1024.  512 runs the streamed kernels (whole-network
 *                forwards and backwards, the persistent Euler flow, dW + Adam in one launch),
 *                every other width one GEMM launch per layer and an unfused Adam.
 *   num_hidden   1..15 (at 16 the optimiser's table of 128 trainable leaves is full).  At
 *                hidden_dim 512: 1..8 run the streamed kernels, and small populations split
 *                them into clusters of blocks, the forwards and the Euler flow from 3 hidden
 *                layers, the backwards from 2, nothing at 1; 9..15 run the per-layer path with
 *                one dW GEMM per layer.  fqlpop_rollout and fqlpop_synth_collect serve 1..8
 *                (FQLPOP_E_UNSUPPORTED above); fqlpop_act and fqlpop_sample_actions any depth.
 *   num_qs       1..4, on every path, q_agg mean or min.  State layout: the critic's and the
 *                target critic's leaves are [num_qs][...] for num_qs >= 2 (kernels
 *                [num_qs][in][out], biases and LayerNorm leaves [num_qs][out]); at num_qs = 1
 *                they have NO ensemble axis ([in][out], [out]), where a flax tree keeps a
 *                leading axis of 1.  fqlpop_leaf_info reports the shapes; the flat order and
 *                the number of floats are the same either way.
 *   action_dim   1..8, on every path.
 *   obs_dim      >= 1.  At hidden_dim 512 the streamed forwards and the Euler flow hold up to
 *                64 layer-0 rows: obs_dim + action_dim + 1 <= 64.  Wider inputs run the
 *                per-layer forwards and Euler GEMMs into the streamed backwards and fused
 *                optimiser.  fqlpop_act, fqlpop_rollout and the env-model calls need obs_dim +
 *                action_dim <= 64 (FQLPOP_E_UNSUPPORTED above).
 *   flow_steps   >= 2, on every path.
 *   batch_size   a multiple of 64.
 * Leaves are ordered by name as strings (flax), so from num_hidden = 10 on Dense_10 comes
 * before Dense_2: the flat state is not in layer order. */
typedef struct fqlpop_config {
    int obs_dim;           /* ob_dims[-1]; set by FQLAgent.create from ex_observations */
    int action_dim;        /* set by FQLAgent.create from ex_actions */
    int hidden_dim;        /* width of every hidden layer (actor_hidden_dims == value_hidden_dims) */
    int num_hidden;        /* number of hidden layers (4) */
    int batch_size;        /* AgentConfig.batch_size (256 / 1024) */
    int num_qs;            /* critic ensemble size (2) */
    int layer_norm;        /* critic LayerNorm (scripts pass --agent.layer_norm) */
    int actor_layer_norm;  /* actor LayerNorm (False) */
    int flow_steps;        /* Euler steps (10) */
    int q_agg_min;         /* q_agg == "min" (else "mean") */
    int normalize_q_loss;  /* normalize_q_loss */
    float discount;        /* 0.99   } the value every member starts with; per member:  */
    float tau;             /* 0.005  } fqlpop_set_member_hparams                         */
    float lr;              /* Adam learning rate 3e-4 (likewise)                         */
    int use_graph;         /* capture each step into a hipGraph (1) or launch eagerly (0) */
} fqlpop_config;

typedef struct fqlpop fqlpop_t;

/* Message of the last failed call on this thread ("" if none). */
const char* fqlpop_last_error(void);

/* Engine options: process-wide defaults read by every later fqlpop_create.  They
 * select alternate code paths and stream schedules with the same results
 * (bit-identical, or the per-layer / unfused paths within the parity tolerance),
 * for tests and profiling; there is no reference counterpart.  Names:
 *   euler_fused, stream_fwd, stream_bwd, fused_adam, serial  (0/1)
 *   dw_tile_critic / dw_tile_actor (0..10), adam_nt (0..3),
 *   split (0 off, 1 auto, 2 / 4 / 8: small populations run the streamed forwards, the
 *   Euler flow and the critic / one-step backwards as clusters of 2-8 blocks per 16-column
 *   tile; bit-identical to the unsplit kernels),
 *   small_sched (0/1: up to 256 16-column tiles per step, the target critic and the
 *   critic's TD-column backward run on a fourth stream; bit-identical),
 *   split_sites, split_blocks (per-site split factors and the block cap of a split forward,
 *   for A/B runs),
 *   hw_queues (1..1024, default 4): the GPU_MAX_HW_QUEUES the caller runs the HIP runtime
 *   with.  Below 4 the step is captured on one stream: ROCm 7's graph launch can index past
 *   its pool of branch streams when more than one shares the launch stream's hardware queue.
 *   A caller that sets GPU_MAX_HW_QUEUES passes it here (the Python Population does).
 *   em_seq_sweep (0/1, default 1; read by fqlpop_emtrain_create): multistep env-model
 *   training as a forward and a backward sweep per 16 sequences plus a dW GEMM (0: the
 *   round-5 kernel with dW inside the time loop; same oracle tolerance).
 *   em_ens_xcd (0/1; read by fqlpop_emtrain_create_ensemble): placement of the K models'
 *   blocks of an ensemble training launch.  0: model-major.  1: the block ids that share an
 *   XCD (id mod 8) hold at most ceil(K / 8) models, so an XCD's L2 holds those models'
 *   weights only (fqlpop_emtrain_ensemble_block_map).  Bit-identical results.
 *   lazy_metric (0/1, default 1): a train step leaves the mse info value (the one-step
 *   forward's z_metric columns, a third of that launch, read by no loss or gradient) to be
 *   evaluated when it is read: by fqlpop_read_info(h, 0, .), and before any call that would
 *   overwrite what the evaluation reads (fqlpop_set_state, _set_member with reinit,
 *   _set_active, _clone_members, _step_injected, _total_loss).  Bit-identical to 0, which
 *   evaluates it in every step.  Takes effect with the streamed forward (stream_fwd).
 *   fwd_copies (bit mask 0..3, default 2): in a train step the unsplit streamed forwards
 *   write 1 = the W^T copies of the hidden kernels that the step's streamed backward reads
 *   (BC, one-step and critic forwards), 2 = the target EMA of the critic's hidden kernels
 *   (target forward), and the fused optimiser leaves those copies out.  Bit-identical to 0,
 *   where the optimiser writes both.  Takes effect with stream_fwd, stream_bwd, fused_adam.
 * The defaults are the measured-fastest configuration.  Unknown names or values
 * out of range: FQLPOP_E_ARG.  (Round 3's schedule experiments that measured slower --
 * streams, prio, cdw_sb, dw_stagger, xstep, bc_late, fuse_dq, early_join -- were
 * removed.)  The production library reads no environment variable; result-changing
 * timing switches exist only in diagnostic builds. */
int fqlpop_set_engine_option(const char* name, int value);
int fqlpop_get_engine_option(const char* name, int* value);
int fqlpop_reset_engine_options(void);
/* The split plan a population of n_members created now with `cfg` would run (no GPU call):
 * blocks per 16-column tile of each split launch site, 1 = the unsplit kernel, in site order
 * {BC forward, Euler flow, one-step forward, target critic, critic forward, critic backward
 * (its Q-loss columns under the 4th-stream schedule), one-step backward, critic
 * TD-column backward (4th-stream schedule only)} (blocks_per_tile[8]), and whether the
 * 4th-stream schedule runs.  The step checks each launch against this plan.
 * [no reference counterpart: engine introspection] */
int fqlpop_split_plan(const fqlpop_config* cfg, int n_members, int* blocks_per_tile, int* small_sched);
/* Streams (parallel graph branches) a population created now would capture its step on:
 * 4 (sM, sF, sB, sX), or 1 when engine option serial is set or hw_queues < 4.  The HIP
 * runtime's graph launch indexes past its branch-stream pool when more branches than
 * hardware queues share the launch stream's queue; the capture refuses
 * (FQLPOP_E_STATE) a step with more branches than hw_queues.  No GPU call.  [no reference
 * counterpart: engine introspection] */
int fqlpop_step_streams(int* n_streams);
/* 1 in a diagnostic build (make DIAG=1 / PHASE=1), 0 in the production library. */
int fqlpop_diagnostic_build(void);

/* Replaces FQLAgent.create(seed, ex_obs, ex_act, config)  [EXT]
 * (called at trainer/experiment.py:44-49, utils/agent.py:24-29) for a whole
 * population: allocates the device state for n_members members, member i
 * with alpha alphas[i] and seed seeds[i]; params are initialised on device
 * (Glorot-uniform kernels, zero biases, unit LN scale, target := critic). */
int fqlpop_create(const fqlpop_config* cfg, int n_members, const float* alphas,
                  const uint64_t* seeds, int device, fqlpop_t** out);

/* Frees every device allocation of the handle. */
int fqlpop_destroy(fqlpop_t* h);

/* Replaces the ReplayBuffer/Dataset behind OfflineTaskWithRealEvaluations
 * (task/offline_task_real.py:26-36; sampled at :38-43).  which = 0 train,
 * 1 val.  Row-major host arrays obs[n][obs_dim], act[n][action_dim], rew[n],
 * mask[n], next_obs[n][obs_dim]; copied into an HBM-resident buffer.  If
 * on_device != 0 the pointers are device pointers on the handle's device. */
int fqlpop_set_dataset(fqlpop_t* h, int which, const float* obs, const float* act,
                       const float* rew, const float* mask, const float* next_obs,
                       int64_t n_rows, int on_device);

/* Selects the members that step()/total_loss() advance (SuccessiveHalving
 * pruning, hpo/successive_halving.py:67-101; Experiment.stop at
 * trainer/trainer.py:114-116).  mask[n_members], nonzero = active. */
int fqlpop_set_active(fqlpop_t* h, const uint8_t* mask);

/* Replaces n_steps iterations of the Experiment.train hot loop
 * (trainer/experiment.py:106-109): for every active member, sample a
 * minibatch on device (uniform with replacement, Philox keyed by the member
 * seed and update count) and run agent.update(batch) [EXT FQLAgent.update]. */
int fqlpop_step(fqlpop_t* h, int n_steps);

/* agent.update(batch) (trainer/experiment.py:109) on a host batch: one
 * update of every active member.  batch: per active member (in slot order)
 * the row-major block [obs B*D][act B*A][rew B][mask B][next_obs B*D].
 * noise: NULL => drawn on device (Philox keyed by member seed and update
 * count); else the parity mode: per active member
 * [z_next B*A][x0 B*A][t B][z_d B*A][z_metric B*A].  Host pointers. */
int fqlpop_step_injected(fqlpop_t* h, const float* batch, const float* noise);

/* Replaces agent.total_loss(val_batch, grad_params=None)
 * (trainer/experiment.py:114-115): losses of every active member, no update.
 * batch NULL => sample from the val dataset (which = 1, or the train
 * dataset if no val dataset was set); noise NULL => device RNG; else
 * injected as in fqlpop_step_injected. Results via fqlpop_read_info(h, 1, .). */
int fqlpop_total_loss(fqlpop_t* h, const float* batch, const float* noise);

/* Copies info[n_members][FQLPOP_INFO_STRIDE] of the last train step (which=0)
 * or last total_loss (which=1) to the host; synchronises.  Replaces the
 * update_info / val_info dicts (trainer/experiment.py:109,115).  which=0 first evaluates
 * the last train step's mse if it is still pending (engine option lazy_metric). */
int fqlpop_read_info(fqlpop_t* h, int which, float* out);

/* Replaces agent.sample_actions(observations=obs, seed=..)
 * (evaluator/evaluation.py:58-64,94): clip(onestep(s, z), -1, 1) for n rows of
 * member `member`.  noise[n][action_dim] (host) or NULL => z ~ N(0,1) from
 * Philox(seed).  obs[n][obs_dim], out[n][action_dim] host arrays. */
int fqlpop_sample_actions(fqlpop_t* h, int member, const float* obs, int64_t n,
                          const float* noise, uint64_t seed, float* out);

/* The same policy for every ACTIVE member at once, each on its own n_envs observations:
 * out[z][e] = clip(onestep(obs[z][e], z_noise), -1, 1) for the z-th active member in slot
 * order, the whole network in one launch.  obs[n_active][n_envs][obs_dim],
 * out[n_active][n_envs][action_dim] host arrays.  noise[n_active][n_envs][action_dim]
 * (host) injects z; NULL draws it on the device as fqlpop_rollout draws its policy noise at
 * step t (counted from 1): Philox4x32-10 under seed ^ member key * 0x9E3779B97F4A7C15,
 * counter (env, t, 0x5E11, q), Box-Muller pair q -> actions 2q, 2q + 1.  out_noise, if not
 * NULL, receives the z used (shaped like noise).
 * The staging (pinned host memory and a device buffer) belongs to the handle: sized at the
 * first call, regrown when n_active * n_envs grows, freed by fqlpop_destroy.  One
 * host-to-device copy, one launch and one device-to-host copy on the stream
 * fqlpop_sample_actions uses, then one synchronisation of that stream: the actions come from
 * the parameters every step enqueued before the call leaves, captured graphs stay, and a
 * pending mse evaluation (engine option lazy_metric) stays pending: only parameters are read.
 * Before any GPU call: FQLPOP_E_ARG for a null obs / out, n_envs < 1, or t == 0 with noise
 * NULL; FQLPOP_E_UNSUPPORTED unless obs_dim + action_dim <= 64 and action_dim <= 8 (every
 * hidden_dim and num_hidden fqlpop_create accepts is served).  A poisoned active member is
 * refused as fqlpop_step refuses it.  No active member: success, nothing written.
 * [no reference counterpart: the reference acts one agent at a time, main.py's online loop] */
int fqlpop_act(fqlpop_t* h, const float* obs, int n_envs, const float* noise, uint64_t seed, uint32_t t,
               float* out, float* out_noise);
/* GPU time of the act kernel in the last successful fqlpop_act call on this handle that had
 * an active member, in microseconds (HIP events around the launch; the call's wall time adds
 * the staging and the copies).  FQLPOP_E_STATE before the first.  [no reference counterpart] */
int fqlpop_act_time(fqlpop_t* h, double* kernel_us);

/* Number of floats of one member's flat state (flax tree order: networks
 * actor_bc_flow, actor_onestep_flow, critic, target_critic; leaves sorted as
 * flax does).  which = FQLPOP_STATE_*; M/V have the same layout as PARAMS
 * (target leaves are zero in M/V). */
int fqlpop_state_size(fqlpop_t* h, int64_t* n_floats);

/* flax.serialization.to_state_dict / from_state_dict of one member
 * (trainer/experiment.py:61-63,92,135; utils/agent.py:35): copy the flat
 * state out of / into device memory; synchronises. */
int fqlpop_get_state(fqlpop_t* h, int member, int which, float* flat, int64_t n);
int fqlpop_set_state(fqlpop_t* h, int member, int which, const float* flat, int64_t n);

/* Adam step count of a member (optax count == number of updates). */
int fqlpop_get_count(fqlpop_t* h, int member, int32_t* count);
int fqlpop_set_count(fqlpop_t* h, int member, int32_t count);

/* Per-member alpha and seed (ExperimentConfig.alpha/seed,
 * trainer/config.py:25-28); re-initialises params when reinit != 0.  The member's hparams
 * (below) stay as they are, with or without reinit. */
int fqlpop_set_member(fqlpop_t* h, int member, float alpha, uint64_t seed, int reinit);

/* Per-member learning rate, discount and target-EMA tau: hp[FQLPOP_HP_COUNT], indexed by
 * FQLPOP_HP_*.  fqlpop_create gives every member the fqlpop_config values.  They live in
 * device memory and the step's kernels read their member's row, so a change needs no
 * recapture: set synchronises as fqlpop_set_member does and holds from the next enqueued
 * step on, the replay of a captured graph included; fqlpop_total_loss uses the member's
 * discount too.  set returns FQLPOP_E_ARG before any GPU call, and changes nothing, for a
 * member out of range, an lr that is negative or not finite, or a discount or tau that is
 * NaN or outside [0, 1].  get answers from the host mirror without synchronising.
 * The sampler key of a member is made of its seed and alpha alone: members that share both
 * and differ only in hparams draw the same minibatches and noises (a controlled comparison).
 * The env-model trainers have schedules of their own.  [no reference counterpart: the
 * reference gives every experiment one AgentConfig] */
#define FQLPOP_HP_COUNT 3
enum { FQLPOP_HP_LR = 0, FQLPOP_HP_DISCOUNT = 1, FQLPOP_HP_TAU = 2 };
int fqlpop_set_member_hparams(fqlpop_t* h, int member, const float* hp /*[FQLPOP_HP_COUNT]*/);
int fqlpop_get_member_hparams(fqlpop_t* h, int member, float* hp);

/* Copies the complete training state of member src[i] into member dst[i], i < n_pairs, and
 * gives dst[i] alpha alphas[i] and seed seeds[i]: both parameter buffers and their W^T
 * copies, the target critic, Adam m and v, the update count and src[i]'s hparams (lr,
 * discount, tau; the host mirror follows), in one device launch on the
 * stream the steps run on (and, with fqlpop_synth_create's rings, the ring and its counters
 * in a second one).  Ordered after the steps enqueued before it and before later
 * ones; no host staging and no synchronisation, so it may return before the copy has run
 * (fqlpop_sync waits).  FQLPOP_E_ARG, with nothing enqueued, unless n_pairs >= 1, every
 * index is in range, the dst are pairwise distinct and no dst is also a src; a src may
 * repeat, and neither has to be active.  A src poisoned by a failed split launch is refused
 * (FQLPOP_E_STATE); a successful clone restores a poisoned dst as fqlpop_set_member with
 * reinit does.  [no reference counterpart: PBT exploit] */
int fqlpop_clone_members(fqlpop_t* h, int n_pairs, const int* src, const int* dst,
                         const float* alphas, const uint64_t* seeds);

/* Leaf table of the flat state: name (e.g. "critic/Dense_0/kernel"), offset
 * and shape (up to 3 dims, ndim returned).  i in [0, fqlpop_num_leaves). */
int fqlpop_num_leaves(fqlpop_t* h, int* n);
int fqlpop_leaf_info(fqlpop_t* h, int i, char* name, int name_cap, int64_t* offset,
                     int* ndim, int64_t* shape3);

/* Waits for all work of the handle.  Reports (once) a split launch that gave up; the
 * members it stepped stay poisoned: fqlpop_step / _step_injected refuse while an active
 * member is poisoned, fqlpop_get_state / _get_count refuse for a poisoned member and
 * fqlpop_read_info while any is, until fqlpop_set_state has restored the member's params,
 * Adam m and Adam v (or fqlpop_set_member reinit, or fqlpop_clone_members into it).  [EXT: a JAX error surfaces at the next
 * blocking call of the reference's jitted update] */
int fqlpop_sync(fqlpop_t* h);
/* Test hook: sets the handle's split-error word exactly as a split launch whose hand-off
 * wait gave up does (kernels.hip sp_fail), so the error path above can be exercised without
 * a fault.  FQLPOP_E_STATE if the population runs no split launch.  [no reference
 * counterpart] */
int fqlpop_debug_fail_split(fqlpop_t* h);

/* Measurement hook for bench.py: replays the dominant kernel (the hidden-
 * layer forward GEMM of the Euler flow, all active members in one launch)
 * `iters` times on its own stream between HIP events; returns the mean
 * duration (us) and the algorithmic FLOPs of one launch. */
int fqlpop_time_dominant_kernel(fqlpop_t* h, int iters, double* avg_us, double* flops);

/* In-step timing probe of the dominant kernel (bench.py's roofline): while
 * enabled, every Euler-flow hidden-layer GEMM launch inside fqlpop_step
 * stamps the 100 MHz s_memrealtime clock at the start and end of each of its
 * blocks; a launch lasts max(end) - min(start).  read_probe returns the total
 * (us) and number of launches timed since set_probe (which resets them), and
 * if clock_check != NULL the last fqlpop_time_dominant_kernel cross-check:
 * [0] one isolated launch timed by HIP events, [1] the same by its stamps. */
int fqlpop_set_probe(fqlpop_t* h, int enable);
/* The dominant kernel of fqlpop_step (bench.py's roofline row): its kernel
 * symbol (for profiler filters), algorithmic FLOPs and unique HBM bytes of one
 * launch over the active members. */
int fqlpop_dominant_kernel_info(fqlpop_t* h, char* name, int name_cap, double* flops, double* bytes);
int fqlpop_read_probe(fqlpop_t* h, double* total_us, int64_t* launches, double* clock_check);
/* Probe coverage since set_probe: blocks whose start and end stamps were both written, and
 * blocks launched, summed over the timed launches (equal when every block of every timed
 * launch stamped; the stamps are cleared after each read).  [no reference counterpart] */
int fqlpop_probe_coverage(fqlpop_t* h, int64_t* blocks_seen, int64_t* blocks_expected);

/* ---------------------------------------------------------------------
 * World-model rollout evaluation (BASELINE config 5).
 * Replaces the per-step Python loop of evaluator/evaluation.py:75-114 driving
 * task/offline_task_simulated.py:85-107 (state predictor + termination
 * predictor loaded by utils/envmodel.py:10-56) with ONE device launch for all
 * active members.  Env-model shapes (envmodel/baseline.py:17-37,
 * envmodel/multistep.py:35-54 uses the same cell, envmodel/termination_predictor.py:9-21). */
typedef struct fqlpop_envmodel_config {
    int obs_dim, action_dim;
    int sp_num_hidden;      /* BaselineStatePredictor hidden_dims (multistep default 128,256,128) */
    int sp_hidden[7];
    int tp_num_hidden;      /* TerminationPredictor hidden_dims (default 128,128) */
    int tp_hidden[7];
} fqlpop_envmodel_config;

/* Float counts of the flat parameter vectors in flax leaf order:
 * state predictor  Dense_0/bias, Dense_0/kernel, ..., Dense_n/kernel, LayerNorm_0/bias, LayerNorm_0/scale;
 * termination      Dense_0/bias, Dense_0/kernel, ..., Dense_m/kernel  (kernels [in][out]). */
int fqlpop_envmodel_param_count(const fqlpop_envmodel_config* cfg, int64_t* n_sp, int64_t* n_tp);

/* Upload the env model (utils/envmodel.py:load_model for "baseline"/"multistep"
 * and "termination_predictor"); host arrays, copied. */
int fqlpop_set_env_model(fqlpop_t* h, const fqlpop_envmodel_config* cfg, const float* sp_params, int64_t n_sp,
                         const float* tp_params, int64_t n_tp);

/* Roll every ACTIVE member's one-step policy in the env model from init_obs
 * [n_envs][obs_dim] until each env terminated (termination logit > 0: success 1)
 * or max_steps (truncated: success 0).  noise: NULL (z ~ N(0,1) from Philox keyed
 * by seed and the member seed) or host [n_active][max_steps][n_envs][action_dim].
 * out: host [n_active][n_envs][2] = (success, episode length); out_obs: NULL or
 * host [n_active][n_envs][obs_dim], the observation after the last step run.
 * Active members in slot order.  Needs hidden_dim 512; synchronises. */
int fqlpop_rollout(fqlpop_t* h, const float* init_obs, int n_envs, int max_steps, uint64_t seed,
                   const float* noise, float* out, float* out_obs);

/* One env-model step for given actions (task/offline_task_simulated.py:85-90:
 * state_predictor(obs, actions) then termination_predictor(next_obs)): obs
 * [n][obs_dim], actions [n][action_dim] -> next_obs [n][obs_dim], logits [n]
 * (terminated = logit > 0).  Host arrays; synchronises. */
int fqlpop_envmodel_step(fqlpop_t* h, const float* obs, const float* actions, int n, float* next_obs, float* logits);

/* fqlpop_rollout that also returns the transitions (the reference's evaluate_agent
 * `transitions`): out_traj_obs host [n_active][max_steps][n_envs][obs_dim] and
 * out_traj_act host [n_active][max_steps][n_envs][action_dim], both required.  Entry
 * [t] of an env is the observation before step t + 1 and the clipped action taken
 * there, for every step the env ran (t < episode length); later entries are 0.
 * out / out_obs are exactly fqlpop_rollout's for the same arguments. */
int fqlpop_rollout_record(fqlpop_t* h, const float* init_obs, int n_envs, int max_steps, uint64_t seed,
                          const float* noise, float* out, float* out_obs, float* out_traj_obs,
                          float* out_traj_act);

/* Open-loop replay of recorded actions through the env model, all n episodes in one
 * launch (the reference's "real2sim", evaluator/env_model_evaluator.py:42-56).  Per
 * episode e: x = init_obs[e]; for t = 0 .. lengths[e]-1: if anchor_every > 0, t > 0 and
 * t % anchor_every == 0 then x = anchor_obs[e][t]; x' = state_predictor(x,
 * actions[e][t]); logit = termination_predictor(x'); x = x'.  The replay does not
 * stop at a predicted termination.  anchor_every 0: fully open loop; 1: the
 * teacher-forced one-step error; k: the error at horizon k.
 *   init_obs    [n][obs_dim]       state before step 0
 *   actions     [n][T][action_dim] recorded actions, used as given (no clip)
 *   next_obs    NULL or [n][T][obs_dim]  recorded observation after step t
 *   anchor_obs  NULL or [n][T][obs_dim]  recorded observation before step t
 *   lengths     NULL (= T for all) or [n], each in 1..T
 *   out_logits  [n][T]             termination logit of the predicted x'
 *   out_err     NULL or [n][T][2]  mean_k (x' - next)^2, mean_k |x' - next|; needs next_obs
 *   out_obs     NULL or [n][T][obs_dim]  predicted x'
 * Output entries at t >= lengths[e] are 0.  Host arrays; synchronises.  Runs no actor
 * and reads no member parameters: any hidden_dim; obs_dim + action_dim <= 64,
 * action_dim <= 8 as fqlpop_envmodel_step. */
int fqlpop_envmodel_replay(fqlpop_t* h, const float* init_obs, const float* actions, const float* next_obs,
                           const float* anchor_obs, const int32_t* lengths, int n, int T, int anchor_every,
                           float* out_logits, float* out_err, float* out_obs);

/* GPU time of the replay kernel in the last successful fqlpop_envmodel_replay call on this
 * handle, in microseconds (HIP events around the launch; the call's wall time adds the
 * allocations and copies).  FQLPOP_E_STATE before the first call.  [no reference counterpart] */
int fqlpop_envmodel_replay_time(fqlpop_t* h, double* kernel_us);

/* ---------------------------------------------------------------------
 * World-model ensembles: the rollout above under n_models env models of ONE config
 * (models trained from different seeds), all resident, in one launch.  The ensemble is
 * stored apart from fqlpop_set_env_model's model: setting either never changes what the
 * other's calls return. */
enum { FQLPOP_ENS_PER_MODEL = 0, FQLPOP_ENS_MIXED = 1 };
#define FQLPOP_ENS_MAX_MODELS 16

/* Upload n_models (1..16) state predictor / termination predictor pairs: host
 * sp_params [n_models][n_sp] and tp_params [n_models][n_tp], each row a flat vector as for
 * fqlpop_set_env_model (counts from fqlpop_envmodel_param_count); copied.  Replaces an
 * earlier ensemble.  FQLPOP_E_ARG, with the earlier ensemble kept, for n_models out of
 * range or a count mismatch.  Synchronises.  [no reference counterpart] */
int fqlpop_set_env_model_ensemble(fqlpop_t* h, const fqlpop_envmodel_config* cfg, int n_models,
                                  const float* sp_params, int64_t n_sp, const float* tp_params, int64_t n_tp);

/* fqlpop_rollout of every ACTIVE member under the ensemble; init_obs, noise
 * ([n_active][max_steps][n_envs][action_dim], shared by all models, or NULL: fqlpop_rollout's
 * Philox draw for that seed and member) and the shape limits as there.
 *   FQLPOP_ENS_PER_MODEL: every (member, model) pair runs n_envs episodes under that model.
 *     out host [n_active][n_models][n_envs][2], out_obs NULL or [n_active][n_models][n_envs]
 *     [obs_dim]; slice k is bit for bit fqlpop_rollout's result after
 *     fqlpop_set_env_model(model k).  choice must be NULL.
 *   FQLPOP_ENS_MIXED (trajectory sampling): at step t (from 1) env e steps under model
 *     choice[t - 1][e] (host int32 [max_steps][n_envs], each in [0, n_models)) for both
 *     predictors, or, with choice NULL, under k = (w0 * n_models) >> 32 with w0 the first
 *     word of Philox4x32-10 at counter (e, t, 0x5E12, 0) under the key (low, high 32 bits
 *     of seed): the call seed alone, so every member meets the same model sequence.  The
 *     choice is per env: an episode does not depend on n_envs.  out host
 *     [n_active][n_envs][2], out_obs NULL or [n_active][n_envs][obs_dim]: the observation
 *     after the env's own last step.
 * FQLPOP_E_STATE "no env model ensemble set"; FQLPOP_E_ARG for a bad mode, choice in
 * PER_MODEL mode or a choice entry out of range; FQLPOP_E_UNSUPPORTED as fqlpop_rollout;
 * all before any launch.  Synchronises.  [no reference counterpart] */
int fqlpop_rollout_ensemble(fqlpop_t* h, const float* init_obs, int n_envs, int max_steps, uint64_t seed,
                            const float* noise, int mode, const int32_t* choice, float* out, float* out_obs);

/* fqlpop_rollout_ensemble in FQLPOP_ENS_MIXED with the transitions and the ensemble's
 * disagreement recorded.  out_traj_obs [n_active][max_steps][n_envs][obs_dim] and
 * out_traj_act [..][action_dim] (both required) are fqlpop_rollout_record's: entry [t] of an
 * env is the observation before its step t + 1 and the clipped action taken there.  Optional
 * (NULL or host [n_active][max_steps][n_envs]):
 *   out_traj_model  int32: the model the env stepped under at that step;
 *   out_traj_unc    u = sqrt(max(0, Q / K - |m|^2 / K^2)) with s'_k model k's next observation
 *                   from that (s, a), r_k = s'_k - s'_0, Q = sum_k |r_k|^2, m = sum_k r_k and
 *                   K = n_models: the norm of the ensemble's per-coordinate standard deviation
 *                   of s'.  Exactly 0 when the models' predictions are bitwise equal.  With
 *                   it, every step runs all n_models models, not only the chosen ones.
 * All four are zero where an env did not run the step.  out / out_obs are bit for bit
 * fqlpop_rollout_ensemble's for the same arguments, with or without out_traj_unc.  Errors
 * as there, plus FQLPOP_E_ARG for FQLPOP_ENS_PER_MODEL or a NULL out_traj_obs /
 * out_traj_act.  Synchronises.  [no reference counterpart] */
int fqlpop_rollout_ensemble_record(fqlpop_t* h, const float* init_obs, int n_envs, int max_steps, uint64_t seed,
                                   const float* noise, int mode, const int32_t* choice, float* out, float* out_obs,
                                   float* out_traj_obs, float* out_traj_act, int32_t* out_traj_model,
                                   float* out_traj_unc);

/* GPU time of the kernel of the last successful fqlpop_rollout_ensemble call on this
 * handle, in microseconds (HIP events around the launch, as fqlpop_envmodel_replay_time).
 * FQLPOP_E_STATE before the first call.  [no reference counterpart] */
int fqlpop_rollout_ensemble_time(fqlpop_t* h, double* kernel_us);

/* ---------------------------------------------------------------------
 * Training on world-model branches: a ring of synthetic transitions per member, filled on
 * the device by short on-policy branches in the env model, and a training draw that mixes
 * ring rows with offline rows (MBPO-style branched rollouts).  The reference's
 * Experiment.train is offline only (trainer/experiment.py:106-109): every call of this
 * section has [no reference counterpart].  A population without rings behaves exactly as
 * before. */

/* Allocates, for every one of the n_members slots, a ring of capacity_rows rows of the
 * dataset's five row-major fields (obs[D], act[A], rew, mask, next_obs[D]) and its
 * device-resident counters: rows (valid rows, <= capacity), head (next write position),
 * appended (total so far), all 0; real_ratio is 1.  FQLPOP_E_ARG for capacity_rows < 1 (or
 * >= 2^32); a failed allocation is FQLPOP_E_HIP with the size in the message and leaves no
 * rings; a second call is FQLPOP_E_STATE.  Synchronises; drops the captured step graphs.
 * Every other call of this section is FQLPOP_E_STATE before it. */
int fqlpop_synth_create(fqlpop_t* h, int64_t capacity_rows);

/* real_ratio rho in [0, 1] (else FQLPOP_E_ARG): a device-resident value the training draw
 * reads, written in stream order, so it holds from the next enqueued step on, captured
 * graphs included.  Row b of a member's training minibatch at update count c, with
 * w0..w3 the Philox4x32-10 block at counter (b, c, train salt, 0) under the member key
 * (w0 the row draw and w1 the flow time, as without rings) and u = (w2 >> 8) * 2^-24:
 *   u < rho (float32) or rows == 0:  offline row (w0 * n_rows) >> 32, as without rings;
 *   else:                            position (w0 * rows) >> 32 of the member's ring.
 * rho = 1, or empty rings: every value of the step is what it is without rings, bit for
 * bit.  fqlpop_total_loss and the injected steps never read the rings. */
int fqlpop_synth_set_ratio(fqlpop_t* h, float real_ratio);

/* For every ACTIVE member: n_branches branches of at most horizon steps of its one-step
 * policy in fqlpop_set_env_model's model, appended to its ring.
 *   starts  branch e starts at the training dataset's obs[idx[e]], the same for all members:
 *           idx[e] = start_rows[e] (host int64 [n_branches], each in [0, n_rows)), or, with
 *           start_rows NULL, (w0 * n_rows) >> 32 with w0 the first word of Philox4x32-10 at
 *           counter (e, 0, 0x5E13, 0) under the key (low, high 32 bits of seed).
 *   branch  exactly fqlpop_rollout_record(init_obs = those rows, n_envs = n_branches,
 *           max_steps = horizon, seed, noise = NULL): the same launch on device buffers.
 *   rows    step t < len_e of branch e gives (s_t, a_t, r, m, s_{t+1}): s_{t+1} the next
 *           recorded observation, for the branch's last step the rollout's out_obs; r = 0,
 *           m = 0 if the step terminated (logit > 0), else r = -1, m = 1
 *           (task/offline_task_simulated.py:85-107; reaching horizon is a truncation).
 *   order   the call's valid transitions in (t, then e) order go to ring positions
 *           (head + i) mod capacity; then head advances by their count, rows = min(capacity,
 *           rows + count).  A position is a prefix count over that order, never the order
 *           in which blocks run: identical runs give byte-identical rings.
 * Stream-ordered with the steps and clones enqueued before and after it; copies nothing to
 * the host and may return before it has run.  Before any launch: FQLPOP_E_STATE without
 * rings, env model or training dataset; FQLPOP_E_UNSUPPORTED as fqlpop_rollout;
 * FQLPOP_E_ARG for n_branches < 1, horizon < 1 (or > 65535), n_branches * horizon > capacity
 * (or >= 2^31) or a start row out of range.  No active member: succeeds and does nothing. */
int fqlpop_synth_collect(fqlpop_t* h, int n_branches, int horizon, uint64_t seed, const int64_t* start_rows);

/* fqlpop_synth_collect with the branches run under fqlpop_set_env_model_ensemble's models
 * (trajectory sampling) instead of fqlpop_set_env_model's, which it does not need:
 *   branch  exactly fqlpop_rollout_ensemble_record(init_obs = those rows, n_envs = n_branches,
 *           max_steps = horizon, seed, noise = NULL, FQLPOP_ENS_MIXED, choice = NULL): the same
 *           launch on device buffers, so every member meets the same model sequence.  A
 *           branch's last s_{t+1} is the env's own (a finished env is never merged with its
 *           tile-mates there).
 *   penalty 0: only the chosen models run and the rows are as above.  > 0: every step runs
 *           all models and a row's reward is r - penalty * u with u that step's out_traj_unc
 *           (a MOPO-style uncertainty penalty); m and every other field are unchanged.
 * Starts, rows, order, stream order and the errors are fqlpop_synth_collect's, with
 * FQLPOP_E_STATE "no env model ensemble set" for its "no env model set", plus FQLPOP_E_ARG
 * for a negative or non-finite penalty; all before any launch. */
int fqlpop_synth_collect_ensemble(fqlpop_t* h, int n_branches, int horizon, uint64_t seed, const int64_t* start_rows,
                                  float penalty);

/* The counters of one member's ring (any may be NULL); synchronises. */
int fqlpop_synth_info(fqlpop_t* h, int member, int64_t* rows, int64_t* head, int64_t* appended);

/* Ring positions 0 .. n - 1 of one member (n <= rows, else FQLPOP_E_ARG) to host arrays
 * obs [n][obs_dim], act [n][action_dim], rew [n], mask [n], next_obs [n][obs_dim];
 * synchronises.  For tests and checkpoints. */
int fqlpop_synth_read(fqlpop_t* h, int member, float* obs, float* act, float* rew, float* mask, float* next_obs,
                      int64_t n);

/* Empties one member's ring (counters to 0), or every ring with member = -1; stream-ordered.
 * fqlpop_set_member with reinit != 0 does the same for its member, and
 * fqlpop_clone_members gives dst[i] a copy of src[i]'s ring and counters. */
int fqlpop_synth_clear(fqlpop_t* h, int member);

/* The inverse of fqlpop_synth_read plus fqlpop_synth_info, for checkpoints: ring positions
 * 0 .. n - 1 of one member become the host rows obs [n][obs_dim], act [n][action_dim], rew [n],
 * mask [n], next_obs [n][obs_dim], and its counters rows = n, head = appended mod capacity,
 * appended = appended.  Every ring the engine builds has rows = min(capacity, appended) and
 * head = appended mod capacity, so n must equal min(capacity, appended); n = 0, appended = 0 is
 * fqlpop_synth_clear(member).  The member need not be active.  Stream-ordered on the stream the
 * steps, collects and clones run on: work enqueued earlier sees the old ring, later work the new
 * one, the replay of a captured step graph included (no graph is dropped).  The rows are staged
 * in host memory of the handle's: the arrays may be reused when the call returns, which may be
 * before the ring is written (fqlpop_sync waits).  Before any GPU work, with nothing changed:
 * FQLPOP_E_STATE without rings; FQLPOP_E_ARG for a null handle, a member out of range, a null
 * array with n > 0, n < 0 or n > capacity, appended < n or n != min(capacity, appended).
 * [no reference counterpart] */
int fqlpop_synth_write(fqlpop_t* h, int member, const float* obs, const float* act, const float* rew,
                       const float* mask, const float* next_obs, int64_t n, int64_t appended);

/* Appends n host rows (arrays as fqlpop_synth_write's) to one member's ring by
 * fqlpop_synth_collect's "order" rule with the host rows in place of the branch transitions:
 * row i goes to position (head + i) mod capacity; then head advances by n, rows = min(capacity,
 * rows + n) and appended += n.  The placement reads head from the device counters, so an append
 * enqueued behind a collect lands behind that collect's rows without a host round trip.  This
 * is how observed transitions of an environment of the caller's reach a ring (FQL's
 * offline-to-online setting).  0 <= n <= capacity; n = 0 succeeds and does nothing.  Member,
 * stream order, graphs, staging and the errors are fqlpop_synth_write's (without those on
 * appended).  [no reference counterpart] */
int fqlpop_synth_append(fqlpop_t* h, int member, const float* obs, const float* act, const float* rew,
                        const float* mask, const float* next_obs, int64_t n);

/* fqlpop_synth_append for every ACTIVE member in one call: the arrays are
 * [n_active][n][..] (obs and next_obs rows of obs_dim, act rows of action_dim, rew and mask
 * scalars), block z for the z-th active member in slot order.  One staging copy, one
 * placement launch over (field, member) and one commit launch that advances every active
 * slot's counters: rings and counters are byte for byte what n_active calls of
 * fqlpop_synth_append in slot order leave.  0 <= n <= capacity rows per member; n = 0, or no
 * active member, succeeds and does nothing.  Stream order, graphs, staging and the errors
 * (before any GPU work) are fqlpop_synth_append's.  [no reference counterpart] */
int fqlpop_synth_append_active(fqlpop_t* h, const float* obs, const float* act, const float* rew,
                               const float* mask, const float* next_obs, int n);

/* ---------------------------------------------------------------------------
 * Env-model trainer: the reference's world-model
 * trainers, one fused GPU step per train_step.
 *   FQLPOP_EM_STATE_PREDICTOR: StatePredictorTrainer.train_step
 *     (envmodel/state_predictor_trainer.py:67-95) on BaselineStatePredictor
 *     (envmodel/baseline.py:25-37) with state_prediction_loss
 *     (envmodel/loss.py:80-111, reconstruction_weight 0 as train_env_model.py:37-44
 *     binds it; termination_weight > 0 scores the predicted next observation with
 *     a frozen termination predictor, fqlpop_emtrain_set_frozen_termination).
 *   FQLPOP_EM_TERMINATION: TerminationPredictorTrainer.train_step
 *     (envmodel/termination_predictor_trainer.py:55-76) on TerminationPredictor
 *     (envmodel/termination_predictor.py:14-21, input dropout) with focal_loss
 *     (envmodel/loss.py:33-66, train_env_model.py:79).
 *   Optimiser: optax.adam(optax.cosine_decay_schedule(init_lr, steps))
 *     (state_predictor_trainer.py:57-61).
 * Parameters are flat vectors in flax leaf order (path-sorted): Dense_i/bias,
 * Dense_i/kernel ([in][out]) ..., then LayerNorm_0/bias, LayerNorm_0/scale. */
enum { FQLPOP_EM_STATE_PREDICTOR = 0, FQLPOP_EM_TERMINATION = 1, FQLPOP_EM_MULTISTEP = 2 };
/* FQLPOP_EM_MULTISTEP: the same trainer on MultistepStatePredictor
 *   (envmodel/multistep.py:31-54, train_env_model.py:46-66): the baseline cell scanned
 *   over sequence_length steps from observations[:, 0] (each prediction is the next
 *   step's observation), state_prediction_loss over all B x T predictions, gradients by
 *   backpropagation through time.  Batches are [B][T][..]; device sampling draws
 *   MultistepLoader windows (utils/data_loader.py:25-39): a uniform episode of
 *   episode_length rows, a uniform start in [0, episode_length - T). */
#define FQLPOP_EM_LOG_STRIDE 8
/* logs: state predictor  [loss, next_observation_loss, termination_loss,
 *                         true_termination_loss, false_termination_loss]
 *       termination      [loss, true_loss, false_loss, accuracy, precision, recall]
 *       (accuracy / precision / recall: eval only; envmodel/termination_predictor_trainer.py:78-112) */
typedef struct fqlpop_emtrain_config {
    int kind;                      /* FQLPOP_EM_* */
    int obs_dim, action_dim;
    int num_hidden;
    int hidden_dims[8];            /* --model.hidden_dims, default (128, 256, 128) (argparser.py:184-189) */
    int batch_size;                /* multiple of 16 (256) */
    int steps;                     /* cosine decay horizon (TrainerConfig.steps) */
    float init_lr;                 /* 1e-3 */
    float termination_weight;      /* state predictor (argparser default 1.0; baseline scripts 0) */
    float true_termination_weight; /* 30 */
    float focal_alpha, focal_gamma;/* 0.25, 2 */
    float dropout_rate;            /* 0.1 */
    uint64_t seed;                 /* device sampling and the fixed dropout mask */
    int tp_num_hidden;             /* frozen termination predictor (termination_weight > 0) */
    int tp_hidden_dims[8];
    int sequence_length;           /* FQLPOP_EM_MULTISTEP: T (--sequence_length, 256) */
    int episode_length;            /* FQLPOP_EM_MULTISTEP device sampling: rows per episode (1000) */
} fqlpop_emtrain_config;
typedef struct fqlpop_emtrain fqlpop_emtrain_t;

int fqlpop_emtrain_param_count(const fqlpop_emtrain_config* cfg, int64_t* n_params);
/* Replaces TrainState.create(params=model.init(...), tx=adam(schedule)) of the
 * trainers' __init__; params are the initial flat parameters (host, copied). */
int fqlpop_emtrain_create(const fqlpop_emtrain_config* cfg, const float* params, int64_t n_params, int device,
                          fqlpop_emtrain_t** out);
int fqlpop_emtrain_destroy(fqlpop_emtrain_t* h);
/* utils/envmodel.py load_model("termination_predictor") of the state trainer's __init__.
 * A failed call keeps the earlier predictor. */
int fqlpop_emtrain_set_frozen_termination(fqlpop_emtrain_t* h, const float* tp_params, int64_t n);
/* The StepLoader's dataset (utils/data_loader.py:47-52), uploaded once: rows sampled on
 * device (uniform with replacement, Philox keyed by seed and step).  Released before the
 * new one is allocated: a failed upload (FQLPOP_E_HIP) leaves no dataset. */
int fqlpop_emtrain_set_dataset(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                               const float* next_obs, int64_t n_rows);
/* n_steps train_steps on device-sampled batches (asynchronous). */
int fqlpop_emtrain_step(fqlpop_emtrain_t* h, int n_steps);
/* One train_step on a host batch [batch_size][..]; keep_mask: NULL (the handle's fixed
 * Philox dropout mask) or [batch_size][obs_dim] bytes (termination kind). Synchronises. */
int fqlpop_emtrain_step_injected(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                                 const float* next_obs, const uint8_t* keep_mask);
/* eval_step on a host batch (no dropout, no update): logs[FQLPOP_EM_LOG_STRIDE]. */
int fqlpop_emtrain_eval(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                        const float* next_obs, float* logs);
/* Logs of the last train step; synchronises. */
int fqlpop_emtrain_read_logs(fqlpop_emtrain_t* h, float* logs);
/* which = FQLPOP_STATE_PARAMS / _ADAM_M / _ADAM_V; flax.serialization.to_bytes source
 * (train_env_model.py:132-134). Synchronises. */
int fqlpop_emtrain_get_params(fqlpop_emtrain_t* h, int which, float* out, int64_t n);
int fqlpop_emtrain_get_count(fqlpop_emtrain_t* h, int64_t* count);
/* The launch plan chosen at creation (read-only, no GPU call): *sweep = 1 when the multistep
 * step runs em_sweep_kernel + em_seq_dw_kernel, 0 for em_seq_grad_kernel (and for the
 * single-step kinds); *tchunks = T chunks of the dW GEMM (1 off the sweep path); *blocks =
 * 16-row blocks per model.  A null out pointer is skipped. */
int fqlpop_emtrain_get_plan(fqlpop_emtrain_t* h, int* sweep, int* tchunks, int* blocks);
int fqlpop_emtrain_sync(fqlpop_emtrain_t* h);

/* World-model ensemble training: K models behind one handle, every train step one launch
 * chain with a model axis (K x batch_size / 16 blocks) instead of K chains (train_env_model.py
 * --ensemble_size loops train_one).  The models share cfg, the dataset, the frozen termination
 * predictor and the update count (so the cosine learning rate and Adam's bias corrections);
 * each has its own parameters, moments and seed (minibatch draw, dropout mask).  cfg->seed is
 * ignored in favour of seeds[k].  Model k is bitwise the single-model trainer created with
 * seed seeds[k] and params[k], for every K and either em_ens_xcd placement.
 * params: [n_models][P] (P = fqlpop_emtrain_param_count), n_params = n_models * P.
 * n_models outside 1..FQLPOP_EM_ENS_MAX_MODELS, a size mismatch or a null seeds:
 * FQLPOP_E_ARG before any GPU call.  A multistep handle allocates one record store per model
 * (about 300 MB each at B = T = 256 and the default widths); a failed allocation is
 * FQLPOP_E_HIP with the size in the message.
 * fqlpop_emtrain_set_dataset, _set_frozen_termination, _step, _sync, _get_count and _destroy
 * serve both kinds of handle.  On a handle with n_models > 1 the single-model calls
 * _step_injected, _eval, _read_logs and _get_params return FQLPOP_E_ARG and name the call
 * below that replaces them. */
#define FQLPOP_EM_ENS_MAX_MODELS 16
int fqlpop_emtrain_create_ensemble(const fqlpop_emtrain_config* cfg, int n_models, const float* params,
                                   int64_t n_params, const uint64_t* seeds, int device, fqlpop_emtrain_t** out);
int fqlpop_emtrain_num_models(fqlpop_emtrain_t* h, int* n_models);
/* One train_step of every model on host batches.  shared = 1: one [batch_size][..] batch (and
 * keep mask) for all models; shared = 0: [n_models][batch_size][..] arrays.  keep_mask may be
 * NULL (each model's Philox dropout mask).  Synchronises. */
int fqlpop_emtrain_step_injected_ensemble(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                                          const float* next_obs, const uint8_t* keep_mask, int shared);
/* eval_step of every model (no dropout, no update): logs[n_models][FQLPOP_EM_LOG_STRIDE]. */
int fqlpop_emtrain_eval_ensemble(fqlpop_emtrain_t* h, const float* obs, const float* act, const float* rew,
                                 const float* next_obs, int shared, float* logs);
/* Logs of the last train step of every model, logs[n_models][FQLPOP_EM_LOG_STRIDE]; one
 * synchronisation for all of them. */
int fqlpop_emtrain_read_logs_ensemble(fqlpop_emtrain_t* h, float* logs);
/* fqlpop_emtrain_get_params of one model; n = P. */
int fqlpop_emtrain_get_params_model(fqlpop_emtrain_t* h, int model, int which, float* out, int64_t n);
/* The placement of an ensemble launch of n_models x blocks_per_model blocks (no GPU call):
 * the grid size, and the (model, block within the model) that linear block id linear_block
 * runs; model = block = -1 marks a padding block, which exits at once.  xcd_mode as engine
 * option em_ens_xcd.  n_models outside 1..16, blocks_per_model < 1, xcd_mode outside {0, 1},
 * linear_block outside the grid: FQLPOP_E_ARG.  [no reference counterpart: introspection] */
int fqlpop_emtrain_ensemble_block_map(int n_models, int blocks_per_model, int xcd_mode, int linear_block,
                                      int* grid_blocks, int* model, int* block);

/* Bootstrapped training (PETS / MBPO / MOPO): every model of a handle (one of a single-model
 * handle) draws its minibatches through its own resample of the dataset, and is evaluated on
 * the units its resample missed (out of bag).  The unit is what the device draw draws: a row
 * (n_units = n_rows) for the state and termination predictors, an episode (n_units = n_rows /
 * episode_length) for FQLPOP_EM_MULTISTEP, whose window start inside the episode is drawn as
 * without a table.  A device-sampled step computes its unit index u as without a table (same
 * Philox counter, salt and modulus) and then trains on unit table[model][u]; the injected
 * calls ignore the table.  An identity table gives the bits of a handle without one.
 *   table[k][i] (drawn on the device)  Philox4x32-10, key = seeds[k] (cfg.seed of a
 *       single-model handle), counter (lo32(i), hi32(i), FQLPOP_EM_SALT_BOOT, 0):
 *       (x1 << 32 | x0) mod n_units
 *   oob[k]    the units that do not occur in table[k], ascending; n_oob[k] of them
 *   out-of-bag batch j of a call with `draw`, batch position p:  counter (p, j,
 *       FQLPOP_EM_SALT_OOB, lo32(draw)), key = seeds[k]: unit oob[k][(x1 << 32 | x0) mod
 *       n_oob[k]]; multistep: window start x2 mod (episode_length - T), as in training
 * The set-up (fill, mark, compact: three small launches for all K models, deterministic) runs
 * once per call of a setter, not on the step's path.  Every refusal below comes before any
 * launch and changes neither the tables nor the models.  fqlpop_emtrain_set_dataset drops the
 * tables (they index the old rows): bootstrap is off until it is set again. */
#define FQLPOP_EM_SALT_BOOT 0xB7u
#define FQLPOP_EM_SALT_OOB 0xB5u
/* enable = 1 draws the K tables and out-of-bag lists, 0 drops them (the handle trains as if
 * they had never been set).  FQLPOP_E_STATE before fqlpop_emtrain_set_dataset; FQLPOP_E_ARG
 * for another value of enable.  A failed allocation (FQLPOP_E_HIP) keeps the earlier tables. */
int fqlpop_emtrain_set_bootstrap(fqlpop_emtrain_t* h, int enable);
/* A caller's own resample or partition: table[n_models][n_units], n = n_models * n_units.
 * FQLPOP_E_STATE before the dataset; FQLPOP_E_ARG for another n or an entry outside
 * [0, n_units) (the host checks every entry). */
int fqlpop_emtrain_set_bootstrap_table(fqlpop_emtrain_t* h, const int64_t* table, int64_t n);
/* One model's table[n_units] and, when oob is not NULL, its out-of-bag list (oob_cap >=
 * n_oob entries of room, else FQLPOP_E_ARG); *n_oob always.  FQLPOP_E_STATE without tables;
 * FQLPOP_E_ARG for a model out of range or another n_units.  Synchronises. */
int fqlpop_emtrain_get_bootstrap(fqlpop_emtrain_t* h, int model, int64_t* table, int64_t n_units, int64_t* oob,
                                 int64_t oob_cap, int64_t* n_oob);
/* eval_step of every model on n_batches out-of-bag batches drawn on the device (no dropout,
 * no update, the update count unchanged): logs[n_models][FQLPOP_EM_LOG_STRIDE], each the
 * float32 mean over the batches of the logs fqlpop_emtrain_eval_ensemble gives for that
 * batch, summed in batch order on the device; no upload, one synchronisation.
 * FQLPOP_E_ARG for n_batches < 1; FQLPOP_E_STATE without a dataset or tables, or when a
 * model's out-of-bag list is empty (the text names the model). */
int fqlpop_emtrain_eval_oob(fqlpop_emtrain_t* h, int n_batches, uint64_t draw, float* logs);

/* ---------------------------------------------------------------------------
 * Initial-observation VAE (the decoder as a source of episode
 * starts): InitialObservationEnvModel and vae_loss (envmodel/initial_observation.py:8-78).
 *   encoder  x -> relu(Dense(h)) for h in hidden_dims -> mu = Dense(latent), logvar =
 *            Dense(latent), both from the last hidden activation (:8-18)
 *   decoder  z -> relu(Dense(h)) for h in hidden_dims[::-1] -> Dense(obs_dim) (:21-29, :39)
 *   forward  z = mu + eps exp(logvar / 2), eps ~ N(0, 1) fresh on every step (:41-52, :62)
 *   loss     (w mean((x - xhat)^2) + kl) / (w + 1), kl = -0.5 mean(1 + logvar - mu^2 -
 *            exp(logvar)), w = reconstruction_weight (:65-70)
 *   optimiser  the reference ships no trainer for this model; the one of its other
 *            env-model trainers: optax.adam(optax.cosine_decay_schedule(init_lr, steps))
 *            (envmodel/state_predictor_trainer.py:57-61)
 * Parameters are one flat vector in flax leaf order (path-sorted): decoder/Dense_i/bias,
 * decoder/Dense_i/kernel ([in][out]), i = 0..num_hidden, then encoder/Dense_i/..., i =
 * 0..num_hidden + 1 (Dense_{num_hidden} = mu, Dense_{num_hidden + 1} = logvar).
 * A step is one fused launch (forward, loss, backward of 16-row blocks) and the Adam
 * launches, on the handle's one stream.  Random draws: csrc/emtrain.hip, VAE section. */
#define FQLPOP_INITOBS_LOG_STRIDE 4
/* logs: [reconstruction_loss, kl, loss] (initial_observation.py:72-76) */
typedef struct fqlpop_initobs_config {
    int obs_dim;
    int latent_dim;                /* --model.latent_dim, 1..64 */
    int num_hidden;                /* 1..6 */
    int hidden_dims[8];            /* --model.hidden_dims, each 1..512 (initial_observation.py:35: (128,)) */
    int batch_size;                /* multiple of 16 */
    int steps;                     /* cosine decay horizon */
    float init_lr;
    float reconstruction_weight;   /* --reconstruction_weight */
    uint64_t seed;                 /* device row sampling and eps */
} fqlpop_initobs_config;
typedef struct fqlpop_initobs fqlpop_initobs_t;

/* FQLPOP_E_ARG on a shape outside the ranges above. */
int fqlpop_initobs_param_count(const fqlpop_initobs_config* cfg, int64_t* n_params);
/* model.init + TrainState.create as the other trainers' __init__
 * (state_predictor_trainer.py:50-61); params: initial flat parameters (host, copied).
 * FQLPOP_E_UNSUPPORTED, before any GPU call, when the widths do not fit the fused
 * step's 160 KB of LDS. */
int fqlpop_initobs_create(const fqlpop_initobs_config* cfg, const float* params, int64_t n_params, int device,
                          fqlpop_initobs_t** out);
int fqlpop_initobs_destroy(fqlpop_initobs_t* h);
/* InitialObservationLoader's rows (utils/data_loader.py:14-22), [n_rows][obs_dim], copied:
 * minibatches are drawn from them on the device, uniform with replacement.  Released before
 * the new rows are allocated: a failed upload (FQLPOP_E_HIP) leaves no dataset. */
int fqlpop_initobs_set_dataset(fqlpop_initobs_t* h, const float* obs, int64_t n_rows);
/* n_steps updates on device-drawn rows and device-drawn eps (vae_loss + adam;
 * asynchronous).  FQLPOP_E_STATE before fqlpop_initobs_set_dataset. */
int fqlpop_initobs_step(fqlpop_initobs_t* h, int n_steps);
/* One update on a host batch obs [batch_size][obs_dim]; eps [batch_size][latent_dim], or
 * NULL for the device draw of the current update count (initial_observation.py:62: a new
 * key per call).  Synchronises. */
int fqlpop_initobs_step_injected(fqlpop_initobs_t* h, const float* obs, const float* eps);
/* vae_loss's logs of the current parameters on a host batch, no update
 * (initial_observation.py:55-78); eps is required (FQLPOP_E_ARG if NULL). */
int fqlpop_initobs_eval(fqlpop_initobs_t* h, const float* obs, const float* eps, float* logs);
/* Logs of the last step [FQLPOP_INITOBS_LOG_STRIDE]; synchronises. */
int fqlpop_initobs_read_logs(fqlpop_initobs_t* h, float* logs);
/* which = FQLPOP_STATE_PARAMS / _ADAM_M / _ADAM_V; the source of initial_observation.pt
 * (distribution_visualizer.py:62-99 reads params/decoder from it).  Synchronises. */
int fqlpop_initobs_get_params(fqlpop_initobs_t* h, int which, float* out, int64_t n);
int fqlpop_initobs_get_count(fqlpop_initobs_t* h, int64_t* count);
int fqlpop_initobs_sync(fqlpop_initobs_t* h);
/* out [n][obs_dim] = decoder(z) (distribution_visualizer.py:84-99: decoder.apply on
 * N(0, 1) latents); z: host [n][latent_dim], or NULL for normals drawn on the device
 * from (seed, row, latent index).  n >= 1.  Synchronises. */
int fqlpop_initobs_sample(fqlpop_initobs_t* h, int64_t n, uint64_t seed, const float* z, float* out);

/* Algorithmic GEMM FLOPs of one member-update at the handle's config
 * (SURVEY.md 8d formula). */
double fqlpop_flops_per_member_step(const fqlpop_config* cfg);
/* GEMM FLOPs one train step of this population runs per member: the count above, less the
 * one-step forward's z_metric columns when the handle defers them (engine option
 * lazy_metric); those run when the train info is read.  0 for a null handle. */
double fqlpop_train_step_flops(fqlpop_t* h);
/* Deferred mse evaluations (engine option lazy_metric) the handle has launched so far: a
 * fqlpop_read_info with nothing pending launches nothing.  [test hook] */
int fqlpop_metric_evaluations(fqlpop_t* h, int64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* FQLPOP_H */
