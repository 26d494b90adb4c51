/*
 * rlx_hip.h -- C ABI of librlxhip.so: the MI355X (gfx950) PPO/SAC training hot path
 * behind RL-X's plugin API.
 *
 * The reference (nico-bohlinger/RL-X) is 100 % Python; its "kernels" are XLA fusions
 * produced by jax.jit.  There is no FFI in the reference; each entry point below
 * names the reference jit region / function it replaces (paths relative to the
 * reference repository root).  INTEGRATION.md shows the ctypes stub a maintainer
 * would add on the reference side.
 *
 * Conventions
 *   - extern "C"; every function returns int: 0 = ok, negative = RLX_E*;
 *     rlx_last_error() returns a thread-local message valid until the next call.
 *   - tensor arguments are raw DEVICE pointers (contiguous, row-major, fp32 /
 *     int32 / uint32), caller-owned; the library never frees or retains them.
 *   - PRNG keys (uint32[2]) are HOST pointers (two words; split on the host).
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *     Launches are asynchronous; no implicit synchronisation.
 *   - library-owned scratch lives in the opaque rlx_ctx; one ctx per thread/GPU.
 *   - rollout arrays are time-major [T,N,...] exactly like the reference's Batch
 *     (rl_x/algorithms/ppo/flax/batch.py:1-11); flattened sample index i = t*N + n
 *     (rl_x/algorithms/ppo/flax/ppo.py:180-184).
 *
 * Flat parameter layout of one MLP (rlx_mlp_desc), shared with oracle/nets.py:
 *   for each hidden layer l: W_l[in,out] row-major (flax Dense kernel), b_l[out],
 *   then for layer 0 iff ln_first: ln_scale[out], ln_bias[out];
 *   head W[in,out], b[out]; iff has_logstd: logstd[out_dim].
 */
#ifndef RLX_HIP_H
#define RLX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLX_OK 0
#define RLX_EINVAL (-1)  /* bad argument                                  */
#define RLX_EHIP (-2)    /* a HIP runtime call failed (see rlx_last_error) */
#define RLX_ENOMEM (-3)  /* scratch allocation failed                      */
#define RLX_EUNSUP (-4)  /* shape/arch outside the supported envelope      */

#define RLX_ACT_TANH 0
#define RLX_ACT_ELU 1
#define RLX_ACT_RELU 2
#define RLX_ACT_NONE 3 /* identity (internal GEMM stages; not a valid rlx_mlp_desc.act) */
#define RLX_ACT_SILU 4 /* x * sigmoid(x): only behind a LayerNorm (rlx_lnmlp_desc, FastSAC); not a valid rlx_mlp_desc.act */

#define RLX_THREEFRY_LEGACY 0        /* jax_threefry_partitionable=False */
#define RLX_THREEFRY_PARTITIONABLE 1 /* default since JAX 0.5.0          */

typedef struct rlx_ctx rlx_ctx; /* opaque: device id + scratch arenas */

/* One MLP actor or critic.
 * arch A: rl_x/algorithms/ppo/flax/policy.py:31-40, critic.py:22-30
 *         n_hidden=2, hidden={H,H}, act=TANH, ln_first=0
 * arch B: rl_x/algorithms/ppo/flax_full_jit/policy.py:30-42, critic.py:21-32
 *         n_hidden=3, hidden={512,256,128}, act=ELU, ln_first=1                */
typedef struct rlx_mlp_desc {
  int32_t in_dim;
  int32_t n_hidden; /* 1..3 */
  int32_t hidden[4];
  int32_t out_dim;
  int32_t act;        /* RLX_ACT_*                                   */
  int32_t ln_first;   /* 1: LayerNorm(eps 1e-6) after the first Dense */
  int32_t has_logstd; /* policy: trailing logstd[out_dim]             */
} rlx_mlp_desc;

/* PPO hyper-parameters of one update (rl_x/algorithms/ppo/flax/default_config.py:9-26). */
typedef struct rlx_ppo_hparams {
  float clip_range;
  float entropy_coef;
  float critic_coef;
  float max_grad_norm; /* <= 0: no clipping */
  float adam_b1, adam_b2, adam_eps;
  int32_t discrete_actions; /* 0: diagonal-Gaussian policy (out_dim = action dim, has_logstd = 1).  1: Categorical policy
                             * (DiscreteFlatValuesPolicy, rl_x/algorithms/ppo/pytorch/policy.py:96-135 -- the only discrete
                             * PPO head of the reference): out_dim = number of actions (<= 8), has_logstd = 0, the `actions`
                             * arrays hold ONE float per sample = the action index. */
  const float* critic_states; /* NULL: policy and critic read the same observation rows (`states`, width pdesc->in_dim ==
                             * cdesc->in_dim).  Otherwise DEVICE [T, N, cdesc->in_dim]: the critic's OWN observation columns of
                             * the same rollout rows -- an env with critic_observation_indices != policy_observation_indices
                             * (`x[..., self.critic_observation_indices]`, rl_x/algorithms/ppo/flax/critic.py:12,24; policy.py:13,33);
                             * `states` then holds the policy's columns [T, N, pdesc->in_dim].  The column selection itself is
                             * rlx_select_columns_f32, applied once per acting step when the row is stored. */
} rlx_ppo_hparams;

/* ---- library ----------------------------------------------------------------- */
int rlx_version(void);
const char* rlx_last_error(void);
int rlx_ctx_create(int device, rlx_ctx** out);
int rlx_ctx_destroy(rlx_ctx* ctx);
/* number of fp32 parameters of `desc` (== oracle MLPSpec.n_params) */
int64_t rlx_mlp_param_count(const rlx_mlp_desc* desc);
/* out[m, j] = x[m, cols[j]] for j < n_cols: `x[..., indices]` of the networks that read a subset of the env's observation
 * (policy_observation_indices / critic_observation_indices: rl_x/algorithms/ppo/flax/policy.py:13,33, critic.py:12,24,
 * sac/flax/policy.py:14,31, critic.py:11,23, ppo_lstm/flax_full_jit/policy.py:15,74).  x: DEVICE [M, ldx]; cols: DEVICE
 * int32[n_cols], every entry in [0, ldx); out: DEVICE [M, ldo], ldo >= n_cols (columns >= n_cols are left untouched).      */
int rlx_select_columns_f32(rlx_ctx*, const float* x, int ldx, const int32_t* cols, int n_cols, float* out, int ldo, int64_t M,
                           void* stream);


/* ---- live kernel timing for bench.py's roofline leg ------------------------------------
 * Between rlx_prof_begin and rlx_prof_end every launch of the MFMA kernels is bracketed by HIP
 * events ON THE STREAM IT IS LAUNCHED ON.  rlx_prof_end synchronises the device and returns, per
 * kernel KIND k < rlx_prof_kernel_count() (names: rlx_prof_kernel_name(k) = "k_gemm_fwd",
 * "k_gemm_dx", "k_gemm_dw", "k_dx_l1bwd", "k_l1fwd_mfma", "k_head_loss", "k_reduce_segments"; a kind covers both engines, e.g. "k_gemm_fwd" =
 * k_gemm_fwd<> and k_gemm_bx<0,...>): total milliseconds, total algorithmic FLOPs
 * (2*M*N*K per launch), total algorithmic HBM bytes (every operand once) and launch count.      */
/* rlx_dbg_set_option("prof_sample", n): only every n-th launch of each (kernel, engine, shape) row carries events (default
 * 1 = all); averages and rates are then over the sampled launches, rlx_prof_union_ms is meaningful for n == 1 only.    */
int rlx_prof_kernel_count(void);
const char* rlx_prof_kernel_name(int k);
int rlx_prof_begin(rlx_ctx* ctx);
int rlx_prof_end(rlx_ctx* ctx, double* ms_out, double* flops_out, double* bytes_out, int64_t* count_out);
/* after rlx_prof_end: the same records per (kernel kind, engine, problem shape).  `launches` counts EVERY launch of the row
 * between begin and end, `timed` those that carried events (every prof_sample-th launch of THAT ROW: the sampling counter is
 * per row, so it cannot alias with a periodic launch pattern); ms / flops / bytes are sums over the timed launches.
 * engine: 0 = exact-fp32 MFMA kernels (k_gemm_fwd / k_gemm_dx / k_gemm_dw, k_dx_l1bwd<.., false>), 1 = split-fp32 operands on
 * the fp16 pipe (k_gemm_bx<0> / k_gemm_bx<1> / k_gemm_dw_bx, k_dx_l1bwd<.., true>).  Returns the row count in *n_out
 * (rows beyond `capacity` are not written).                                                                            */
typedef struct rlx_prof_row {
  int32_t kernel;   /* index for rlx_prof_kernel_name */
  int32_t engine;
  int32_t N, K;     /* GEMM shape of the launch: C[M, N] over a contraction of K (weight gradient: C[N.., ..] see DESIGN.md) */
  int64_t M;
  int64_t launches, timed;
  double ms, flops, bytes;
} rlx_prof_row;
int rlx_prof_rows(rlx_ctx* ctx, rlx_prof_row* rows, int capacity, int* n_out);
/* after rlx_prof_end: milliseconds during which AT LEAST ONE instrumented kernel was running (union of the launch
 * intervals over all streams) -- with policy and critic on two streams the per-launch durations overlap. */
int rlx_prof_union_ms(rlx_ctx* ctx, double* out);

/* test hook: named library options (an unknown name is RLX_EINVAL).
 * "disable_l1fused" = 1 routes the first-layer backward through the unfused kernels (k_gemm_dx + k_l1<bwd> +
 *   k_gemm_dw_skinny) so both paths stay tested.
 * "l1fwd_mfma" = 0: first-layer forward of the 512-wide LayerNorm / ELU shape on the VALU kernel instead of k_l1fwd_mfma.
 * "two_streams" = 0 makes the update calls run their networks back to back on the caller's stream instead of concurrently
 *   (PPO: critic on a library-owned side stream; SAC: the policy-loss chain).
 * "pipeline_updates" = 0 restores the join between consecutive minibatch updates of rlx_ppo_update_f32 (policy and critic
 *   chains otherwise run through the whole call without meeting; the gathered rows are double buffered).
 * "fused_recurrent_act" = 0 makes rlx_ppo_lstm_act_f32 use separate launches for torso / head / sampling / critic
 *   instead of the fused decoder kernel.
 * "gemm_bx" (default 1; environment RLX_GEMM_BX=0 sets the default of new contexts to 0): the hidden-layer GEMMs of passes
 *   with >= 4096 rows run on the half-precision matrix pipe with split fp32 operands (rl-x_amd/csrc/gemm_bx.h; fp64-referenced
 *   error budget in tests/test_gpu_gemm.py); 0 = the exact-fp32 MFMA engine everywhere.
 * "bx_debug" (also read from the environment variable RLX_BX_DEBUG when the context is created): bit 16 / 32 / 64 / 128 keeps the forward / input-gradient / weight-gradient / fused first-layer-backward
 *   kernels on the exact engine, bit 256 the recurrent product of k_lstm_seq_fwd.  "bx_force_mi" = 1 / 2 forces the 64- /
 *   128-row block tile of the split-operand kernels.  rlx_dbg_gemm_f32 modes 3 / 4 / 5 run the split forms of modes 0 / 1 / 2.
 * "adam_emit" (default 1): in rlx_ppo_update_f32 / rlx_ppo_update_dist_f32 the clip + Adam kernel rewrites the weight images
 *   from the parameters it has just written (bit-identical to laying them out again); 0 = one image launch per update and net.
 * "sac_twin" (default 1): both critics of a pair in ONE launch per layer (grid.y = 2; forward passes bit-identical to two
 *   sequential passes, weight gradients summed over half as many M-slabs).
 * "bx_gscale_log2" = e: the power-of-two scale 2^e the split-operand kernels apply to their GRADIENT operand when a test
 *   calls them outside an update (rlx_dbg_gemm_f32 modes 4 / 5); inside the update calls the library sets
 *   8 * 2^ceil(log2(global minibatch rows)) itself for the duration of every backward pass (gemm_bx.h: bx_grad_scale).
 * "prof_sample": see rlx_prof_begin.
 * Round 5 (PPO update; DESIGN.md section 4.2 has the measurements): "ppo_twin" (-1 default: policy || critic as twin launches,
 *   grid.y = 2 on one stream, for minibatches of 6144 to 16384 rows -- two chains on two streams, one all-reduce each, below (with
 *   grouped gathers) and above, and at every size when the context owns an RCCL communicator of more than one rank; 0 never; 1
 *   whenever the shapes allow), "ppo_tail" (-1 default: the last hidden layer forward + head + loss + both input gradients in one
 *   launch per network -- 32-row tiles up to 8192-row minibatches and above 16384, 64-row tiles in between; 0 off; 1 / 2 force a form), "l12_fused" (1: first + second layer forward in one launch),
 *   "dw_merge" (1: the weight gradients of two layers as one two-job launch), "dw_recompute" (0: the first-layer activations
 *   rebuilt inside the weight gradient instead of stored -- correct, fewer bytes, slower), "lf_idle_cus" (0).
 * Round 5 (SAC step): "fwd2h" (1: the whole forward of a 256-256 network incl. its head, and the dQ/da chain of the policy loss,
 *   as single launches per 32-row tile -- fwd2h.hip).  (What rlx_sac_update_f32 writes and keeps is NOT an option: see
 *   rlx_sac_hparams::keep_images and the NULL-able states / next_states arguments.)
 * Round 6: "gather_records" (1: a whole-update call first lays the rollout out as one aligned record per row, [obs | action |
 *   log_prob, return, advantage | pad] of 32 / 64 / 128 floats in a library arena (134 MB at T*N = 524288), and its minibatch
 *   gathers read two cache lines per sampled row instead of six; bit-identical results; 0: gather from the five arrays).
 *   "gather_group_rows" (524288: in the two-chain schedules of rlx_ppo_update_f32 / rlx_ppo_update_dist_f32 the rows of that many samples -- one epoch at
 *   configs[1] -- are gathered by ONE launch into one of two alternating buffers, and the chains meet once per group instead of once
 *   per update; needs "gather_records").  0, or at most one minibatch, means one gather per update in the two-chain schedule of
 *   rlx_ppo_update_f32 ONLY: the twin schedule and both schedules of rlx_ppo_update_dist_f32 have a floor of 32768 rows per gather
 *   launch, so any value up to 32768 (0 included) still groups 32768 / rows-per-update updates there.
 * Round 7: "tail32_waves" (8 default; 4 or 8, anything else is RLX_EINVAL): waves per 32-row tile of k_tail32_bx, in its single,
 *   twin (grid.y = 2) and valid-rows launches alike.  8 runs the same tile with the same LDS on 512 threads -- four waves per SIMD
 *   instead of two -- with the same arithmetic in the same order: bit-identical results (tests/test_gpu_tail32_waves.py); 4 is
 *   the earlier form.
 * Round 8: "ln_row_once" (1 default; 0 or 1, anything else is RLX_EINVAL): in k_dx_l1bwd's split-operand forms and k_l12fwd every
 *   wave computes the LayerNorm mean and 1 / std of a tile's 32 rows once (one row per lane) and the per-row loops load them,
 *   instead of every lane recomputing both for each of its 16 rows at every use.  The same operations in the same order:
 *   bit-identical results (tests/test_gpu_ln_row_once.py); 0 is the earlier form.
 * Round 9: "l1_stats_handover" (1 default; 0 or 1, anything else is RLX_EINVAL): in the PPO minibatch pass k_l12fwd leaves the
 *   LayerNorm mean and 1 / std of every row in a [2][M] array next to h1 and the fused first-layer backward of the same pass loads
 *   them instead of rebuilding them from its recomputed z1.  Active only with "ln_row_once" = 1 on the split-operand engine
 *   ("gemm_bx" = 1) where the pass's forward was k_l12fwd -- there both kernels run the same code on the same rows: bit-identical
 *   results (tests/test_gpu_l1_stats_handover.py); everywhere else, and with 0, the earlier kernels run unchanged.
 * Round 10: "l1_wrap_refill" (1 default; 0 or 1, anything else is RLX_EINVAL): where "l1_stats_handover" selects the handover form
 *   of the fused first-layer backward, 1 runs it with unconditional weight-fragment refills in its main loop that wrap into the
 *   first-layer image (k_dx_l1bwd_stats_wrap: no drained wait in the K loop, no loads in the z1 recompute); the same operand words
 *   into the same MFMAs in the same order: bit-identical results (tests/test_gpu_l1_wrap_refill.py); 0, and everywhere the
 *   handover form is not selected, the earlier kernels run unchanged.
 * Round 11: "l12_prefetch" (1 default; 0 or 1, anything else is RLX_EINVAL): where k_l12fwd runs in its "ln_row_once" form with
 *   hidden[1] = 256, 1 runs k_l12fwd_pf: a row tile's z1 product takes its first-layer weight fragments from registers (the
 *   previous tile's layer-2 K loop refills its last two fragment slots from the first-layer image and requests the rest behind its
 *   last product; a workgroup's first tile requests all eight before anything else), the next tile's observation loads follow
 *   them and are staged behind the K loop, and no spilled register is reloaded at the tile top.  The same operand words into the
 *   same MFMAs in the same order, the same stores: bit-identical results (tests/test_gpu_l12_prefetch.py); 0, hidden[1] = 512,
 *   "ln_row_once" = 0 and every caller that does not take the k_l12fwd path run the earlier kernels unchanged.
 * Round 12: "rollout_persistent" (1 default; 0 or 1, anything else is RLX_EINVAL): 1 lets rlx_ppo_rollout_f32 run the acting
 *   steps as ceil(T / rollout_chunk_steps) launches of k_rollout_steps, each of which carries its 32-row tiles through several
 *   steps (parameters, head weights, episode counters and the observation tile stay on chip between steps; the critic
 *   workgroups rebuild their observations from the env's own functions, so no workgroup waits for another) -- where both nets
 *   have hidden[0] = 512, two or three hidden layers and weight images from rlx_ppo_rollout_begin; everywhere else, with
 *   "ro_exit" or stamps set, and with 0, the T launches of k_rollout_step run unchanged.  The same operations in the same order:
 *   bit-identical results (tests/test_gpu_rollout_persistent.py).  "rollout_chunk_steps" (32 default; 1 .. 64, anything else
 *   is RLX_EINVAL): acting steps per launch of k_rollout_steps; the results do not depend on it.
 * Round 13: "tail32_lean" (1 default; 0 or 1, anything else is RLX_EINVAL): with "tail32_waves" = 8, 1 runs k_tail32_bx_lean in
 *   every launch of the 32-row tail (single, twin, valid-rows): the head weights sit in LDS with 16 bytes of padding per eight
 *   rows (the head's reads are conflict-free instead of 8-way), the metric fold and the bias / logstd column sums run on waves
 *   4 and 5 beside the head's weight-gradient partials (the metric sums have LDS slots of their own: one barrier fewer), and those
 *   partials cross row groups as 16-byte LDS stores and loads; 65920 instead of 65600 bytes of LDS.  Every sum keeps its operands
 *   and their order: bit-identical results (tests/test_gpu_tail32_lean.py); 0, and "tail32_waves" = 4, run the earlier kernels
 *   unchanged.
 * "espo_chunk" (2): rlx_espo_update_f32 submits that many epochs between two copies of its device-side stop word to the host
 *   (at most two chunks of epochs run as wasted work after a stop); the result does not depend on it.
 * (The measured-negative experiments of rounds 2-4 -- hipGraph replay, fused forward, 64-row / pipelined first-layer backward,
 *  split recurrent chains, plane-tensor GEMMs with direct-to-LDS staging, ... -- are documented in DESIGN.md Appendix A; their
 *  code lives in the git history only.)                                                                                    */
int rlx_dbg_set_option(rlx_ctx* ctx, const char* name, int value);
/* test hooks: "scratch_ptr:<bank>:<slot>" / "scratch_bytes:<bank>:<slot>" = device address / size of a library-owned scratch
 * arena (lets a test inspect intermediates); "allreduce_calls" = collectives this context has issued so far (through its RCCL
 * communicator or the all-reduce hook) -- bench.py's multi_gpu.collectives_per_step is the difference over the timed steps;
 * "dx_l1bwd_wrap_launches" = launches of k_dx_l1bwd_stats_wrap so far (option "l1_wrap_refill"; the profiler books both forms of
 * the kernel under one row); "l12fwd_pf_launches" = launches of k_l12fwd_pf so far (option "l12_prefetch"; the profiler books both
 * forms of k_l12fwd under one row); "bx_window_fallbacks" = rollouts (rlx_ppo_rollout_begin) that found a weight of the acting nets at or above 1023 -- outside
 * the fp16 window of the split-operand engine -- and therefore ran their T steps on the exact-fp32 engine; "gemm_bx" = the
 * current value of that option; "ro_persistent_launches" / "ro_step_launches" = launches of k_rollout_steps / of
 * k_rollout_step so far (option "rollout_persistent": which path a rollout took); "ro_critic_es_ptr" = device address of the
 * int32 [N] episode-step counters the critic workgroups of the last persistent rollout kept (equal to ep_step after it)  */
int rlx_dbg_get_counter(rlx_ctx* ctx, const char* name, int64_t* out);

/* test hook: the next rlx_sac_update_f32 calls take their N(0,1) draws from eps_next / eps_cur (DEVICE [B, A] each: the
 * next-state and current-state policy samples) instead of the per-sample threefry keys -- lets a test feed the update the
 * noise a reference run consumed.  NULL, NULL restores the PRNG.  The key schedule (key_io) is unaffected.            */
int rlx_dbg_set_sac_noise(rlx_ctx* ctx, const float* eps_next, const float* eps_cur);

/* tuning hook: instrumented kernels (fwd2h.hip: k_fwd2h) write clock64() stamps of their phases, taken by thread 0 of workgroup
 * (0, 0), to stamps[0 .. 16) (DEVICE, 16 x uint64).  NULL switches the stamps off.                                          */
int rlx_dbg_set_stamps(rlx_ctx* ctx, void* stamps);

/* debug / micro-benchmark hook: run ONE of the exact-fp32 MFMA GEMM kernels on caller buffers.
 *   mode 0: C[M,N]  = act(A[M,K] @ B[K,N] + aux[N])                 forward hidden layer
 *   mode 1: C[M,K] <- (A[M,N] @ B[K,N]^T) * act'(C[M,K]) in place   input gradient (act < 0: no act')
 *   mode 2: C[K,N]  = A[M,K]^T @ B[M,N]; aux[N] = column sums of B  weight gradient (split-M + reduce) */
int rlx_dbg_gemm_f32(rlx_ctx* ctx, int mode, const float* A, const float* B, float* C, float* aux, int64_t M, int N,
                     int K, int act, void* stream);

/* debug / micro-benchmark hook: the fused first layer (Dense + LayerNorm + activation) alone.
 * bwd = 0: H[M,Hd] = act(LN(X[M,O] @ W[O,Hd] + b));  bwd = 1: H holds dL/dH on entry and
 * dL/dZ1 on exit, ln_partials[grid][2*Hd] receives per-workgroup d(ln scale), d(ln bias).     */
int rlx_dbg_l1_f32(rlx_ctx* ctx, int bwd, const float* X, const float* W, const float* b, const float* g,
                   const float* be, float* H, float* ln_partials, int64_t M, int O, int Hd, int act, int ln, int grid,
                   void* stream);

/* ---- PRNG: jax.random restated (third-party jax<=0.7.2, not in the reference tree) --
 * call sites: rl_x/algorithms/ppo/flax/ppo.py:64-65,114-115,191-193                    */
/* host: `keys = jax.random.split(key, num)`; key_in/keys_out are HOST uint32 arrays     */
int rlx_threefry_split_host(const uint32_t key_in[2], uint32_t* keys_out /*[num,2]*/, int num, int scheme);
/* device: `_random_bits(key, 32, [n])` -> uint32[n]                                     */
int rlx_random_bits_u32(rlx_ctx*, const uint32_t key[2], uint32_t* out, int64_t n, int scheme, void* stream);
/* device: `jax.random.normal(key, [n])` -> float32[n] (Giles erfinv, like XLA f32)      */
int rlx_normal_f32(rlx_ctx*, const uint32_t key[2], float* out, int64_t n, int scheme, void* stream);
/* `key, sub = split(key); idx = permutation(sub, tile(arange(B),(E,1)), axis=1, independent=True)`
 * replaces rl_x/algorithms/ppo/flax/ppo.py:191-193.  key_io (HOST uint32[2]) is advanced in
 * place; out is DEVICE int32[E*B]; bit-exact w.r.t. jax (stable ascending sort per row,
 * ceil(3 ln(E*B)/ln(2^32-1)) rounds).                                                   */
int rlx_permutation_i32(rlx_ctx*, uint32_t key_io[2], int32_t* out, int E, int64_t B, int scheme, void* stream);

/* ---- synthetic random-observation env (the build's own) -------------
 * env object contract mirrored: rl_x/environments/custom_mujoco/ant/warp_torch/environment.py:142-186 */
int rlx_env_reset_f32(rlx_ctx*, uint32_t seed, int env_id_offset, int N, int obs_dim, int horizon,
                      float* obs /*[N,O]*/, int32_t* ep_step /*[N]*/, float* ep_ret /*[N]*/,
                      float* last_ret /*[N]*/, float* last_len /*[N]*/, void* stream);
int rlx_env_step_f32(rlx_ctx*, uint32_t seed, int env_id_offset, uint32_t t, int N, int obs_dim, int act_dim,
                     int horizon, float p_term, float reward_noise,
                     const float* action /*[N,A]*/, float* obs /*[N,O] in: current, out: post-reset next*/,
                     float* final_obs /*[N,O] pre-reset next obs (Batch.next_states row)*/,
                     float* reward /*[N]*/, float* terminated /*[N] 0/1*/, float* truncated /*[N] 0/1*/,
                     int32_t* ep_step, float* ep_ret, float* last_ret, float* last_len,
                     float* episode_stats /*dev [4] += {finished episodes, sum return, sum length, 0} or NULL*/,
                     void* stream);
/* the same step that also stores the PRE-step observation (the one the action was computed from) into prev_obs_out [N,O]
 * (NULL: none) -- the `states` row of the replay ring slot this transition fills (sac/flax/replay_buffer.py:23): one copy
 * launch less per vector step */
int rlx_env_step_copy_f32(rlx_ctx*, uint32_t seed, int env_id_offset, uint32_t t, int N, int obs_dim, int act_dim,
                          int horizon, float p_term, float reward_noise, const float* action, float* obs, float* final_obs,
                          float* reward, float* terminated, float* truncated, int32_t* ep_step, float* ep_ret,
                          float* last_ret, float* last_len, float* episode_stats, float* prev_obs_out, void* stream);

/* ---- acting: `get_action_and_value`, rl_x/algorithms/ppo/flax/ppo.py:110-119 ---------
 * (full-jit twin rl_x/algorithms/ppo/flax_full_jit/ppo.py:133-140).  key_io HOST uint32[2]
 * advanced like `key, subkey = split(key)`; noise = normal(subkey, [N_global,A]) rows
 * [env_id_offset, env_id_offset+N) so a sharded run draws the same noise as one device.
 * Also copies obs into states_row (Batch.states[t]) when states_row != NULL.             */
int rlx_actor_critic_fwd_sample_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams,
                                    const rlx_mlp_desc* cdesc, const float* cparams,
                                    const float* obs /*[N,O]*/, const float* critic_obs /*[N, cdesc->in_dim] or NULL: = obs*/,
                                    uint32_t key_io[2], int scheme,
                                    float* action /*[N,A]*/, float* processed /*[N,A] or NULL*/,
                                    float* value /*[N]*/, float* logp /*[N]*/, float* states_row /*[N,O] or NULL*/,
                                    int N, int clip_and_rescale, const float* act_low /*dev [A] or NULL*/,
                                    const float* act_high, int env_id_offset, int N_global, void* stream);
/* Categorical twin of rlx_actor_critic_fwd_sample_f32 for discrete action spaces (DiscreteFlatValuesPolicy,
 * rl_x/algorithms/ppo/pytorch/policy.py:96-135 -- the reference's only discrete PPO head; BASELINE.json configs[0],
 * CartPole): pdesc->out_dim = number of actions (2..8), has_logstd = 0.  action [N] = sampled index as float
 * (argmax(logits + Gumbel noise), the jax.random.categorical construction on the threefry stream; deterministic != 0:
 * argmax(logits), key untouched), logp [N] = log_softmax(logits)[action], value [N].                                  */
int rlx_actor_critic_fwd_sample_discrete_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams,
                                             const rlx_mlp_desc* cdesc, const float* cparams, const float* obs /*[N,O]*/,
                                             uint32_t key_io[2], int scheme, float* action /*[N]*/, float* value /*[N]*/,
                                             float* logp /*[N]*/, float* states_row /*[N,O] or NULL*/, int N,
                                             int env_id_offset, int N_global, int deterministic, void* stream);
/* ---- fused acting step: ONE launch = policy fwd + critic fwd + sample + log-prob
 * (+ the synthetic env transition when fuse_env != 0).  Same semantics and key schedule as
 * rlx_actor_critic_fwd_sample_f32 followed by rlx_env_step_f32, i.e. one iteration of the acting
 * loop rl_x/algorithms/ppo/flax/ppo.py:275-296 (full-jit: ppo/flax_full_jit/ppo.py:130-153).
 * Observations are double buffered by the caller: obs_in = Batch.states[t] (read only),
 * obs_out = Batch.states[t+1] (post-reset next observation, written when fuse_env).
 * rlx_ppo_rollout_step_supported() tells whether the network shapes fit the fused kernel
 * (1 <= in_dim <= 32, one to three hidden layers, hidden[0] % 64 == 0 and in [64, 512], later hidden layers 128 or 256 wide,
 * 1 <= out_dim <= 32 -- a single hidden layer of 512 with 32 outputs included: its head is staged across the two LDS regions
 * that are free then -- the same in_dim for both nets, a policy with logstd, a critic with one output).                      */
int rlx_ppo_rollout_step_supported(const rlx_mlp_desc* pdesc, const rlx_mlp_desc* cdesc);
/* Optional bracket around the T acting steps of one rollout: rlx_ppo_rollout_begin lays out the split-fp16 weight images of the
 * hidden layers l >= 1 of both nets (one small launch; gemm_bx option), and the rlx_ppo_rollout_step_f32 calls that follow with
 * the SAME parameter pointers run those layers on the fp16 matrix pipe (no LDS weight stage, no barrier in the K loop).
 * CONTRACT: the parameters must not change between begin and the last step that should use the images; every
 * parameter-updating entry point of this library (rlx_ppo_update_f32, rlx_ppo_update_dist_f32, rlx_clip_adam_step_f32) and
 * rlx_ppo_rollout_end drop them.  A caller that writes the parameter buffers itself (checkpoint load) must call
 * rlx_ppo_rollout_end (or begin again).  Without a begin the steps use the exact-fp32 layers.
 * Engine window: begin first takes max |parameter| of both nets (two small launches + ONE blocking 8-byte read per rollout); a
 * weight at or above 1023 would overflow its fp16 image, so in that case no images are laid out, the T steps run on the exact-fp32
 * layers and the counter "bx_window_fallbacks" (rlx_dbg_get_counter) is incremented.                                          */
int rlx_ppo_rollout_begin(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, const float* pparams, const rlx_mlp_desc* cdesc,
                          const float* cparams, void* stream);
int rlx_ppo_rollout_end(rlx_ctx* ctx);
int rlx_ppo_rollout_step_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, const rlx_mlp_desc* cdesc,
                             const float* cparams, const float* obs_in /*[N,O]*/, float* obs_out /*[N,O] or NULL*/,
                             uint32_t key_io[2], int scheme, float* action /*[N,A]*/, float* processed /*[N,A] or NULL*/,
                             float* value /*[N]*/, float* logp /*[N]*/, int N, int clip_and_rescale,
                             const float* act_low, const float* act_high, int noise_row_offset, int N_global,
                             int fuse_env, uint32_t env_seed, int env_id_offset, uint32_t env_t, int horizon,
                             float p_term, float reward_noise, float* final_obs /*[N,O]*/, float* reward /*[N]*/,
                             float* terminated /*[N]*/, int32_t* ep_step, float* ep_ret, float* last_ret,
                             float* last_len, float* episode_stats /*[4] or NULL*/, void* stream);

/* The T iterations of the acting loop (rl_x/algorithms/ppo/flax/ppo.py:275-296) queued by ONE call: step t reads states[t] and
 * writes actions[t], values[t], logps[t], final_obs[t], rewards[t], terminated[t] and the post-reset next observation into
 * states[t+1] (obs_last for t = T-1); the env clock of step t is env_t0 + t; key_io advances by T splits.  Same launches, keys
 * and results as T calls of rlx_ppo_rollout_step_f32 with fuse_env = 1 and processed = NULL (bit-identical:
 * tests/test_gpu_rollout.py) -- what changes is the host: it leaves the loop after ~0.5 ms instead of ~3 ms of per-step binding
 * overhead, so whatever the caller queues next (rlx_ppo_prefetch_permutation, GAE, the update) reaches the GPU while it still
 * runs the rollout.  With the option "rollout_persistent" (default) and a network inside k_rollout_steps' envelope the T steps
 * run as ceil(T / rollout_chunk_steps) launches instead of T; keys, results and error returns are the same.                  */
int rlx_ppo_rollout_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, const rlx_mlp_desc* cdesc,
                        const float* cparams, float* states /*[T,N,O]*/, float* obs_last /*[N,O]*/, uint32_t key_io[2],
                        int scheme, float* actions /*[T,N,A]*/, float* values /*[T,N]*/, float* logps /*[T,N]*/, int T, int N,
                        int clip_and_rescale, const float* act_low, const float* act_high, int noise_row_offset, int N_global,
                        uint32_t env_seed, int env_id_offset, uint32_t env_t0, int horizon, float p_term, float reward_noise,
                        float* final_obs /*[T,N,O]*/, float* rewards /*[T,N]*/, float* terminated /*[T,N]*/, int32_t* ep_step,
                        float* ep_ret, float* last_ret, float* last_len, float* episode_stats /*[4] or NULL*/, void* stream);

/* generic MLP forward: out[n,out_dim] = net(x[n,in_dim]);  critic on next_states
 * (rl_x/algorithms/ppo/flax/ppo.py:129) and deterministic actions (:235-238).            */
int rlx_mlp_fwd_f32(rlx_ctx*, const rlx_mlp_desc* desc, const float* params, const float* x, float* out,
                    int64_t n, void* stream);

/* ---- `next_values = critic(next_states)` of calculate_gae_advantages (rl_x/algorithms/ppo/flax/ppo.py:129) for a rollout
 * whose values[t] = critic(states[t]) were produced with the SAME critic parameters: next_values[t] = values[t+1] wherever
 * next_states[t] == states[t+1] bit for bit (all rows but the final-observation ones, ppo.py:277-286); the remaining rows
 * and the last step go through the critic.  The row selection, its length and the scatter stay on the device (no host
 * synchronisation); the result equals rlx_mlp_fwd_f32 on all T*N rows bit for bit.  All arrays time-major [T,N(,O)].    */
int rlx_ppo_next_values_f32(rlx_ctx*, const rlx_mlp_desc* cdesc, const float* cparams, const float* states,
                            const float* next_states, const float* values, float* next_values, int T, int N, void* stream);

/* ---- the iteration's logged scalars (rl_x/algorithms/ppo/flax/ppo.py:215-216, 226-230, 300-307) reduced ON THE DEVICE in two
 * library launches: out12[0..9] = column means of the [n_updates, 10] per-update metric rows of rlx_ppo_update_f32,
 * out12[10] = explained variance 1 - var(returns - values) / (var(returns) + 1e-8) over the n = T * N rollout entries
 * (population variances, fp64 sums in a fixed order), out12[11] = mean(exp(logstd[0..act_dim))) (logstd NULL: 0, the
 * Categorical policy).  All pointers DEVICE; the caller copies the 12 floats to the host once per iteration.              */
int rlx_ppo_reduce_metrics_f32(rlx_ctx*, const float* metrics, int n_updates, const float* returns, const float* values,
                               int64_t n, const float* logstd, int act_dim, float* out12, void* stream);

/* ---- GAE: `calculate_gae_advantages`, rl_x/algorithms/ppo/flax/ppo.py:122-135 --------
 * all arrays [T,N]; masks with terminations only (no reset at truncation).               */
int rlx_gae_f32(rlx_ctx*, const float* rewards, const float* values, const float* next_values,
                const float* terminations, float* advantages, float* returns, int T, int N, float gamma,
                float gae_lambda, void* stream);

/* ---- one minibatch: gather + advantage normalisation + loss + grads ------------------
 * replaces `minibatch_update` up to value_and_grad, rl_x/algorithms/ppo/flax/ppo.py:196-210
 * with loss_fn :142-177.  idx: DEVICE int32[mb_local] (flattened i = t*N+n).  Advantages are
 * normalised with mean/std over the gathered minibatch (population std, + 1e-8).
 * grads: DEVICE, same flat layout as params (policy then separate critic buffer).
 * metrics: DEVICE float[8] = {pg_loss, critic_loss, entropy_loss, approx_kl, clip_fraction,
 * adv_mean, adv_std, reserved} (means over the GLOBAL minibatch; the combined loss is
 * pg - entropy_coef*entropy + critic_coef*critic, linear in these means).
 * stats_io: NULL, or DEVICE double[4] for the multi-GPU two-phase protocol:
 *   phase 0 gathers the local rows and writes {sum_adv, sum_adv2, count, 0}, then returns;
 *   the host all-reduces stats_io (and sums mb_local into mb_global); phase 1 consumes the
 *   reduced sums, uses 1/mb_global as the loss denominator and produces LOCAL gradient /
 *   metric contributions that the host all-reduces (sum).  phase 2 = gather + consume
 *   externally supplied global sums in one call (batched statistics).
 *   phase 3 / 4 = phase 2 in halves: 3 gathers and runs the POLICY net only (cgrads may be NULL),
 *   4 runs the CRITIC net on the rows phase 3 gathered (pgrads may be NULL; `metrics` receives only
 *   the critic loss) -- lets the host all-reduce the policy gradients while the critic computes.
 *   phase 5 = gather + consume the supplied sums ONLY (no net); phase 6 = POLICY net on the gathered rows; with
 *   5 -> {6 on one stream, 4 on another} the host runs the two nets concurrently (the critic half uses its own
 *   activation / slab arenas).
 *   Single GPU: stats_io = NULL (phase ignored).                                         */
int rlx_ppo_minibatch_fwd_bwd_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, float* pgrads,
                                  const rlx_mlp_desc* cdesc, const float* cparams, float* cgrads,
                                  float* metrics, const float* states, const float* actions,
                                  const float* log_probs, const float* returns, const float* advantages,
                                  const int32_t* idx, int mb_local, int mb_global, double* stats_io, int phase,
                                  const rlx_ppo_hparams* hp, void* stream);

/* ---- optimizer: optax.chain(clip_by_global_norm, adam), ppo/flax/ppo.py:84-100,212-213 */
int rlx_grad_global_norm_f32(rlx_ctx*, const float* grads, int64_t n, float* norm_out /*dev [1]*/, void* stream);
/* step is 1-based (optax count+1); lr evaluated by the host (linear_schedule, ppo.py:76-80);
 * grad_norm_out (dev [1]) receives the pre-clip global norm (metric, ppo.py:215-216).
 * NON-FINITE GRADIENTS (every Adam kernel of this library: this entry point, the PPO / PPO+LSTM update calls,
 * rlx_sac_update_f32, the FastSAC updates): when a network's global gradient norm is not finite its step is SKIPPED on the device
 * -- parameters, both moments, a fused Polyak target update and the weight-image rewrite are all left as they were -- and the
 * non-finite norm is still reported in the metrics.  The host-side step counter (opt_count_io / `step`) advances regardless, so
 * the bias correction of later steps is that of the advanced count.  This DEVIATES from the reference, deliberately: optax / JAX
 * would write the NaN into the parameters, torch.optim in FastSAC would do the same and still run its Polyak step.  The plugins
 * check the reported norms once per logged interval and stop (or, ppo.hip, redo the update on the exact-fp32 engine first).  */
int rlx_clip_adam_step_f32(rlx_ctx*, float* params, const float* grads, float* m, float* v, int64_t n_params,
                           int64_t step, float lr, float max_grad_norm, float b1, float b2, float eps,
                           float* grad_norm_out, void* stream);

/* ---- whole `update`: rl_x/algorithms/ppo/flax/ppo.py:138-232 -------------------------
 * runs nr_epochs*nr_minibatches minibatch updates (permutation + the two calls above) on
 * `stream`.  opt_count_io (HOST int64) = optimizer steps so far, advanced by E*M.
 * lr_schedule: HOST float[E*M] learning rate per update (host evaluates linear_schedule).
 * metrics_out: DEVICE float[E*M, 10] = the 8 minibatch metrics + policy_grad_norm +
 * critic_grad_norm per update (the reference means them over updates, ppo.py:226).        */
/* optional: generate -- on the library's side stream, ordered after the PREVIOUS rlx_ppo_update_f32 of this context
 * (its last read of the permutation buffer; before the first update: after the work already queued on `stream`), i.e.
 * UNDER the rollout whether the caller queues it before or after this call -- the permutation the NEXT
 * rlx_ppo_update_f32 call will need.  key_at_update (HOST) = the key that call will receive: the current key
 * advanced by the T acting splits, which are data independent.  A later update whose key_io / nr_epochs / T*N /
 * scheme match consumes it (its stream waits for the generation to finish); otherwise it is discarded.        */
int rlx_ppo_prefetch_permutation(rlx_ctx*, const uint32_t key_at_update[2], int nr_epochs, int64_t B, int scheme,
                                 void* stream);
/* ======================= data-parallel job: one process per GPU, RCCL over xGMI =======================
 * The reference has no multi-device path; contract = BASELINE.json north_star + SURVEY.md 8(b)/(e).
 * Envs -- and with them every [T, N, .] rollout array -- are sharded over the ranks (rank g owns the GLOBAL env ids
 * [env_id_offset, env_id_offset + N_local)); parameters, Adam moments and the PRNG key are replicated; the minibatch
 * permutation (ppo/flax/ppo.py:191-194) is computed identically on every rank over the GLOBAL index space
 * i = t * N_global + n; each rank runs the minibatch kernels on its local rows, normalising advantages with the
 * all-reduced statistics and scaling the loss by 1 / minibatch_size(global); the flat gradient vectors are summed over
 * the ranks with ncclAllReduce issued BY THE LIBRARY (no host callback), then clip + Adam run redundantly.
 *
 * RCCL is bound at run time (the process must hold one RCCL: the one PyTorch-ROCm mapped): rlx_dist_load_rccl(path)
 * with path = <torch>/lib/librccl.so, NULL = search (already-mapped symbols, $RLX_RCCL_LIBRARY, librccl.so).        */
/* what the RCCL entry points were bound to: the path of the copy this process had already mapped (PyTorch-ROCm's), "(global
 * symbols)", or the candidate a fresh copy was loaded from when none was mapped; "" before the first bind.  The library never
 * loads a second RCCL next to a mapped one.                                                                              */
const char* rlx_dist_rccl_path(void);
int rlx_dist_load_rccl(const char* path);
/* rank 0: ncclGetUniqueId -> id_out (HOST, 128 bytes); the host broadcasts it to the other ranks (any transport)      */
int rlx_dist_unique_id(void* id_out);
/* context of rank `rank` of `world`; a non-NULL id creates the communicator (ncclCommInitRank, collective
 * over all ranks) and the stream all collectives of this context are issued on.  world == 1 with id == NULL is
 * rlx_ctx_create; world == 1 WITH an id is a one-rank job whose collectives are still enqueued on RCCL (tests).      */
int rlx_ctx_create_dist(int device, int rank, int world, const void* nccl_unique_id /*128 B, or NULL iff world == 1*/,
                        rlx_ctx** out);
int rlx_ctx_rank(const rlx_ctx* ctx, int* rank_out, int* world_out);
/* ranks of the context's RCCL communicator as RCCL itself reports them (ncclCommCount); 0 when the context owns no
 * communicator (single rank, or collectives routed through the test hook) -- bench.py prints it next to n_gpus          */
int rlx_dist_comm_count(const rlx_ctx* ctx, int* count_out);
/* sum buf[n] (DEVICE fp32) over the ranks in place, ordered after the work queued on `stream` and before what is queued
 * on it next (SURVEY.md 8(b) export set; the update below calls the same routine internally)                            */
int rlx_allreduce_grads(rlx_ctx*, float* buf, int64_t n, void* stream);
/* rows a rank-local minibatch is padded to: the launch shapes of the data-parallel update are fixed (mean + 6.5 sigma of
 * the local row count, rounded up to 128; == minibatch_size when N_local == N_global); padding rows carry zero weight    */
int rlx_dist_row_capacity(int minibatch_size_global, int n_local, int n_global);
/* K4b: restrict the global permutation to this rank.  perm: DEVICE int32 [n_minibatches, minibatch_size_global] global
 * flattened indices; lidx: DEVICE int32 [n_minibatches, cap] receives, per minibatch and in permutation order, the LOCAL
 * flattened indices t * N_local + (n - env_id_offset) of the rows that live here; counts: DEVICE int32 [n_minibatches].   */
int rlx_dist_local_rows_i32(rlx_ctx*, const int32_t* perm, int n_minibatches, int minibatch_size_global, int n_local,
                            int n_global, int env_id_offset, int cap, int32_t* lidx, int32_t* counts, void* stream);
/* Capacity overflows since the last call (blocking on `stream`, where the read and the reset are ordered behind the updates
 * issued on it; reading resets both counters).  *rows_any_rank: rows dropped by ANY rank, taken from slot 3 of the per-minibatch
 * statistics records that rlx_ppo_update_dist_f32 all-reduces anyway -- identical on every rank, so a job that treats non-zero
 * as an error (the excess rows were dropped; probability < 1e-10 per minibatch) fails on ALL ranks in the same iteration and no
 * rank is left waiting in a collective for one that raised.  *minibatches_this_rank (may be NULL): minibatches THIS rank
 * truncated, including calls of rlx_dist_local_rows_i32 outside an update -- rank-local, a diagnostic only.               */
int rlx_dist_overflow_count(rlx_ctx*, int* rows_any_rank, int* minibatches_this_rank, void* stream);
/* optional, under the rollout: permutation + local-row restriction of the NEXT rlx_ppo_update_dist_f32 on the library's
 * side stream (same contract as rlx_ppo_prefetch_permutation)                                                         */
int rlx_ppo_dist_prefetch(rlx_ctx*, const uint32_t key_at_update[2], int nr_epochs, int T, int n_local, int n_global,
                          int env_id_offset, int minibatch_size_global, int scheme, void* stream);
/* the whole `update` (ppo/flax/ppo.py:138-232) on ONE RANK: rollout arrays are this rank's shard [T, N_local, .];
 * minibatch_size is GLOBAL (T * N_global must be a multiple of it); key_io / opt_count_io / lr_schedule / metrics_out as
 * rlx_ppo_update_f32.  Collectives per call: 1 (advantage sums, fp64 [E*M, 4]) + 2 * E*M (gradients) + 1 (metrics).
 * metrics_out holds the GLOBAL values on every rank.  Policy chain on `stream`, critic chain on the side stream, no
 * join between updates.  With one rank (and no hook) no collective is issued and the results equal rlx_ppo_update_f32's. */
int rlx_ppo_update_dist_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
                            const rlx_mlp_desc* cdesc, float* cparams, float* cm, float* cv, const float* states,
                            const float* actions, const float* log_probs, const float* returns, const float* advantages,
                            int T, int n_local, int n_global, int env_id_offset, int nr_epochs, int minibatch_size,
                            uint32_t key_io[2], int scheme, int64_t* opt_count_io, const float* lr_schedule,
                            const rlx_ppo_hparams* hp, float* metrics_out, void* stream);
/* test hooks: (1) stand-in for the collectives -- fn(user, buf, n, dtype (0 fp32, 1 fp64), on_side_stream) must sum buf
 * over the (emulated / gloo) ranks in place with work queued on the caller's stream (on_side_stream = 0) or on
 * rlx_ctx_side_stream (= 1); NULL restores RCCL.  (2) rank / world of a context WITHOUT communicator (emulated ranks).  */
typedef int (*rlx_allreduce_fn)(void* user, void* buf, int64_t n, int dtype, int on_side_stream);
int rlx_dbg_set_allreduce_hook(rlx_ctx*, rlx_allreduce_fn fn, void* user);
int rlx_dbg_set_rank(rlx_ctx*, int rank, int world);
/* the library-owned side stream (hipStream_t) of this context, created on first use */
void* rlx_ctx_side_stream(rlx_ctx*);
int rlx_ppo_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
                       const rlx_mlp_desc* cdesc, float* cparams, float* cm, float* cv,
                       const float* states, const float* actions, const float* log_probs,
                       const float* returns, const float* advantages, int T, int N,
                       int nr_epochs, int minibatch_size, uint32_t key_io[2], int scheme,
                       int64_t* opt_count_io, const float* lr_schedule, const rlx_ppo_hparams* hp,
                       float* metrics_out, void* stream);

/* ======================================= SAC ==========================================
 * Networks (flat layout as above): policy = MLP with out_dim = 2*act_dim, head columns
 * [0,A) = mean, [A,2A) = raw log_std (rl_x/algorithms/sac/flax/policy.py:31-41), no logstd param;
 * critic = TWO MLPs back to back (Q0 then Q1), each in_dim = obs+act, out_dim = 1
 * (rl_x/algorithms/sac/flax/critic.py:17-53); log_alpha = one float (entropy_coefficient.py:5-11). */
typedef struct rlx_sac_hparams {
  float gamma, tau, target_entropy;
  float log_std_min, log_std_max;
  float lr_policy, lr_critic, lr_alpha; /* host evaluates the schedule (sac.py:79-87) */
  float adam_b1, adam_b2, adam_eps;
  int32_t key_schedule; /* 0: host-loop flavour, keys = split(key, 2B+1), noise keys interleaved (sac/flax/sac.py:195-197);
                         * 1: fully jitted flavour, keys = split(key, 2B+2), keys[1] = replay-sampling key, noise keys in two
                         *    contiguous blocks (sac/flax_full_jit/sac.py:273-275)                                           */
  const float* critic_states;      /* NULL, or DEVICE [B, qdesc->in_dim - act_dim]: the critics' own observation columns of the   */
  const float* critic_next_states; /* sampled transitions (`x[..., critic_observation_indices]`, sac/flax/critic.py:11,23);
                                    * states / next_states then hold the policy's columns [B, pdesc->in_dim] (policy.py:14,31) */
  /* Data parallel (one process per GPU): this rank holds rows [batch_row_offset, batch_row_offset + B) of a
   * global batch of batch_global samples.  0 = the B rows are the whole batch.  With batch_global > B the losses are scaled
   * by 1 / batch_global, sample i draws its noise from key index batch_row_offset + i of split(key, 2 * batch_global + 1),
   * and ONE all-reduce (the context's RCCL communicator, rlx_dist_*) sums [policy grads | critic grads | loss sums] before
   * the three Adam steps, which every rank applies redundantly: parameters stay bit-identical across ranks.            */
  int64_t batch_global;
  int64_t batch_row_offset;
  /* Optional replay source (all NULL / 0: the batch arguments of rlx_sac_update_f32 already hold the transitions).  With
   * ring_states != NULL the update first gathers transition i = ring[ring_idx1[i], ring_idx2[i]] exactly like
   * rlx_sac_replay_sample_f32 -- INTO the batch arguments (states, next_states, actions, rewards, terminations are then
   * outputs as well) -- in the launch that lays out the critics' input rows: one launch and one call less per update.  */
  const float *ring_states, *ring_next_states, *ring_actions, *ring_rewards, *ring_terminations; /* [capacity, nr_envs, .] */
  const int32_t *ring_idx1, *ring_idx2;                                                          /* DEVICE int32 [B]       */
  int32_t ring_nr_envs;
  /* keep_images != 0 (batches >= 4096 rows): the five networks' split fp16 weight images stay in a library-owned arena after this
   * call -- the optimizer launch rewrites them from the parameters / Polyak targets it stores -- and the next rlx_sac_update_f32 /
   * rlx_sac_act_f32 call on the SAME parameter pointers and descriptors uses them instead of laying the images out again.  By
   * passing keep_images != 0 the caller states, for THIS call, that pparams / qparams / qtarget have not been written by anybody
   * but rlx_sac_update_f32 since its previous keep_images call on this context; after writing them (load, broadcast, a test poking
   * weights) call rlx_sac_invalidate_images first.  0: images are laid out per call and none are kept (any kept ones are dropped). */
  int32_t keep_images;
} rlx_sac_hparams;

/* drops the weight images a keep_images update left on the context: call it after writing SAC parameter / target vectors from
 * outside rlx_sac_update_f32 (the next update / acting call lays them out again from the parameters).  Always RLX_OK.   */
int rlx_sac_invalidate_images(rlx_ctx*);

/* `ReplayBuffer.sample` gather (rl_x/algorithms/sac/flax/replay_buffer.py:30-38) from the
 * device-resident ring [capacity, nr_envs, .]; idx1/idx2 are DEVICE int32[B] (drawn on the host with
 * numpy's Generator exactly like the reference: rng.integers(size), rng.integers(nr_envs)).        */
int rlx_sac_replay_sample_f32(rlx_ctx*, const float* ring_states, const float* ring_next_states,
                              const float* ring_actions, const float* ring_rewards, const float* ring_terminations,
                              int nr_envs, int obs_dim, int act_dim, const int32_t* idx1, const int32_t* idx2, int64_t B,
                              float* states, float* next_states, float* actions, float* rewards, float* terminations,
                              void* stream);
/* the fully jitted flavour's index draw (sac/flax_full_jit/sac.py:273-282) on the device: replay_key = split(update_key,
 * 2B+2)[1]; idx1 = randint(replay_key, (B,), 0, size); idx2 = randint(replay_key, (B,), 0, nr_envs) -- the SAME key for
 * both, as the reference has it.  update_key (HOST) = the key the following rlx_sac_update_f32 (key_schedule = 1) receives. */
int rlx_sac_replay_draw_i32(rlx_ctx*, const uint32_t update_key[2], int scheme, int64_t B, int size, int nr_envs,
                            int32_t* idx1 /*dev [B]*/, int32_t* idx2 /*dev [B]*/, void* stream);
/* `get_action` (sac.py:119-125): key, sub = split(key); action = tanh(mean + std * normal(sub, [N_global, A])[rows]);
 * deterministic != 0: tanh(mean), key untouched (sac.py:217-221).                                   */
int rlx_sac_act_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, const float* obs /*[N,O]*/,
                    uint32_t key_io[2], int scheme, float* action /*[N,A]*/, int N, float log_std_min,
                    float log_std_max, int deterministic, int row_offset, int N_global, void* stream);
/* rlx_sac_act_f32 plus, from the same launch, the action the env receives -- `get_processed_action`
 * (sac/flax/policy.py:44-48): processed[n, j] = low[j] + (clip(action[n, j], -1, 1) + 1) * half_range[j] with
 * half_range = 0.5 * (high - low)  (low, half_range: DEVICE [A]; processed: DEVICE [N, A]).                      */
int rlx_sac_act_processed_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, const float* obs /*[N,O]*/,
                              uint32_t key_io[2], int scheme, float* action /*[N,A]*/, int N, float log_std_min,
                              float log_std_max, int deterministic, int row_offset, int N_global, const float* low,
                              const float* half_range, float* processed, void* stream);
/* the whole jitted `update` (sac.py:128-215): per-sample noise keys split(key, 2B+1), loss_fn, three
 * plain Adam steps, Polyak.  opt_count_io (HOST) = optimizer steps so far, advanced by one.
 * metrics_out: DEVICE float[10] = {q_loss, policy_loss, entropy_loss, entropy, alpha, q_value,
 * policy_grad_norm, critic_grad_norm, entropy_grad_norm, 0}.
 * With the ring source (hp->ring_states != NULL) the five batch arguments are OUTPUTS (the gathered transitions); states and
 * next_states may then BOTH be NULL -- "I do not want the sampled observation rows back" (12 of the gather's 44 MB at configs[3])
 * -- provided obs_dim > 32 (narrow observations are read by the policy from these very arrays: RLX_EINVAL).  actions, rewards,
 * terminations and every other output are bit-identical with and without them (tests/test_gpu_sac.py).                */
int rlx_sac_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
                       const rlx_mlp_desc* qdesc, float* qparams /*[2*nq]*/, float* qm, float* qv, float* qtarget,
                       float* log_alpha /*dev [1]*/, float* am, float* av, const float* states, const float* next_states,
                       const float* actions, const float* rewards, const float* terminations, int64_t B,
                       uint32_t key_io[2], int scheme, int64_t* opt_count_io, const rlx_sac_hparams* hp,
                       float* metrics_out, void* stream);

/* ---- FastSAC's observation normaliser (rl_x/algorithms/fastsac/pytorch/observation_normalizer.py:11-53) ----------------
 * State on the DEVICE: running_mean, running_var, running_std_dev fp32 [O] (initially 0, 1, 1) and count int64[1] (0).
 * update: batch mean / population variance of obs [B, O] merged into the running statistics with the reference's formula
 * (its squared-difference term is taken against the already updated mean, :44-49), running_std_dev = sqrt(running_var),
 * count += B; fp64 column sums in a fixed order (bit-reproducible).  On a data-parallel context (communicator or all-reduce
 * hook) the sums and the row count are all-reduced first: every rank merges the GLOBAL batch, the statistics stay replicated.
 * apply:  out = (obs - running_mean) / (running_std_dev + epsilon)   (epsilon 1e-8 in the reference; out may alias obs).
 * The plugin calls them where FastSAC does (fastsac.py:253-254 acting / evaluation without update, :288-289 the sampled states
 * and next states with update), behind sac.hip's flag enable_observation_normalization.                                 */
int rlx_obs_norm_update_f32(rlx_ctx*, const float* obs, int64_t B, int O, float* running_mean, float* running_var,
                            float* running_std_dev, int64_t* count, void* stream);
int rlx_obs_norm_apply_f32(rlx_ctx*, const float* obs, int64_t B, int O, const float* running_mean,
                           const float* running_std_dev, float epsilon, float* out, void* stream);

/* ---- FastSAC's distributional critic step (rl_x/algorithms/fastsac/pytorch/fastsac.py:144-213) --------------------------
 * From the four networks' logits [B, nr_atoms] (online critics on (s, a), target critics on (s', a')) and the transition:
 * categorical projection of the entropy-adjusted n-step target onto the support linspace(v_min, v_max, nr_atoms) (the
 * reference's two index_add_ passes in their sequential order: deterministic), the clipped-double-Q choice of the projection
 * with the smaller expectation (or each critic's own), q_loss = q1_loss + q2_loss with q_k_loss = -mean_b sum_j target_kj
 * log_softmax(q_k)_j, and d q_loss / d logits of both online critics (what their backward passes start from).
 * rewards, dones, truncations, effective_n_steps, next_log_probs: DEVICE float[B]; log_alpha: DEVICE float[1] (alpha = exp);
 * out4: DEVICE float[4] = {q_loss, q_min, q_max, 0} (extrema of the first projection's expectation, fastsac.py:212-213).      */
int rlx_c51_critic_loss_f32(rlx_ctx*, const float* q1_logits, const float* q2_logits, const float* q1_next_logits,
                            const float* q2_next_logits, const float* rewards, const float* dones, const float* truncations,
                            const float* effective_n_steps, const float* next_log_probs, const float* log_alpha, int64_t B,
                            int nr_atoms, float gamma, float v_min, float v_max, int clipped_double_q, float* d_q1_logits,
                            float* d_q2_logits, float* out4, void* stream);

/* ---- FastSAC: networks and update steps (rl_x/algorithms/fastsac/pytorch) ------------------------------------------------
 * rlx_lnmlp_desc: every hidden layer is Dense -> LayerNorm (torch.nn.LayerNorm: population variance, eps 1e-5) -> SiLU, then a
 * Dense head (policy.py:46-57 with a [mean | log_std] head of width 2 * act_dim; q_network.py:27-38 with nr_atoms outputs).
 * FLAT LAYOUT: per hidden layer W[in, out] row-major, b[out], ln_scale[out], ln_bias[out]; then head W[in, out_dim], b[out_dim].
 * Hidden widths: multiples of 64, at most 768.                                                                                */
typedef struct rlx_lnmlp_desc {
  int32_t in_dim;
  int32_t n_hidden; /* 1..4 */
  int32_t hidden[4];
  int32_t out_dim;
} rlx_lnmlp_desc;
int64_t rlx_lnmlp_param_count(const rlx_lnmlp_desc*);
/* head output [M, out_dim] of x [M, in_dim] (row stride ldx >= in_dim)                                                      */
int rlx_lnmlp_fwd_f32(rlx_ctx*, const rlx_lnmlp_desc*, const float* params, const float* x, int ldx, float* out, int64_t M,
                      void* stream);

typedef struct rlx_fastsac_hparams { /* fastsac/pytorch/default_config.py:12-33 */
  float gamma, tau, v_min, v_max, log_std_min, log_std_max, target_entropy;
  float lr_policy, lr_critic, lr_alpha, weight_decay, adam_b1, adam_b2, adam_eps; /* torch.optim.AdamW (fastsac.py:88-91) */
  float max_grad_norm;       /* -1 (the reference's default): none; else torch.nn.utils.clip_grad_norm_ on the critics' / the policy's
                              * gradients before their AdamW steps: g *= min(1, c / (norm + 1e-6)) (fastsac.py:129-130, :218-219);
                              * the reported gradient norm is the un-clipped one, as clip_grad_norm_ returns it              */
  int32_t nr_atoms;          /* 2..128 */
  int32_t clipped_double_q;  /* clipped_double_q_learning */
} rlx_fastsac_hparams;

/* ReplayBuffer.sample (fastsac/pytorch/replay_buffer.py:34-96) for GIVEN start rows idx_t and env columns idx_e (DEVICE int32
 * [B]; the reference draws them with torch.randint over [0, max_start) x [0, nr_envs), max_start = capacity once the ring is
 * full, else max(1, size - n_steps + 1); n_steps == 1: [0, size)).  Ring arrays: DEVICE [capacity, nr_envs, .], pos / size as the
 * reference's add() leaves them.  Outputs [B, .]: state and action of the start row, the n-step discounted reward up to the first
 * done, next state / done / truncation of the step the window ends on, and the number of steps that counted.                    */
int rlx_fastsac_replay_sample_f32(rlx_ctx*, const float* ring_states, const float* ring_next_states, const float* ring_actions,
                                  const float* ring_rewards, const float* ring_dones, const float* ring_truncations, int capacity,
                                  int nr_envs, int obs_dim, int act_dim, int n_steps, float gamma, int pos, int size,
                                  const int32_t* idx_t, const int32_t* idx_e, int64_t B, float* states, float* next_states,
                                  float* actions, float* rewards, float* dones, float* truncations, float* effective_n_steps,
                                  void* stream);
/* policy.get_action (policy.py:93-108): action [N, A] = tanh(mean + exp(log_std) eps) * action_scale, or tanh(mean) *
 * action_scale when deterministic; log_std = min + 0.5 (max - min) (tanh(raw) + 1) (policy.py:66-72).  obs: already normalised /
 * column-selected policy observations [N, pdesc->in_dim].  key, subkey = split(key); eps[n, j] = normal(bits(subkey, (n +
 * row_offset) * A + j of N_global * A)) -- the reference draws with torch's CUDA generator, which nothing else reproduces;
 * rlx_dbg_set_sac_noise(eps_next, .) injects a given noise.                                                                  */
int rlx_fastsac_act_f32(rlx_ctx*, const rlx_lnmlp_desc* pdesc, const float* pparams, const float* obs, const float* action_scale,
                        uint32_t key_io[2], int scheme, float* action, int N, int deterministic, int row_offset, int N_global,
                        const rlx_fastsac_hparams* hp, void* stream);
/* ONE critic_and_entropy_loss_fn call plus the Polyak update that follows it (fastsac.py:144-241, :323-327): next action and
 * log-prob from the policy (no gradient), target critics on (s', a'), categorical projection of the entropy-adjusted n-step
 * target (rlx_c51_critic_loss_f32), both online critics' backward, AdamW step of the 2 * nq critic parameters (one optimizer
 * state, as in the reference), entropy-coefficient loss and its AdamW step, target <- (1 - tau) target + tau params.
 * qparams / qm / qv / qtarget: the two critics back to back.  critic_states / critic_next_states: NULL, or the critics' own
 * observation columns [B, qdesc->in_dim - act_dim].  dones / truncations / effective_n_steps: as ReplayBuffer.sample returns
 * them (replay_buffer.py:34-96).  opt_count_io (HOST): optimizer steps of the critic / entropy optimizers so far, advanced by 1.
 * metrics_out: DEVICE float[8] = {q_loss, entropy_loss, q_min, q_max, entropy, critic_grad_norm, entropy_grad_norm (the
 * reference logs norm^2, fastsac.py:237), alpha before the step}.                                                           */
int rlx_fastsac_critic_update_f32(rlx_ctx*, const rlx_lnmlp_desc* pdesc, const float* pparams, const rlx_lnmlp_desc* qdesc,
                                  float* qparams, float* qm, float* qv, float* qtarget, float* log_alpha, float* am, float* av,
                                  const float* states, const float* next_states, const float* critic_states,
                                  const float* critic_next_states, const float* actions, const float* rewards, const float* dones,
                                  const float* truncations, const float* effective_n_steps, const float* action_scale, int64_t B,
                                  uint32_t key_io[2], int scheme, int64_t* opt_count_io, const rlx_fastsac_hparams* hp,
                                  float* metrics_out, void* stream);
/* ONE policy_loss_fn call (fastsac.py:106-141): loss = mean(alpha log_prob - q), q = (q1 + q2) / 2 or min(q1, q2) of the
 * critics' EXPECTED values sum_j softmax(logits)_j z_j; gradient through both critics to the action and on through the squashing
 * to the policy; AdamW step of the policy.  metrics_out: DEVICE float[3] = {policy_loss, alpha, policy_grad_norm}.           */
int rlx_fastsac_policy_update_f32(rlx_ctx*, const rlx_lnmlp_desc* pdesc, float* pparams, float* pm, float* pv,
                                  const rlx_lnmlp_desc* qdesc, const float* qparams, const float* log_alpha, const float* states,
                                  const float* critic_states, const float* action_scale, int64_t B, uint32_t key_io[2], int scheme,
                                  int64_t* opt_count_io, const rlx_fastsac_hparams* hp, float* metrics_out, void* stream);

/* ---- FastTD3: networks and update steps (rl_x/algorithms/fasttd3/pytorch) ------------------------------------------------
 * Networks: rlx_mlp_desc with act = RLX_ACT_RELU, ln_first = 0, has_logstd = 0 -- Dense -> ReLU per hidden layer, then a Dense
 * head (policy.py:38-47: 512-256-128, head act_dim wide, tanh applied by the entry points below; q_network.py:28-36: input
 * [critic obs | action], 1024-512-256, head nr_atoms wide).  FLAT LAYOUT: per hidden layer W[in, out] row-major, b[out]; then
 * head W[in, out_dim], b[out_dim] (rlx_mlp_param_count).  FastTD3's own check: 1..3 hidden layers, widths multiples of 64 up to
 * 1024, act_dim <= 64.  Sampling: rlx_fastsac_replay_sample_f32 (the same ring, fasttd3/pytorch/replay_buffer.py); normaliser:
 * rlx_obs_norm_* (observation_normalizer.py).  Noise: threefry, key, subkey = split(key) per call; rlx_dbg_set_sac_noise(eps_next,
 * .) injects the N(0, 1) draws of the exploration noise (act, [N, A]) and of the smoothing noise (critic update, [B, A]).        */
typedef struct rlx_fasttd3_hparams { /* fasttd3/pytorch/default_config.py:12-38 */
  float gamma, tau, v_min, v_max;
  float lr_policy, lr_critic, weight_decay, adam_b1, adam_b2, adam_eps; /* torch.optim.AdamW, default betas (fasttd3.py:88-89) */
  float max_grad_norm;        /* -1: none; else torch.nn.utils.clip_grad_norm_ before each AdamW step (fasttd3.py:125-126, :214-215);
                               * the reported gradient norm is the un-clipped one                                                */
  float smoothing_epsilon;    /* target-policy smoothing: noise = clamp(randn * smoothing_epsilon, +-smoothing_clip_value) */
  float smoothing_clip_value; /* (fasttd3.py:143-144)                                                                     */
  int32_t nr_atoms;           /* 2..128 */
  int32_t clipped_double_q;   /* clipped_double_q_learning */
} rlx_fasttd3_hparams;

/* noise_scales[N] = U[0, 1) (noise_std_max - noise_std_min) + noise_std_min (fasttd3.py:241 at reset; :274-278 after a step:
 * only where dones[i] > 0).  dones: NULL (every env) or DEVICE float[N].  key, subkey = split(key); u_i = bits(subkey, i of N).  */
int rlx_fasttd3_noise_scales_f32(rlx_ctx*, uint32_t key_io[2], int scheme, float* noise_scales, const float* dones, int N,
                                 float noise_std_min, float noise_std_max, void* stream);
/* Policy.get_action (policy.py:57-66): action[N, A] = tanh(policy(obs)) + eps * noise_scales[n] (what the ring stores, unclipped);
 * processed_action = clip_and_rescale ? low + 0.5 (clamp(action, -1, 1) + 1)(high - low) : action (what the env gets; low / high:
 * DEVICE float[A]).  deterministic: no noise, key untouched (evaluation, test()).  obs: normalised, column-selected policy
 * observations [N, pdesc->in_dim].  eps[n, j] = normal(bits(subkey, (n + row_offset) * A + j of N_global * A)).                 */
int rlx_fasttd3_act_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, const float* obs, const float* noise_scales,
                        uint32_t key_io[2], int scheme, float* action, float* processed_action, int N, int deterministic,
                        int clip_and_rescale, const float* low, const float* high, int row_offset, int N_global, void* stream);
/* ONE critic_loss_fn call plus the Polyak update that follows it (fasttd3.py:140-225, :316-320): next action = clamp(tanh(policy(s'))
 * + clamp(eps * smoothing_epsilon, +-smoothing_clip_value), -1, 1) (no gradient, no target policy), target critics on (s', a'),
 * categorical projection of the n-step target without an entropy term (rlx_c51_critic_loss_f32 with alpha = 0), both online
 * critics' backward, ONE AdamW step over the 2 * nq critic parameters, target <- (1 - tau) target + tau params.
 * qparams / qm / qv / qtarget: the two critics back to back.  states / next_states: policy columns [B, pdesc->in_dim];
 * critic_states / critic_next_states: NULL, or the critics' own columns [B, qdesc->in_dim - act_dim].  opt_count_io (HOST): critic
 * optimizer steps so far, advanced by 1.  metrics_out: DEVICE float[4] = {q_loss, q_min, q_max (of q1's projected expectation,
 * fasttd3.py:208-209), critic_grad_norm}.                                                                                      */
int rlx_fasttd3_critic_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, const rlx_mlp_desc* qdesc, float* qparams,
                                  float* qm, float* qv, float* qtarget, const float* states, const float* next_states,
                                  const float* critic_states, const float* critic_next_states, const float* actions,
                                  const float* rewards, const float* dones, const float* truncations, const float* effective_n_steps,
                                  int64_t B, uint32_t key_io[2], int scheme, int64_t* opt_count_io, const rlx_fasttd3_hparams* hp,
                                  float* metrics_out, void* stream);
/* ONE policy_loss_fn call (fasttd3.py:105-136): loss = -mean(q), q = min(q1, q2) (torch.minimum: a tie splits the gradient 1/2 each)
 * or (q1 + q2) / 2 of the critics' EXPECTED values sum_j softmax(logits)_j z_j on (s, tanh(policy(s))); gradient through both
 * critics to the action, through the tanh to the policy; AdamW step of the policy.  metrics_out: DEVICE float[2] =
 * {policy_loss, policy_grad_norm}.                                                                                             */
int rlx_fasttd3_policy_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, const rlx_mlp_desc* qdesc,
                                  const float* qparams, const float* states, const float* critic_states, int64_t B,
                                  int64_t* opt_count_io, const rlx_fasttd3_hparams* hp, float* metrics_out, void* stream);

/* ---- TQC: truncated quantile critics (rl_x/algorithms/tqc/flax) ------------------------------------------------------------
 * SAC's host-loop flavour (sac/flax/sac.py) with another critic: tqc/flax/policy.py and replay_buffer.py are sac/flax's files, so
 * acting and sampling are rlx_sac_act_processed_f32 and rlx_sac_replay_sample_f32.  Networks: rlx_mlp_desc with act =
 * RLX_ACT_RELU, ln_first = 0, has_logstd = 0 (policy.py:22-41: out_dim = 2 * act_dim, head columns [0, A) mean, [A, 2A) raw
 * log_std; critic.py:17-55: ensemble_size independent networks on [critic obs | action], each nr_atoms_per_net outputs, BACK TO
 * BACK in one flat vector like rlx_sac_update_f32's two).  FLAT LAYOUT of a network: FastTD3's (above).  Envelope: 1..3 hidden
 * layers, widths multiples of 64 up to 1024, act_dim <= 64, 1 <= ensemble_size <= 8, nr_atoms_per_net >= 1, total atoms T =
 * ensemble_size * nr_atoms_per_net <= 128, 0 <= nr_dropped_atoms_per_net < nr_atoms_per_net, huber_kappa > 0, B > 0; a descriptor
 * or size outside it is RLX_EUNSUP, every other bad argument RLX_EINVAL, rlx_last_error() names the argument.
 * Flat atom index i = e * nr_atoms_per_net + n (q_atoms.reshape(nr_total_atoms), tqc.py:162); K = T - ensemble_size *
 * nr_dropped_atoms_per_net target atoms (tqc.py:61).  Atoms that are NaN are outside the contract (the sort drops them).        */
typedef struct rlx_tqc_hparams {              /* tqc/flax/default_config.py:9-28 */
  float gamma, tau, target_entropy, log_std_min, log_std_max;
  float lr_policy, lr_critic, lr_alpha;       /* host evaluates the schedule (tqc.py:85-93) */
  float adam_b1, adam_b2, adam_eps;           /* optax.adam defaults 0.9, 0.999, 1e-8 (tqc.py:101,108,114) */
  float huber_kappa;                          /* tqc.py:169-170 */
  int32_t ensemble_size, nr_atoms_per_net, nr_dropped_atoms_per_net;   /* tqc.py:51-53, :60-61 */
  const float *critic_states, *critic_next_states;   /* as in rlx_sac_hparams: the critics' own observation columns
                                                      * (critic.py:11,23) of s / s', or NULL both (the policy's) */
} rlx_tqc_hparams;

/* the critic loss on given atoms (tqc.py:155-170), like rlx_c51_critic_loss_f32: q_atoms, next_atoms DEVICE [E, B, N]
 * (critic-major, as E head GEMMs leave them); y[b, k] = r_b + gamma (1 - term_b) (sorted pooled next atoms[k] - exp(log_alpha)
 * next_logp_b), k < K (tqc.py:156-158: the POOLED T atoms are sorted, not each network's); loss = mean over b, i, k of
 * |tau_i - [y_k < q_i]| huber_kappa(y_k - q_i) / kappa, tau_i = (i + 0.5) / T (tqc.py:164-170); dq_out [E, B, N] = d loss / d q_atoms;
 * loss_out DEVICE [1]; y_out NULL or DEVICE [B, K] */
int rlx_tqc_quantile_loss_f32(rlx_ctx*, const float* q_atoms, const float* next_atoms, const float* rewards,
                              const float* terminations, const float* next_logp, const float* log_alpha, int64_t B,
                              const rlx_tqc_hparams* hp, float* dq_out, float* loss_out, float* y_out, void* stream);

/* the whole jitted `update` (tqc.py:134-230): loss_fn meaned over the batch (:139-209), per-sample keys keys = split(key, 2B+1),
 * key = keys[0], next-state noise keys[1::2], current-state noise keys[2::2] (:211-212; rlx_dbg_set_sac_noise(eps_next, eps_cur)
 * injects the N(0, 1) draws [B, A] instead), three plain optax.adam steps without clipping (:218-220), Polyak of all critics
 * (:223).  qparams / qm / qv / qtarget: [E * nq], the E critics back to back.  states / next_states: the policy's columns
 * [B, pdesc->in_dim].  One call, no host synchronisation.  opt_count_io (HOST): optimizer steps so far, advanced by 1.
 * metrics_out DEVICE float[10] in rlx_sac_update_f32's order (q_value = mean over all atoms, tqc.py:183; [9] = 0) */
int rlx_tqc_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
                       const rlx_mlp_desc* qdesc, float* qparams /*[E*nq]*/, float* qm, float* qv, float* qtarget,
                       float* log_alpha, float* am, float* av, const float* states, const float* next_states,
                       const float* actions, const float* rewards, const float* terminations, int64_t B,
                       uint32_t key_io[2], int scheme, int64_t* opt_count_io, const rlx_tqc_hparams* hp,
                       float* metrics_out, void* stream);

/* ---- REDQ: randomized ensembled double Q-learning (rl_x/algorithms/redq/flax) -------------------------------------------------
 * SAC's policy, entropy coefficient, acting and replay ring (redq/flax/policy.py is sac/flax's) with ensemble_size scalar critics
 * (critic.py:17-53: Dense(H) -> ReLU -> Dense(H) -> ReLU -> Dense(1), BACK TO BACK in one flat vector like rlx_tqc_update_f32's) and
 * a high update-to-data `update` (redq.py:144-261): G = q_update_steps critic steps on G fresh batches, each followed by plain
 * Adam of all critics and Polyak (:228-242), then ONE policy / entropy step on batch 0 with the critics from after the loop
 * (:246-253).  Networks: rlx_mlp_desc with act = RLX_ACT_RELU, ln_first = 0, has_logstd = 0; FLAT LAYOUT of a network: FastTD3's
 * (above).  Q values are laid out [E, B], critic-major.  Envelope: 1..3 hidden layers, widths multiples of 64 up to 1024, act_dim
 * <= 64, qdesc->out_dim = 1, 1 <= ensemble_size <= 16, 1 <= in_target_minimization_size <= ensemble_size, 1 <= q_update_steps <=
 * 64, B > 0; a descriptor or size outside it is RLX_EUNSUP, every other bad argument RLX_EINVAL, rlx_last_error() names it.     */
typedef struct rlx_redq_hparams {              /* redq/flax/default_config.py:9-27 */
  float gamma, tau, target_entropy, log_std_min, log_std_max;
  float lr_policy, lr_critic, lr_critic_delta, lr_alpha;   /* host evaluates the schedules (redq.py:82-98); critic step i of the
                                                            * call runs at lr_critic + i * lr_critic_delta: q_linear_schedule is
                                                            * linear in the critic step count (:82-86) */
  float adam_b1, adam_b2, adam_eps;            /* optax.adam defaults 0.9, 0.999, 1e-8 (redq.py:110,117,123) */
  int32_t ensemble_size, in_target_minimization_size, q_update_steps;   /* redq.py:51-53 */
  const float *critic_states, *critic_next_states;   /* [G, B, Oc]: the critics' own observation columns (critic.py:11,23) of
                                                      * s / s', or NULL both (the policy's) */
} rlx_redq_hparams;

/* host only, no context: the target subset REDQ draws from sample_key (redq.py:232-233): jax.random.choice(sample_key, arange(E),
 * (M,), replace=False) = permutation(sample_key, E)[:M], i.e. ceil(3 ln E / ln(2^32 - 1)) rounds of {key, sub = split(key); stable
 * sort by random_bits(sub, (E,))}: one round for 2 <= E <= 16, none (the identity) for E = 1.  1 <= M <= E <= 16. */
int rlx_redq_subset_host(const uint32_t sample_key[2], int E, int M, int scheme, int32_t* idx_out /*[M]*/);

/* the two loss heads on given values; any output may be NULL except the one its inputs serve (dq_out; seed_out when qa is given).
 * Critic (redq.py:163-169, meaned over batch and ensemble, :219): y_out [B] = r + gamma (1 - term) (min over the M rows of
 * q_next_sel - exp(log_alpha) next_logp); dq_out [E, B] = 2 (q - y) / (B E); loss_out DEVICE [1] = mean (q - y)^2.
 * Policy (redq.py:195-198), qa != NULL: minq_out [B] = min over ALL E rows of qa; seed_out [E, B] = d mean(-min) / d qa =
 * -[qa == min] / (B n_ties): jnp.min's gradient, split evenly among exact ties. */
int rlx_redq_losses_f32(rlx_ctx*, const float* q /*[E,B]*/, const float* q_next_sel /*[M,B]*/, const float* rewards,
                        const float* terminations, const float* next_logp, const float* log_alpha, const float* qa /*[E,B] or NULL*/,
                        int64_t B, const rlx_redq_hparams* hp, float* y_out, float* dq_out, float* loss_out,
                        float* seed_out /*[E,B]*/, float* minq_out /*[B]*/, void* stream);

/* the whole jitted `update` (redq.py:144-261) in one call on one stream, no host synchronisation.  Critic step i: keys =
 * split(key, B + 2), key = keys[0], sample_key = keys[1] (the step's target subset), row b's next-action noise from keys[2 + b]
 * (:229-236); policy step: keys = split(key, B + 1), key = keys[0], row b's noise from keys[1 + b] (:247-250).
 * rlx_dbg_set_sac_noise(eps_next, eps_cur) injects the N(0, 1) draws instead: eps_next [G, B, A], eps_cur [B, A].
 * states / next_states [G, B, pdesc->in_dim], actions [G, B, A], rewards / terminations [G, B]; the policy step reads batch 0.
 * qparams / qm / qv / qtarget: [E * nq].  q_opt_count_io / pi_opt_count_io (HOST): the two optax counters (:107-124), advanced by
 * G and by 1; critic step i is Adam step q_count + i + 1.  metrics_out DEVICE float[10] in rlx_sac_update_f32's order: [0] q_loss
 * and [7] critic_grad_norm are the means over the G steps (:244), [5] q_value the mean of the min over all E critics, [9] = 0.
 * subsets_out: NULL or HOST int32 [G, M], the target networks each step selected.  Nothing is written when a check fails. */
int rlx_redq_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
                        const rlx_mlp_desc* qdesc, float* qparams /*[E*nq]*/, float* qm, float* qv, float* qtarget,
                        float* log_alpha, float* am, float* av, const float* states /*[G,B,O]*/, const float* next_states,
                        const float* actions, const float* rewards /*[G,B]*/, const float* terminations, int64_t B,
                        uint32_t key_io[2], int scheme, int64_t* q_opt_count_io /* += G */, int64_t* pi_opt_count_io /* += 1 */,
                        const rlx_redq_hparams* hp, float* metrics_out /*DEVICE [10]*/, int32_t* subsets_out /*HOST [G,M] or NULL*/,
                        void* stream);

/* ---- AQE: truncated-mean multi-head ensemble critics (rl_x/algorithms/aqe/flax) -------------------------------------------------
 * REDQ's high update-to-data `update` (aqe.py:145-259: G = q_update_steps critic steps on G fresh batches, each followed by plain
 * Adam of all critics and Polyak, :230-240; then ONE policy / entropy step on batch 0 with the critics from after the loop,
 * :245-251) over ensemble_size critics with nr_heads_per_net outputs each (critic.py: Dense(H) -> ReLU -> Dense(H) -> ReLU ->
 * Dense(nr_heads_per_net), BACK TO BACK in one flat vector like rlx_tqc_update_f32's).  Networks: rlx_mlp_desc with act =
 * RLX_ACT_RELU, ln_first = 0, has_logstd = 0; FLAT LAYOUT of a network: FastTD3's (above).  Q values are laid out [E, B, H],
 * critic-major; flat index i = e * nr_heads_per_net + h (reshape(nr_total_q_values), aqe.py:165); T = E * H values per transition,
 * K = T - nr_dropped_q_values of them kept in the target (aqe.py:58-59: dropped from the POOL, not per net).  Envelope: 1..3 hidden
 * layers, widths multiples of 64 up to 1024, act_dim <= 64, qdesc->out_dim = nr_heads_per_net >= 1, 1 <= ensemble_size <= 16, T <=
 * 128, 0 <= nr_dropped_q_values < T, 1 <= q_update_steps <= 64, B > 0; a descriptor or size outside it is RLX_EUNSUP, every other
 * bad argument RLX_EINVAL, rlx_last_error() names it.  Q values that are NaN are outside the contract (the sort drops them).       */
typedef struct rlx_aqe_hparams {               /* aqe/flax/default_config.py:9-28 */
  float gamma, tau, target_entropy, log_std_min, log_std_max;
  float lr_policy, lr_critic, lr_critic_delta, lr_alpha;   /* host evaluates the schedules (aqe.py:83-99); critic step i of the call
                                                            * runs at lr_critic + i * lr_critic_delta (q_linear_schedule, :83-87) */
  float adam_b1, adam_b2, adam_eps;            /* optax.adam defaults 0.9, 0.999, 1e-8 (aqe.py:111,118,124) */
  int32_t ensemble_size, nr_heads_per_net, nr_dropped_q_values, q_update_steps;   /* aqe.py:51-52, :58-59 */
  const float *critic_states, *critic_next_states;   /* [G, B, Oc]: the critics' own observation columns of s / s', or NULL both
                                                      * (the policy's) */
} rlx_aqe_hparams;

/* the two loss heads on given values; any output may be NULL except the one its inputs serve (dq_out; seed_out when qa is given).
 * Critic (aqe.py:164-171, meaned over the batch, :221): y_out [B] = r + gamma (1 - term) (mean of the K lowest of the row's T
 * POOLED values of q_next - exp(log_alpha) next_logp); dq_out [E, B, H] = 2 (q - y) / (B T); loss_out DEVICE [1] = mean (q - y)^2.
 * Policy (aqe.py:197-200), qa != NULL: meanq_out [B] = the row's mean over all T values of qa; seed_out [E, B, H] =
 * d mean(-mean_q) / d qa = -1 / (B T). */
int rlx_aqe_losses_f32(rlx_ctx*, const float* q /*[E,B,H]*/, const float* q_next /*[E,B,H]*/, const float* rewards,
                       const float* terminations, const float* next_logp, const float* log_alpha, const float* qa /*[E,B,H] or NULL*/,
                       int64_t B, const rlx_aqe_hparams* hp, float* y_out, float* dq_out, float* loss_out,
                       float* seed_out /*[E,B,H]*/, float* meanq_out /*[B]*/, void* stream);

/* the whole jitted `update` (aqe.py:145-259) in one call on one stream, no host synchronisation.  Every step, critic or policy:
 * keys = split(key, B + 1), key = keys[0], row b's noise from keys[1 + b] (:231-232, :245-246).
 * rlx_dbg_set_sac_noise(eps_next, eps_cur) injects the N(0, 1) draws instead: eps_next [G, B, A], eps_cur [B, A].
 * states / next_states [G, B, pdesc->in_dim], actions [G, B, A], rewards / terminations [G, B]; the policy step reads batch 0.
 * qparams / qm / qv / qtarget: [E * nq].  q_opt_count_io / pi_opt_count_io (HOST): the two optax counters (:108-125), advanced by
 * G and by 1; critic step i is Adam step q_count + i + 1.  metrics_out DEVICE float[10] in rlx_sac_update_f32's order: [0] q_loss
 * and [7] critic_grad_norm are the means over the G steps (:242), [5] q_value the mean over batch and all T heads, [9] = 0.
 * Nothing is written when a check fails. */
int rlx_aqe_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
                       const rlx_mlp_desc* qdesc, float* qparams /*[E*nq]*/, float* qm, float* qv, float* qtarget,
                       float* log_alpha, float* am, float* av, const float* states /*[G,B,O]*/, const float* next_states,
                       const float* actions, const float* rewards /*[G,B]*/, const float* terminations, int64_t B,
                       uint32_t key_io[2], int scheme, int64_t* q_opt_count_io /* += G */, int64_t* pi_opt_count_io /* += 1 */,
                       const rlx_aqe_hparams* hp, float* metrics_out /*DEVICE [10]*/, void* stream);

/* ---- DroQ: dropout Q-functions (rl_x/algorithms/droq/flax) -----------------------------------------------------------------------
 * REDQ's `update` (droq.py:144-261 is redq.py:144-261 plus dropout keys) over ensemble_size critics -- two by default -- whose EVERY
 * hidden block is Dense -> Dropout -> LayerNorm -> ReLU (droq/flax/critic.py:25-35; flax's LayerNorm: eps 1e-6, scale and bias).
 * THE CRITIC OF THIS ENTRY POINT IS LayerNorm-IN-EVERY-HIDDEN-BLOCK: qdesc is a rlx_mlp_desc under REDQ's descriptor rules (act =
 * RLX_ACT_RELU, ln_first = 0, has_logstd = 0, out_dim = 1), and the FLAT LAYOUT of one critic is per hidden block W[in, out], b[out],
 * LN scale[out], LN bias[out], then the head W[in, 1], b[1]; E critics BACK TO BACK.  Dropout has no parameters.  The policy is
 * REDQ's.  Dropout is active in every critic pass (critic.py:28, :32: deterministic=False): the online critics', the selected
 * targets' and the policy step's, input-gradient passes included.
 * THE MASK STREAM IS THE LIBRARY'S OWN (flax's make_rng folds hashed module paths into the dropout key, which cannot be restated):
 * for row b, the j-th network evaluated in a pass (from 0; a target pass of M networks uses j = 0 .. M - 1), hidden layer l of L,
 * unit u of D:  row_key = split(step_key, count)[base + stride b];  net_key = split(row_key, E)[j] (nn.vmap splits the dropout rng
 * over axis_size = ensemble_size, critic.py:50-57);  layer_key = split(net_key, L)[l];  kept iff uniform(layer_key, (D,))[u] < keep,
 * keep = 1 - dropout_rate in float32 (jax.random.bernoulli); kept units are divided by keep, the others are 0.
 * Envelope: REDQ's, with the critics' hidden widths multiples of 64 up to 768, 0 <= dropout_rate < 1, 3 B + 2 <= 2^31 - 1; a
 * descriptor or size outside it is RLX_EUNSUP, every other bad argument RLX_EINVAL, rlx_last_error() names it.                     */
typedef struct rlx_droq_hparams {              /* droq/flax/default_config.py:9-28: rlx_redq_hparams, then dropout_rate */
  float gamma, tau, target_entropy, log_std_min, log_std_max;
  float lr_policy, lr_critic, lr_critic_delta, lr_alpha;   /* as rlx_redq_hparams (droq.py:82-98) */
  float adam_b1, adam_b2, adam_eps;
  int32_t ensemble_size, in_target_minimization_size, q_update_steps;   /* droq.py:51-53; defaults 2, 2, 20 */
  const float *critic_states, *critic_next_states;   /* [G, B, Oc] or NULL both */
  float dropout_rate;                          /* default_config.py:20 (0.01); 0: no draws, a plain LayerNorm + ReLU block */
} rlx_droq_hparams;

/* test entry point: DEVICE flags_out [B, D] = 1 where the unit is kept, of the mask stream above for one (key layout, j, E, l, L, D,
 * rate); key: the step key (HOST).  D a multiple of 64 up to 768; base + stride (B - 1) < count <= 2^31 - 1. */
int rlx_droq_mask_u8(rlx_ctx*, const uint32_t key[2], int scheme, uint32_t base, uint32_t stride, uint32_t count, int j, int E, int l,
                     int L, int64_t B, int D, float rate, uint8_t* flags_out, void* stream);

/* test entry point: the fused Dropout -> LayerNorm -> ReLU block (critic.py:28-30, :32-34) on given values.  Z [M, D]: the Dense
 * output, never written.  scale_bias [2 D]: LN scale then LN bias.  backward == 0: H_io [M, D] = relu(LN(mask Z / keep) scale + bias).
 * backward != 0: H_io holds d L / d H and receives d L / d Z = (mask / keep) LNbwd(dH relu'), the mask regenerated from the keys;
 * dg_out / db_out DEVICE [D]: the summed scale / bias gradients.  Keys and sizes as rlx_droq_mask_u8; rate 0 makes no draws. */
int rlx_droq_block_f32(rlx_ctx*, const float* Z, float* H_io, const float* scale_bias, const uint32_t key[2], int scheme, uint32_t base,
                       uint32_t stride, uint32_t count, int j, int E, int l, int L, int64_t M, int D, float rate, int backward,
                       float* dg_out, float* db_out, void* stream);

/* the whole jitted `update` (droq.py:144-261) in one call on one stream, no host synchronisation: rlx_redq_update_f32's arguments,
 * schedule and metrics.  Critic step i: keys = split(key, 3 B + 2), key = keys[0], sample_key = keys[1] (the step's target subset,
 * rlx_redq_subset_host's rule); row b's next-action noise from keys[2 + 3 b], the online critics' dropout from keys[3 + 3 b], the
 * selected targets' from keys[4 + 3 b] (:229-236).  Policy step: keys = split(key, 2 B + 1), key = keys[0], row b's noise from
 * keys[1 + 2 b], the E critics' dropout on (s_0, a~) from keys[2 + 2 b] (:247-250).  rlx_dbg_set_sac_noise keeps REDQ's meaning (the
 * N(0, 1) draws only; the masks always come from the keys).  Adam and Polyak run over the whole flat critic vector, LayerNorm
 * parameters included.  Nothing is written when a check fails. */
int rlx_droq_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
                        const rlx_mlp_desc* qdesc, float* qparams /*[E*nq]*/, float* qm, float* qv, float* qtarget,
                        float* log_alpha, float* am, float* av, const float* states /*[G,B,O]*/, const float* next_states,
                        const float* actions, const float* rewards /*[G,B]*/, const float* terminations, int64_t B,
                        uint32_t key_io[2], int scheme, int64_t* q_opt_count_io /* += G */, int64_t* pi_opt_count_io /* += 1 */,
                        const rlx_droq_hparams* hp, float* metrics_out /*DEVICE [10]*/, int32_t* subsets_out /*HOST [G,M] or NULL*/,
                        void* stream);

/* ---- batch renormalisation (rl_x/algorithms/crossq/flax/batch_renorm.py:77-130) ---------------------------------------------------
 * The library's column-statistics layer: it normalises x [M, D] over its M ROWS, per column, with scale g, bias b and running
 * statistics ra_mean (initially 0) / ra_var (initially 1).
 *   eval (:87-93)    y = (x - ra_mean) rsqrt(ra_var + eps) g + b; no state changes.
 *   train (:95-128)  mu = mean_i x, v = max(0, mean_i x^2 - mu^2);  r = clip(sqrt(v + eps) / sqrt(ra_var + eps), 1 / r_max, r_max),
 *                    d = clip((mu - ra_mean) / sqrt(ra_var + eps), -d_max, d_max), both constants of the backward (stop_gradient);
 *                    w = warmed;  cm = mu - w d sqrt(v) / r;  rho = rsqrt(v (w / r^2 + 1 - w) + eps);  y = (x - cm) rho g + b;
 *                    then ra_mean <- momentum ra_mean + (1 - momentum) mu, ra_var likewise with v, in place.
 * warmed is the CALLER's statement that the layer's count of earlier training passes has reached warm_up_steps (:104); the library
 * keeps no step counter.  Column sums run in double and in a fixed order: identical calls give identical bits.
 * DEVIATION, zero batch variance: where v == 0 the reference's sqrt(v) has an infinite derivative (its autodiff gives NaN there);
 * the library takes that term's gradient as 0 where w = 0 or v = 0, and every result stays finite. */
typedef struct rlx_brn_config {
  float momentum;                              /* batch_renorm_momentum (crossq default_config.py: 0.99); in [0, 1) */
  float eps, r_max, d_max;                     /* batch_renorm.py:80-83: 1e-3, 3, 5 */
  int32_t warmed;                              /* w above: 0 plain batch norm with eps, non-zero the clipped r / d correction */
} rlx_brn_config;
enum { RLX_BRN_EVAL_FWD = 0, RLX_BRN_TRAIN_FWD = 1, RLX_BRN_EVAL_BWD = 2, RLX_BRN_TRAIN_BWD = 3 };

/* test entry point: one batch-renormalisation layer alone, over E independent networks in one call (all DEVICE, float32):
 * x [E, M, ld] (never written), ld a multiple of 4 and >= D, 16-byte aligned; scale_bias [E, 2 D]: g then b; stats [E, 2 D]: ra_mean
 * then ra_var; save [E, 7 ((D + 3) & ~3)]: written by RLX_BRN_TRAIN_FWD, read by RLX_BRN_TRAIN_BWD (NULL in the eval modes).
 *   RLX_BRN_EVAL_FWD / _TRAIN_FWD  y_io [E, M, ld] receives y; the training pass advances stats in place.
 *   RLX_BRN_EVAL_BWD / _TRAIN_BWD  y_io holds d L / d y and receives d L / d x, times 1[x > 0] when relu_mask != 0 (x is a ReLU's
 *                                  output: the ReLU's derivative fused); dgb_out [E, 2 D] (or NULL) receives d g then d b.
 *                                  _TRAIN_BWD answers the _TRAIN_FWD that wrote save, on the same x; stats is not read.
 * The columns D .. ld - 1 of what y_io receives are 0.  M >= 2 (one row has no variance), D >= 1, 1 <= E <= 16 (RLX_EUNSUP above);
 * every other bad argument is RLX_EINVAL; nothing is written when a check fails. */
int rlx_brn_f32(rlx_ctx*, const float* x, int ld, int64_t M, int D, int E, const float* scale_bias, float* stats,
                const rlx_brn_config* cfg, int mode, float* y_io, float* save, int relu_mask, float* dgb_out, void* stream);

/* ---- CrossQ: batch-renormalised critics, no target networks (rl_x/algorithms/crossq/flax) ----------------------------------------
 * SAC's tanh-Gaussian policy and entropy coefficient over ensemble_size critics, every Dense of every network preceded by a batch
 * renormalisation (above): x -> BRN -> Dense -> ReLU -> BRN -> ... -> BRN -> Dense head (critic.py:25-60, policy.py:34-72).  There are
 * no target networks and no Polyak step.  Networks: rlx_mlp_desc with act = RLX_ACT_RELU, ln_first = 0, has_logstd = 0; policy
 * out_dim = 2 A (columns [0, A) the mean, [A, 2 A) the log-std, clipped to [log_std_min, log_std_max]); critics in_dim = Oc + A,
 * out_dim = 1.  FLAT LAYOUT of one network: bn0.scale[in], bn0.bias[in], W1[in, H1], b1[H1], bn1.scale[H1], bn1.bias[H1], W2, b2, ...,
 * bnL.scale[HL], bnL.bias[HL], W_head[HL, out], b_head[out] (rlx_crossq_param_count); the E critics BACK TO BACK.  RUNNING STATISTICS
 * are a vector of their own per network: bn0.mean[in], bn0.var[in], bn1.mean[H1], bn1.var[H1], ... (rlx_crossq_stats_count; initially
 * mean 0, var 1); qstats holds the E critics' back to back.
 * WARM-UP: a network's layers use the clipped r / d correction once its count of earlier training passes has reached
 * brn_warmup_steps.  A network makes one training pass per update, so the library decides from the optimiser counts it is handed:
 * critics q_opt_count >= brn_warmup_steps, policy pi_opt_count >= brn_warmup_steps (in the reference a net's `steps` equals its
 * number of updates).
 * Envelope: hidden widths multiples of 64 up to 2048, 1..3 hidden layers, A <= 64, B >= 2 (one row has zero batch variance),
 * 1 <= ensemble_size <= 16; outside it RLX_EUNSUP (widths, E > 16, and A > 64 in the two updates) or RLX_EINVAL, rlx_last_error() names
 * the argument, and nothing is written.  Passes of 4096 rows and more run their hidden-layer GEMMs on the split-operand engine, as REDQ's.
 * rlx_dbg_set_sac_noise(eps_next, eps_cur) injects the N(0, 1) block draws of the two updates ([B, A] each: eps_next the critic
 * update's, eps_cur the policy update's); acting ignores it. */
typedef struct rlx_crossq_hparams {              /* crossq/flax/default_config.py */
  float gamma, target_entropy, log_std_min, log_std_max;
  float lr_policy, lr_critic, lr_alpha;          /* learning_rate (1e-3) for all three in the reference */
  float policy_adam_b1, critic_adam_b1;          /* 0.5, 0.5 */
  float alpha_adam_b1;                           /* optax's default 0.9 (crossq.py: the entropy coefficient's plain optax.adam) */
  float adam_b2, adam_eps;                       /* 0.999, 1e-8 */
  float brn_momentum, brn_eps, brn_r_max, brn_d_max;   /* 0.99; batch_renorm.py:80-83: 1e-3, 3, 5 */
  int32_t brn_warmup_steps;                      /* batch_renorm_warmup_steps (100000) */
  int32_t ensemble_size;                         /* 2 */
  const float *critic_states, *critic_next_states;   /* [B, Oc] the critics' own observation columns, or NULL both */
} rlx_crossq_hparams;

int64_t rlx_crossq_param_count(const rlx_mlp_desc* desc);   /* floats of one network's flat parameter vector */
int64_t rlx_crossq_stats_count(const rlx_mlp_desc* desc);   /* floats of one network's running statistics */

/* acting (crossq.py:135-143): the policy in EVAL mode on obs [N, pdesc->in_dim]; key, subkey = split(key_io) (HOST, advanced);
 * action [N, A] = tanh(mean + std normal(subkey, (N, A))), or tanh(mean) when deterministic != 0 (the key advances either way). */
int rlx_crossq_act_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, const float* pstats, const float* obs, int64_t N,
                       uint32_t key_io[2], int scheme, float* action, int deterministic, const rlx_crossq_hparams* hp, void* stream);

/* the critic update (crossq.py:147-206) in one call on one stream, no host synchronisation: key, subkey = split(key); the policy in
 * EVAL mode on s'; a' = tanh(.) from ONE block draw normal(subkey, (B, A)), logp' with the 1e-6 term; every critic in TRAIN mode on
 * the 2 B rows [(s, a); (s', a')] in one joint pass; q = the first B outputs, next_q the last B; y = r + gamma (1 - term) (min_e next_q
 * - alpha logp') under stop_gradient; q_loss = mean over E and B of (q - y)^2; plain Adam with critic_adam_b1 at step q_opt_count + 1
 * over all E critics, no clipping; qstats advance.  q_opt_count_io (HOST) += 1.  metrics_out DEVICE float[10] in
 * rlx_sac_update_f32's order: this call writes [0] q_loss and [7] critic_grad_norm and leaves the other slots alone.  pparams,
 * pstats and log_alpha are only read. */
int rlx_crossq_critic_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, const float* pstats,
                                 const rlx_mlp_desc* qdesc, float* qparams /*[E*nq]*/, float* qm, float* qv, float* qstats /*[E*ns]*/,
                                 const float* log_alpha, const float* states /*[B,O]*/, const float* next_states,
                                 const float* actions, const float* rewards /*[B]*/, const float* terminations, int64_t B,
                                 uint32_t key_io[2], int scheme, int64_t* q_opt_count_io /* += 1 */, const rlx_crossq_hparams* hp,
                                 float* metrics_out /*DEVICE [10]*/, void* stream);

/* the policy and entropy update (crossq.py:210-274) on the same batch: key, subkey = split(key); the policy in TRAIN mode on s; a
 * block draw (B, A); the critics in EVAL mode with the statistics as the critic update left them; policy_loss = mean(alpha logp -
 * min_e q), the gradient to the minimising critic (split evenly among exact ties, as jnp.min's); entropy_loss = mean(exp(log_alpha)
 * (-logp - target_entropy)); Adam on the policy with policy_adam_b1 and on log_alpha with alpha_adam_b1, both at step pi_opt_count +
 * 1; pstats advance.  pi_opt_count_io (HOST) += 1.  metrics_out: this call writes [1..6], [8] and [9] (= 0) and leaves [0] and [7]
 * alone.  qparams and qstats are only read.  hp->critic_states (with critic_next_states non-NULL too) gives the critics' columns. */
int rlx_crossq_policy_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, float* pstats,
                                 const rlx_mlp_desc* qdesc, const float* qparams, const float* qstats, float* log_alpha, float* am,
                                 float* av, const float* states /*[B,O]*/, int64_t B, uint32_t key_io[2], int scheme,
                                 int64_t* pi_opt_count_io /* += 1 */, const rlx_crossq_hparams* hp, float* metrics_out, void* stream);

/* =================================== REPPO ===============================================
 * Relative Entropy Pathwise Policy Optimization (rl_x/algorithms/reppo/pytorch): on-policy rollouts, soft TD-lambda targets,
 * per minibatch a distributional critic step and a pathwise policy step through the updated critic with a sampled KL trust
 * region.  nn.RMSNorm = weight only, eps = float32 epsilon 1.1920929e-07.  Hidden widths: multiples of 64, at most 768;
 * act_dim <= 64; nr_bins 2..256.
 * POLICY FLAT LAYOUT (policy.py:42-52): W1[policy_obs_dim, Hp], b1[Hp], rms1[Hp] | W2[Hp, Hp], b2, rms2 | head W[Hp, 2A], b[2A]
 *   (columns [0, A) = loc, [A, 2A) = log_std) | log_entropy_coefficient | log_kl_coefficient.
 * CRITIC FLAT LAYOUT (critic.py:33-55), Hc = critic_hidden: encoder W1[critic_obs_dim + A, Hc], b1, rms1 | W2[Hc, Hc], b2 (-> the
 *   features F) | critic_head W3[Hc, Hc], b3, rms3 | W4[Hc, nr_bins], b4 | pred_head W5[Hc, Hc], b5, rms5 | W6[Hc, Hc + 1], b6
 *   (column 0 = reward, 1.. = next features) | zero_distribution[nr_bins].  Both heads start with SiLU(F).
 * Observations: the FULL normalised state rows [., O]; pidx / cidx: DEVICE int32 policy / critic column indices
 * (policy_observation_indices / critic_observation_indices), or NULL when that network sees all O columns.
 * Noise: threefry, key, subkey(s) = split(key) per call; rlx_dbg_set_sac_noise(eps_next, eps_cur) injects the N(0, 1) draws:
 * eps_next = act / evaluate_next [N, A] and the policy step's new-action noise [B, A]; eps_cur = its old-policy noise [K, B, A]. */
typedef struct rlx_reppo_desc {
  int32_t policy_obs_dim, critic_obs_dim, act_dim;
  int32_t policy_hidden, critic_hidden;  /* policy_hidden_dim, critic_hidden_dim (default_config.py: 512, 512) */
  int32_t nr_bins;
} rlx_reppo_desc;
/* net 0: policy, 1: critic; -1 on a bad descriptor */
int64_t rlx_reppo_param_count(const rlx_reppo_desc*, int net);

typedef struct rlx_reppo_hparams { /* reppo/pytorch/default_config.py */
  float gamma, gae_lambda, v_min, v_max;
  float kl_bound;
  float target_entropy;          /* act_dim * target_entropy_multiplier (reppo.py:63) */
  float policy_min_std;
  float auxiliary_loss_coefficient;
  float max_grad_norm;           /* clip_grad_norm_ of both networks (reppo.py:134, :172); <= 0: none */
  float adam_b1, adam_b2, adam_eps;  /* torch.optim.Adam defaults (reppo.py:97-98) */
  int32_t nr_kl_samples;         /* 1..1024 */
} rlx_reppo_hparams;

/* REPPO's ObservationNormalizer (reppo/pytorch/observation_normalizer.py) -- NOT rlx_obs_norm_*: count is a DEVICE float32
 * starting at 1e-4 and advanced in float32; update merges the batch mean / population variance of obs[N, O] into mean / var
 * (:14-28); apply: out = (obs - mean) / sqrt(var + 1e-8) (:31-34, out may alias obs).                                         */
int rlx_reppo_obs_norm_update_f32(rlx_ctx*, const float* obs, int64_t N, int O, float* mean, float* var, float* count, void* stream);
int rlx_reppo_obs_norm_apply_f32(rlx_ctx*, const float* obs, int64_t N, int O, const float* mean, const float* var, float* out,
                                 void* stream);
/* rollout_act (reppo.py:187-192): policy on obs, Policy.sample_and_log_prob (policy.py:56-64): action = tanh(loc + (exp(log_std)
 * + min_std) eps) [N, A] (what the batch stores), processed_action = low + 0.5 (clamp(action, -1, 1) + 1)(high - low) (what the env
 * gets; low / high DEVICE float[A]).  deterministic: action = tanh(loc) (evaluation, test(); policy.py:77-78), key untouched.   */
int rlx_reppo_act_f32(rlx_ctx*, const rlx_reppo_desc*, const float* pparams, const float* obs, int O, const int32_t* pidx,
                      uint32_t key_io[2], int scheme, float* action, float* processed_action, const float* low, const float* high, int64_t N,
                      int deterministic, const rlx_reppo_hparams* hp, void* stream);
/* rollout_evaluate_next (reppo.py:195-204) on the normalised actual next state: a fresh policy sample a' with its log-prob, the
 * critic encoder + critic_head on (s', a') (the pred_head is skipped: unused).  Writes next_features[N, critic_hidden] (F),
 * next_value[N] = sum softmax(logits + 40 zero_distribution) centers, soft_reward[N] = r - gamma next_logp exp(log_entropy_coef). */
int rlx_reppo_evaluate_next_f32(rlx_ctx*, const rlx_reppo_desc*, const float* pparams, const float* qparams, const float* next_obs, int O,
                                const int32_t* pidx, const int32_t* cidx, const float* rewards, uint32_t key_io[2], int scheme,
                                float* next_features, float* next_value, float* soft_reward, int64_t N, const rlx_reppo_hparams* hp,
                                void* stream);
/* compute_td_lambda_targets (reppo.py:207-219): reverse scan over T of [T, N] arrays from next_values[T - 1], truncation branch */
int rlx_reppo_td_lambda_f32(rlx_ctx*, const float* soft_rewards, const float* next_values, const float* terminations,
                            const float* truncations, int T, int N, float gamma, float gae_lambda, float* targets, void* stream);
/* ONE critic_loss_fn call (reppo.py:119-136) on the batch rows `rows` (DEVICE int32[B]; NULL: rows 0..B-1) of the flat batch
 * (states [., O], actions [., A], rewards, targets, terminations, truncations [.], next_features [., critic_hidden]): HL-Gauss
 * cross-entropy masked by (1 - trunc) + auxiliary_loss_coefficient x the masked next-feature / reward prediction loss, backward,
 * clip_grad_norm_(max_grad_norm), torch.optim.Adam step number `step` (>= 1) at learning rate lr.  metrics_out: DEVICE float[5] =
 * {critic_update_loss, auxiliary_loss, q_mean, explained_variance, critic_grad_norm (before clipping)}.                      */
int rlx_reppo_critic_step_f32(rlx_ctx*, const rlx_reppo_desc*, float* qparams, float* qm, float* qv, const float* states, int O,
                              const int32_t* cidx, const float* actions, const float* rewards, const float* targets,
                              const float* next_features, const float* terminations, const float* truncations, const int32_t* rows,
                              int64_t B, int64_t step, float lr, const rlx_reppo_hparams* hp, float* metrics_out, void* stream);
/* ONE policy_loss_fn call (reppo.py:140-184) with the critic's parameters frozen (differentiated through to the action):
 * pathwise value of a fresh sample, the old policy's (old_pparams) nr_kl_samples samples and the new policy's log-prob at them
 * (atanh of the clamped action), kl = mean_k(old_lp - new_lp); loss = where(kl < kl_bound, alpha logp - value, beta kl) +
 * the two coefficient losses; clip_grad_norm_, Adam.  metrics_out: DEVICE float[9] = {policy_loss, entropy_coefficient_loss,
 * kl_coefficient_loss, entropy, kl_divergence, entropy_coefficient, kl_coefficient, policy_q_mean, policy_grad_norm}.        */
int rlx_reppo_policy_step_f32(rlx_ctx*, const rlx_reppo_desc*, float* pparams, float* pm, float* pv, const float* old_pparams,
                              const float* qparams, const float* states, int O, const int32_t* pidx, const int32_t* cidx,
                              const int32_t* rows, int64_t B, uint32_t key_io[2], int scheme, int64_t step, float lr,
                              const rlx_reppo_hparams* hp, float* metrics_out, void* stream);
/* The whole optimisation phase of one iteration (reppo.py:358-397): for every epoch e and minibatch m, the rows
 * perm[e, m * mb : (m + 1) * mb] (perm: DEVICE int32[nr_epochs, batch], mb = batch / nr_minibatches), one critic step then one
 * policy step on the updated critic, both at Adam step *opt_count_io + 1 (advanced per minibatch).  metrics_out: DEVICE
 * float[nr_epochs * nr_minibatches, 14] = the critic step's 5 values then the policy step's 9 per minibatch (no host sync).  */
int rlx_reppo_update_f32(rlx_ctx*, const rlx_reppo_desc*, float* pparams, float* pm, float* pv, const float* old_pparams,
                         float* qparams, float* qm, float* qv, const float* states, int O, const int32_t* pidx, const int32_t* cidx,
                         const float* actions, const float* rewards, const float* targets, const float* next_features,
                         const float* terminations, const float* truncations, int64_t batch, const int32_t* perm, int nr_epochs,
                         int nr_minibatches, uint32_t key_io[2], int scheme, int64_t* opt_count_io, float lr, const rlx_reppo_hparams* hp,
                         float* metrics_out, void* stream);

/* =================================== MPO =================================================
 * Maximum a posteriori policy optimisation (rl_x/algorithms/mpo/pytorch): a C51-style critic whose target is the triangular
 * projection of the target critic's distributions at S target-policy samples per next state, a non-parametric E-step over S
 * samples per state, a decoupled Gaussian M-step with per-dimension KL terms, and Adam on the dual variables.
 * Hidden widths: a multiple of 64, at most 512 (every layer has the same width); act_dim 1..64; nr_atoms 2..128;
 * action_sampling_number 1..64; any batch B >= 1.  torch.nn.LayerNorm eps 1e-5.
 * POLICY FLAT LAYOUT (policy.py:39-49), H = hidden: W1[policy_obs_dim, H], b1[H], ln_g[H], ln_b[H] | W2[H, H], b2 | W3[H, H], b3 |
 *   head W[H, 2A], b[2A] (columns [0, A) = the `mean` Linear, [A, 2A) = the `std` Linear before the softplus).
 * CRITIC FLAT LAYOUT (q_network.py:28-37): W1[critic_obs_dim + A, H] (rows [0, critic_obs_dim) = observation, then action), b1,
 *   ln_g, ln_b | W2, b2 | W3, b3 | head W[H, nr_atoms], b[nr_atoms].
 * DUALS (dual_variables.py:7-10): log_eta | log_alpha_mean[A] | log_alpha_stddev[A] | log_penalty_temperature  (2A + 2 floats).
 * Observations: the FULL normalised state rows [., O]; pidx / cidx: DEVICE int32 policy / critic column indices, or NULL.
 * Noise: threefry, key, subkey(s) = split(key) per call; rlx_dbg_set_sac_noise(eps_next, eps_cur) injects the N(0, 1) draws:
 * eps_next = act [N, A] / the critic step's samples [S, B, A]; eps_cur = the actor step's samples [S, 2B, A].                   */
typedef struct rlx_mpo_desc {
  int32_t policy_obs_dim, critic_obs_dim, act_dim;
  int32_t hidden;                /* nr_hidden_units (default_config.py: 256) */
  int32_t nr_atoms;
} rlx_mpo_desc;
/* net 0: policy, 1: critic, 2: duals; -1 on a bad descriptor */
int64_t rlx_mpo_param_count(const rlx_mpo_desc*, int net);

typedef struct rlx_mpo_hparams { /* mpo/pytorch/default_config.py */
  float gamma, v_min, v_max;
  float max_grad_norm;           /* clip_grad_norm_ of all three optimisers (mpo.py:155, :235, :241); <= 0: none */
  float epsilon_non_parametric, epsilon_parametric_mu, epsilon_parametric_sigma, epsilon_penalty;
  float policy_init_scale, policy_min_scale;
  float float_epsilon, min_log_temperature, min_log_alpha;
  float adam_b1, adam_b2, adam_eps;  /* torch.optim.Adam defaults (mpo.py:101-103) */
  int32_t action_sampling_number;    /* S: 1..64 */
  int32_t action_clipping, action_rescaling;
} rlx_mpo_hparams;

/* Policy.sample_action / get_deterministic_action (policy.py:89-97) on obs [N, O]: action = mean + std eps [N, A] (what the ring
 * stores), processed_action = scale_to_env(action): clamp to [-1, 1] (action_clipping), then low + 0.5 (p + 1)(high - low)
 * (action_rescaling; low / high DEVICE float[A]).  deterministic: action = mean, key untouched.                                */
int rlx_mpo_act_f32(rlx_ctx*, const rlx_mpo_desc*, const float* pparams, const float* obs, int O, const int32_t* pidx,
                    uint32_t key_io[2], int scheme, float* action, float* processed_action, const float* low, const float* high, int64_t N,
                    int deterministic, const rlx_mpo_hparams* hp, void* stream);
/* ONE `update` (mpo.py:124-267) on the batch states, next_states [B, O], actions [B, A], rewards, dones, truncations,
 * effective_n_steps [B]: the critic step (S target-policy samples per next state through the target critic, triangular projection,
 * cross-entropy, clip_grad_norm_, Adam at agent_lr), the actor step on [states; next_states] (E-step weights, M-step losses, clip, Adam
 * at agent_lr) and the dual step (Adam at dual_lr, clip, clamps).  The target networks are only read.  All three optimisers take
 * Adam step number `step` (>= 1).  metrics_out: DEVICE float[17] in the order of mpo.py:389-407 = {critic_loss, actor_loss,
 * dual_loss, loss_eta, loss_alpha, current_q_mean, eta, penalty_temperature, alpha_mean, alpha_std, mean_kl_mean, mean_kl_std,
 * actor_grad_norm, critic_grad_norm, dual_grad_norm, std_min_mean, std_max_mean}.  No host synchronisation.                    */
int rlx_mpo_update_f32(rlx_ctx*, const rlx_mpo_desc*, float* pparams, float* pm, float* pv, const float* target_pparams,
                       float* qparams, float* qm, float* qv, const float* target_qparams, float* duals, float* dm, float* dv,
                       const float* states, const float* next_states, int O, const int32_t* pidx, const int32_t* cidx,
                       const float* actions, const float* rewards, const float* dones, const float* truncations,
                       const float* effective_n_steps, int64_t B, uint32_t key_io[2], int scheme, int64_t step, float agent_lr,
                       float dual_lr, const rlx_mpo_hparams* hp, float* metrics_out, void* stream);

/* =================================== ESPO ================================================
 * Early-stopping policy optimisation (rl_x/algorithms/espo/pytorch).  The nets are PPO's arch A (policy.py:31-38, critic.py:24-30:
 * two tanh layers of nr_hidden_units; the policy has the trailing policy_logstd), so acting, next values and GAE are
 * rlx_ppo_rollout_f32 / rlx_actor_critic_fwd_sample_f32, rlx_ppo_next_values_f32 and rlx_gae_f32 (espo.py:99-110, 186-230).   */
typedef struct rlx_espo_hparams { /* espo/pytorch/default_config.py:18-24 */
  float max_ratio_delta;
  float entropy_coef, critic_coef;
  float max_grad_norm;               /* clip_grad_norm_ of both optimisers (espo.py:137, :154); <= 0: none */
  float adam_b1, adam_b2, adam_eps;  /* torch.optim.Adam defaults (espo.py:87-88) */
  int32_t delta_op;                  /* delta_calc_operator: 0 torch.mean, 1 torch.median (the LOWER median, sorted[(mb - 1) / 2]) */
} rlx_espo_hparams;
/* The whole optimisation phase of one iteration (espo.py:236-278): for epoch e = 0 .. max_epochs - 1 on the rollout rows idx[e, :]
 * (idx: DEVICE int32[max_epochs, mb], each row drawn without replacement from [0, B), B = T * N) one policy step (policy_loss_fn,
 * espo.py:113-141: ratio, approx_kl, ratio_delta, advantages normalised with the UNBIASED std, pg_loss = mean(-A^ ratio) without
 * clipping, minus entropy_coef x entropy; clip_grad_norm_; Adam; policy_logstd is a parameter) and one critic step
 * (critic_loss_fn, :144-158) on the same rows, both at Adam step *opt_count_io + e + 1 and learning rate lr; THEN the loop ends if
 * ratio_delta > max_ratio_delta (:277-278: the epoch that trips the threshold is applied in full; a NaN never trips it).  The
 * stop is decided on the device: epochs are submitted in chunks ("espo_chunk"), later epochs of chunks already submitted run as
 * no-ops behind a device-side gate, and the host waits once, at the end of the call, to write *epochs_run_out (HOST, the
 * reference's `epoch + 1`) and to advance *opt_count_io (HOST) by it.
 * states: the FULL observation rows [B, O]; pidx / cidx: DEVICE int32[n_pidx] / [n_cidx] policy / critic column indices inside
 * [0, O), or NULL (the net reads all O columns; n_* ignored).  pdesc / cdesc: arch A (n_hidden 2, act TANH, ln_first 0; both
 * hidden widths one multiple of 64 in 64..512, the same for both nets), pdesc: in_dim = n_pidx or O, out_dim = action dim 1..64,
 * has_logstd 1; cdesc: in_dim = n_cidx or O, out_dim 1, has_logstd 0.  Flat layouts: rlx_mlp_param_count.  2 <= mb <= 4096
 * (torch.std of one element is NaN), mb <= B, max_epochs >= 1.  A descriptor or mb outside that is RLX_EUNSUP, every other bad
 * argument RLX_EINVAL (an index outside its range included: nothing is applied then).
 * metrics_out: DEVICE float[max_epochs, 8], one row per EXECUTED epoch = {pg_loss, critic_loss, entropy_loss, ratio_delta,
 * approx_kl, policy_grad_norm, critic_grad_norm (both before clipping), reserved}; rows past *epochs_run_out are left untouched.
 * A step whose gradient norm is not finite is skipped on the device, as everywhere in this library.                          */
int rlx_espo_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, const rlx_mlp_desc* cdesc,
                        float* cparams, float* cm, float* cv, const float* states, int O, const int32_t* pidx, int n_pidx,
                        const int32_t* cidx, int n_cidx, const float* actions, const float* log_probs, const float* returns,
                        const float* advantages, int64_t B, const int32_t* idx, int mb, int max_epochs, int64_t* opt_count_io, float lr,
                        const rlx_espo_hparams* hp, float* metrics_out, int32_t* epochs_run_out, void* stream);

/* =================================== FastMPO =============================================
 * Massively parallel MPO (rl_x/algorithms/fastmpo/flax_full_jit): one or two categorical critics whose target is the floor/ceil
 * projection (FastSAC's, c51_body.h) of the MEAN over K target-policy samples of the target critics' pmfs, MPO's E-step over the
 * min or mean of the critics and its M-step and dual step (mpo.hip's kernels), optax's clip_by_global_norm + adamw for policy,
 * critic and duals, Polyak targets for policy and critic.
 * Networks (policy.py:42-124, critic.py:25-89), kind 0 "fastsac": Dense -> LayerNorm(1e-6) -> SiLU x3; 1 "fasttd3": Dense -> ReLU
 * x3; 2 "mpo": Dense -> LayerNorm(1e-6) -> tanh, then Dense -> ELU x2.  Widths: multiples of 64, at most 1024 without a LayerNorm,
 * 768 behind (LayerNorm, SiLU), 512 behind (LayerNorm, tanh) (the row-norm kernels hold a row in one wave).
 * FLAT LAYOUTS: per hidden layer W[in, out] row-major, b[out], then ln_scale[out], ln_bias[out] where the layer has a LayerNorm;
 * then the head W[in, out], b[out].  Policy head [H3, 2A] = [mean | std pre-activation] columns (policy.py:61-64: two Dense
 * layers side by side); std = min_scale + softplus(raw) init_scale / softplus(0).  Critic input [critic obs | action]; with
 * dual_critic the second critic's parameters follow the first's.  DUALS as MPO's: log_eta | log_alpha_mean[A] |
 * log_alpha_stddev[A] | log_penalty_temperature.
 * act_dim 1..64, nr_atoms 2..128, action_sampling_number 1..64.                                                               */
typedef struct rlx_fastmpo_desc {
  int32_t policy_obs_dim, critic_obs_dim, act_dim, nr_atoms;
  int32_t dual_critic;                 /* two critics (critic.py:92-108) */
  int32_t policy_kind, critic_kind;    /* 0 fastsac, 1 fasttd3, 2 mpo */
  int32_t policy_hidden[3], critic_hidden[3];
} rlx_fastmpo_desc;
/* net 0: policy, 1: ONE critic, 2: duals; -1 on a bad descriptor */
int64_t rlx_fastmpo_param_count(const rlx_fastmpo_desc*, int net);

typedef struct rlx_fastmpo_hparams { /* fastmpo/flax_full_jit/default_config.py, what the update reads */
  float gamma, v_min, v_max;
  float max_grad_norm;               /* optax.clip_by_global_norm of all three optimisers (fastmpo.py:158, :168, :177); <= 0: none */
  float policy_weight_decay, critic_weight_decay, dual_weight_decay;   /* optax.adamw */
  float adam_b1, adam_b2, adam_eps;  /* adam_beta1, adam_beta2; optax's eps 1e-8 */
  float critic_tau, policy_tau;      /* optax.incremental_update (fastmpo.py:593, :622) */
  float epsilon_non_parametric, epsilon_parametric_mu, epsilon_parametric_sigma, epsilon_penalty;
  float policy_init_scale, policy_min_scale;
  float float_epsilon, min_log_temperature, min_log_alpha;
  int32_t action_sampling_number;    /* K: 1..64 */
  int32_t action_clipping;
  int32_t action_rescaling;          /* 0 none, 1 normal, 2 fastsac (policy.py:127-138) */
  int32_t clipped_double_q_learning; /* needs dual_critic */
  int32_t nr_critic_updates_per_policy_update, nr_policy_updates_per_step;   /* G, P */
} rlx_fastmpo_hparams;

/* Acting (fastmpo.py:287-290, evaluation :678-680) on the normalised obs [N, O]: action = mean + std eps [N, A] (what the ring
 * stores; deterministic: the mean, key untouched) from the GIVEN policy parameters -- online or target, as
 * collect_data_with_online_policy says; processed_action = get_processed_action(action) (policy.py:127-138): clip to [-1, 1]
 * (action_clipping), then action_rescaling 1: low + 0.5 (a + 1)(high - low), 2: a * action_scale (passed in `low`).  key, subkey =
 * split(key); rlx_dbg_set_sac_noise(eps_next, .) injects the N(0, 1) draws [N, A].                                             */
int rlx_fastmpo_act_f32(rlx_ctx*, const rlx_fastmpo_desc*, const float* pparams, const float* obs, int O, const int32_t* pidx,
                        uint32_t key_io[2], int scheme, float* action, float* processed_action, const float* low, const float* high,
                        int64_t N, int deterministic, const rlx_fastmpo_hparams* hp, void* stream);
/* The optimisation of ONE learning iteration (fastmpo.py:572-627): P rounds; round p runs G critic steps on the batches u = p G ..
 * p G + G - 1 of states, next_states [P G, B, O] (normalised), actions [P G, B, A], rewards, dones, truncations,
 * effective_n_steps [P G, B] -- critic_loss_fn (:314-379), clip + adamw at critic_lr[u], and the critic's Polyak update inside the
 * same Adam launch (:586-593) -- then one policy and dual step on the round's last batch against the updated target critic
 * (policy_and_dual_loss_fn :381-482, :603-620) at policy_lr[p] / dual_lr[p], and the policy's Polyak update (:622).  The target
 * policy is read on s' in the critic steps and on [s; s'] in the policy step.  qparams / qm / qv / target_qparams: the critics
 * back to back (one optimiser over both).  critic_lr [P G], policy_lr [P], dual_lr [P]: HOST arrays.  opt_count_io: HOST
 * int64[3] = optimiser steps so far of {critic, policy, duals}, advanced by P G, P, P when the call returns RLX_OK (untouched on an
 * error).
 * Noise: per-row keys as the reference draws them: row_keys = split(noise_key, P G B 3) (:513-514); the critic step u draws row
 * b's normal of shape (K, A) from row_keys[(u B + b) 3], the policy step its (K, 2, A) from row_keys[(u B + b) 3 + 2] (:582-584;
 * policy_and_dual_loss_fn takes two keys and draws from the second only).  rlx_dbg_set_sac_noise(eps_next, eps_cur) injects the
 * draws instead: eps_next [P G, K, B, A] for the critic steps, eps_cur [P, K, 2B, A] for the policy steps.
 * metrics_out: DEVICE float[28], the last critic step's {q_loss, q_mean, q_max, q_min, critic_learning_rate, critic_grad_norm}
 * then the last policy step's {actor_loss, loss_pg_mean, loss_pg_std, loss_kl_mean, loss_kl_std, dual_loss, loss_alpha_mean,
 * loss_alpha_std, loss_eta, eta, penalty_temperature, alpha_mean, alpha_std, mean_kl_mean, mean_kl_std, improvement_q_mean,
 * std_min_mean, std_max_mean, policy_learning_rate, dual_variables_learning_rate, policy_grad_norm, dual_variables_grad_norm}
 * (:372-377, :595-596, :461-480, :624-627).  No host synchronisation inside the call.
 * RLX_EINVAL / RLX_EUNSUP outside the envelope: clipped_double_q_learning without dual_critic, K or act_dim outside 1..64, nr_atoms
 * outside 2..128, a width that is no multiple of 64 or past its kind's limit, a kind outside 0..2, P or G < 1.                 */
int rlx_fastmpo_update_f32(rlx_ctx*, const rlx_fastmpo_desc*, float* pparams, float* pm, float* pv, float* target_pparams,
                           float* qparams, float* qm, float* qv, float* target_qparams, float* duals, float* dm, float* dv,
                           const float* states, const float* next_states, int O, const int32_t* pidx, const int32_t* cidx,
                           const float* actions, const float* rewards, const float* dones, const float* truncations,
                           const float* effective_n_steps, int64_t B, const uint32_t noise_key[2], int scheme, int64_t* opt_count_io,
                           const float* critic_lr, const float* policy_lr, const float* dual_lr, const rlx_fastmpo_hparams* hp,
                           float* metrics_out, void* stream);

/* =================================== PPO + LSTM =======================================
 * Recurrent policy (rl_x/algorithms/ppo_lstm/flax_full_jit/policy.py:32-142, "concat" and "film" decoders):
 *   lstm_obs_encode / obs_encode: Dense(E)+LN+ELU on obs; OptimizedLSTMCell(H); LN+ELU on h;
 *   torso Dense(D1)+LN+ELU, Dense(D2)+ELU, Dense(D3)+ELU; mean head; state-independent logstd.
 * FLAT LAYOUT: enc_l {W[O,E], b, ln_g, ln_b} | enc_o {same} (absent when share_encoder) |
 *   lstm Wi[E,4H] (gate blocks i,f,g,o; no bias), Wh[H,4H], bh[4H] | lstm_ln g[H], b[H] |
 *   [film W[H,2E], b[2E] iff combine = FILM] | torso1 W[E+H,D1] ([E,D1] with FiLM), b, ln_g, ln_b | torso2 W, b |
 *   torso3 W, b | head W[D3,A], b | logstd[A].
 * The critic is the feed-forward PPO critic (ppo_lstm/flax_full_jit/critic.py:18-33).           */
typedef struct rlx_lstm_policy_desc {
  int32_t obs_dim, act_dim;
  int32_t enc_dim;      /* obs_encoding_dim  (default_config.py)                   */
  int32_t lstm_hidden;  /* lstm_hidden_dim: 64 in this build                       */
  int32_t torso[3];     /* policy torso widths (512, 256, 128)                     */
  int32_t share_encoder;/* share_lstm_obs_encoder / share_gru_obs_encoder          */
  int32_t cell;         /* RLX_CELL_LSTM, or RLX_CELL_GRU: the PPO+GRU policy
                         * (rl_x/algorithms/ppo_gru/flax_full_jit/policy.py:33-141, nn.GRUCell, single carry h:
                         * c_io / c0 arguments are then ignored).  GRU flat layout of the cell block:
                         * Wi[E,3H] (gate blocks r,z,n), bi[3H], Wh_rz[H,2H], Wh_n[H,H], bhn[H]. */
  int32_t combine;      /* lstm_obs_combine_method (policy.py:95-100): RLX_COMBINE_CONCAT: torso input = [obs latent | cell
                         * latent] (E + H wide); RLX_COMBINE_FILM: gamma = Dense(E)(cell latent), beta = Dense(E)(cell latent),
                         * torso input = obs latent * gamma + beta (E wide).  FiLM flat layout: after lstm_ln comes
                         * film W[H, 2E] (columns [0,E) = gamma kernel, [E,2E) = beta kernel), b[2E]; torso1 W is [E, D1]. */
} rlx_lstm_policy_desc;
#define RLX_CELL_LSTM 0
#define RLX_CELL_GRU 1
#define RLX_COMBINE_CONCAT 0
#define RLX_COMBINE_FILM 1

int64_t rlx_lstm_policy_param_count(const rlx_lstm_policy_desc* desc);

/* acting half of `single_rollout` (ppo_lstm.py:137-146): key, sub = split(key); Policy.apply_one_step
 * (policy.py:121-131) on obs [N,O] with carry (c_io, h_io) [N,H] updated IN PLACE (NOT yet masked with
 * done: the caller multiplies by (1-done) after the env step, ppo_lstm.py:148-149 -> rlx_lstm_mask_carry_f32);
 * action = mean + std * normal(sub, [N_global, A])[rows], log_prob, processed action, critic value.
 * deterministic != 0 (test mode): action = mean, key untouched.                                        */
/* the recurrent counterpart of rlx_ppo_rollout_begin (same contract; rlx_ppo_rollout_end and the parameter-updating entry
 * points drop the images): the fused decoder of the acting steps that follow runs its hidden layers on the fp16 matrix pipe  */
int rlx_ppo_lstm_rollout_begin(rlx_ctx* ctx, const rlx_lstm_policy_desc* desc, const float* pparams, const rlx_mlp_desc* cdesc,
                               const float* cparams, void* stream);
int rlx_ppo_lstm_act_f32(rlx_ctx*, const rlx_lstm_policy_desc* desc, const float* pparams, const rlx_mlp_desc* cdesc,
                         const float* cparams, const float* obs, const float* critic_obs /* NULL: the critic reads obs; else DEVICE
                         [N, cdesc->in_dim], its own observation columns (critic_observation_indices, critic.py:12,23) */,
                         float* c_io, float* h_io, uint32_t key_io[2],
                         int scheme, float* action, float* processed, float* value, float* logp, int N,
                         int clip_and_rescale, const float* act_low, const float* act_high, int noise_row_offset,
                         int N_global, int deterministic, void* stream);
/* carry *= (1 - done[:, None])   (ppo_lstm.py:148-149); done = terminated | truncated as 0/1 floats */
int rlx_lstm_mask_carry_f32(rlx_ctx*, float* c_io, float* h_io, const float* terminated, const float* truncated,
                            float* done_out /*[N] or NULL*/, int N, int H, void* stream);
/* one sequence minibatch of `minibatch_update` (ppo_lstm.py:231-259): gathers envs env_idx[ne] (all T steps,
 * rollout arrays [T,N,.]; c0/h0 [N,H] = rollout_init_policy_carry), normalises the advantages over the minibatch,
 * forward_sequence + loss_fn (ppo_lstm.py:181-216) + BPTT.  pgrads/cgrads/metrics as rlx_ppo_minibatch_fwd_bwd_f32. */
int rlx_ppo_lstm_minibatch_fwd_bwd_f32(rlx_ctx*, const rlx_lstm_policy_desc* desc, const float* pparams, float* pgrads,
                                       const rlx_mlp_desc* cdesc, const float* cparams, float* cgrads, float* metrics,
                                       const float* states, const float* actions, const float* log_probs,
                                       const float* returns, const float* advantages, const float* dones,
                                       const float* c0, const float* h0, const int32_t* env_idx, int nr_minibatch_envs,
                                       int T, int N, const rlx_ppo_hparams* hp, void* stream);
/* the whole optimisation phase (ppo_lstm.py:222-263): env-index permutation [E,N] -> E*M minibatches of
 * minibatch_size // T envs, clip + Adam per minibatch.  metrics_out: DEVICE float[E*M, 10] as rlx_ppo_update_f32.
 * Data parallel (context created with world > 1): N = THIS RANK's envs, minibatch_size = the GLOBAL minibatch.
 * Every rank permutes its local env indices with the same replicated key and contributes minibatch_size / (T * world) envs
 * to each minibatch (global minibatch = union over the ranks, each env once per epoch).  Collectives, all issued by the
 * library: the fp64 advantage sums of all minibatches once per call, each network's gradient once per minibatch on that
 * network's stream, the metrics once per call; losses are scaled by 1 / minibatch_size and every rank applies the same clip +
 * Adam step to the reduced gradients.                                                                                    */
int rlx_ppo_lstm_update_f32(rlx_ctx*, const rlx_lstm_policy_desc* desc, float* pparams, float* pm, float* pv,
                            const rlx_mlp_desc* cdesc, float* cparams, float* cm, float* cv, const float* states,
                            const float* actions, const float* log_probs, const float* returns, const float* advantages,
                            const float* dones, const float* c0, const float* h0, int T, int N, int nr_epochs,
                            int minibatch_size, uint32_t key_io[2], int scheme, int64_t* opt_count_io,
                            const float* lr_schedule, const rlx_ppo_hparams* hp, float* metrics_out, void* stream);

/* ---- TD3 and DDPG: deterministic policy gradients (rl_x/algorithms/td3/flax, rl_x/algorithms/ddpg/flax) ----------------------
 * SAC's host loop and replay ring (td3/flax/replay_buffer.py and ddpg/flax/replay_buffer.py are sac/flax's file) with a tanh
 * policy that has no log-std (policy.py:22-44: Dense(H) -> ReLU -> Dense(H) -> ReLU -> Dense(act_dim) -> tanh, the tanh applied
 * by the entry points below) AND a target copy of it, and nr_critics scalar critics (td3/flax/critic.py:17-53: two, BACK TO BACK
 * in one flat vector like rlx_redq_update_f32's; ddpg/flax/critic.py: one).  Networks: rlx_mlp_desc with act = RLX_ACT_RELU,
 * ln_first = 0, has_logstd = 0; FLAT LAYOUT of a network: FastTD3's (above).  Q values are laid out [E, B], critic-major.
 * Envelope: 1..3 hidden layers, widths multiples of 64 up to 1024, act_dim = pdesc->out_dim in 1..64, qdesc->out_dim = 1,
 * nr_critics 1 or 2, joint only with nr_critics == 1, smoothing_epsilon == 0 and policy_step, B > 0, a context of world size 1; a
 * descriptor or size outside it is RLX_EUNSUP, every other bad argument RLX_EINVAL, rlx_last_error() names the rule, and nothing
 * is written when a check fails.                                                                                                */
typedef struct rlx_td3_hparams {               /* td3/flax/default_config.py:9-27, ddpg/flax/default_config.py:9-24 */
  float gamma, tau;
  float smoothing_epsilon, smoothing_clip_value;   /* target-policy smoothing (td3.py:126-127) */
  float lr_policy, lr_critic;                  /* host evaluates linear_schedule at each optimiser's OWN count (td3.py:72-79) */
  float adam_b1, adam_b2, adam_eps;            /* optax.adam defaults 0.9, 0.999, 1e-8 (td3.py:88, :95) */
  int32_t nr_critics;                          /* 2: TD3 (critic.py:13), 1: DDPG */
  int32_t joint;                               /* DDPG's order (ddpg.py:118-156): both gradients at the pre-step parameters, no key */
  int32_t policy_step;                         /* 0: the critic step only, the targets stay (td3.py:266: the delayed policy step) */
  const float *critic_states, *critic_next_states;   /* as in rlx_redq_hparams: the critics' own observation columns of s / s' */
} rlx_td3_hparams;

/* get_action (td3.py:107-112, ddpg.py:105-110) and get_deterministic_action (td3.py:203-205): action [N, A] = clip(tanh(policy(obs))
 * + epsilon normal(subkey, (N, A)), -1, 1) with key, subkey = split(key) -- ONE shape-wide draw, element (n, j) from bits n A + j of
 * N A; processed_action = low + 0.5 (clip(action, -1, 1) + 1)(high - low) (policy.py:39-44; low / high DEVICE float[A]).
 * epsilon == 0: the deterministic action, key_io untouched.  rlx_dbg_set_sac_noise(eps_next, .) injects the N(0, 1) draws [N, A]. */
int rlx_td3_act_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, const float* pparams, const float* obs, uint32_t key_io[2], int scheme,
                    float epsilon, float* action, float* processed_action, int N, const float* low, const float* high, void* stream);

/* the critic loss on given values (td3.py:130-134, meaned over batch and critics, :145): q, q_next DEVICE [E, B], E = nr_critics;
 * y_out [B] (or NULL) = r + gamma (1 - term) min_e q_next[e]; dq_out [E, B] = 2 (q - y) / (E B); loss_out DEVICE [1] = mean (q -
 * y)^2, double accumulators in a fixed order. */
int rlx_td3_losses_f32(rlx_ctx*, const float* q /*[E,B]*/, const float* q_next /*[E,B]*/, const float* rewards,
                       const float* terminations, int64_t B, const rlx_td3_hparams* hp, float* y_out, float* dq_out, float* loss_out,
                       void* stream);

/* ONE vector step's optimisation in one call, no host synchronisation: update_critic (td3.py:116-160) and, with hp->policy_step,
 * update_policy_and_targets (:164-199) -- or, with hp->joint, DDPG's `update` (ddpg.py:114-166).  Critic step: keys = split(key,
 * B + 1), key = keys[0], row b's smoothing noise from keys[1 + b] (td3.py:149-150; hp->joint: no key is taken);
 * rlx_dbg_set_sac_noise(eps_next, .) injects the N(0, 1) draws [B, A] instead.  The policy step evaluates the critics AFTER the
 * critic step's Adam (hp->joint: before it), steps the policy, then moves BOTH targets by tau (ptarget, qtarget); without a policy
 * step neither target moves.  qparams / qm / qv / qtarget: [E * nq].  states / next_states: the policy's columns [B, pdesc->in_dim].
 * q_opt_count_io / pi_opt_count_io (HOST): the two optax counts, advanced by 1 and by hp->policy_step.  metrics_out DEVICE
 * float[5] = {loss/q_loss, gradients/critic_grad_norm, loss/policy_loss, q_value/q_value, gradients/policy_grad_norm}; [2..4] are
 * left alone without a policy step. */
int rlx_td3_update_f32(rlx_ctx*, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, float* ptarget,
                       const rlx_mlp_desc* qdesc, float* qparams /*[E*nq]*/, float* qm, float* qv, float* qtarget, const float* states,
                       const float* next_states, const float* actions, const float* rewards, const float* terminations, int64_t B,
                       uint32_t key_io[2], int scheme, int64_t* q_opt_count_io, int64_t* pi_opt_count_io, const rlx_td3_hparams* hp,
                       float* metrics_out /*DEVICE [5]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RLX_HIP_H */
