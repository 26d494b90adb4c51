// common.h -- shared helpers for librlxhip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <functional>
#include "../../include/rlx_hip.h"

namespace rlx {

void set_error(const std::string& msg);

#define RLX_HIP_TRY(expr)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      ::rlx::set_error(std::string(#expr) + " failed: " + hipGetErrorString(e_) + " (" __FILE__ \
                       ":" + std::to_string(__LINE__) + ")");                                  \
      return RLX_EHIP;                                                                         \
    }                                                                                          \
  } while (0)

#define RLX_REQUIRE(cond, code, msg)                 \
  do {                                               \
    if (!(cond)) {                                   \
      ::rlx::set_error(std::string(msg));            \
      return (code);                                 \
    }                                                \
  } while (0)

#define RLX_LAUNCH_CHECK()                           \
  RLX_HIP_TRY(hipGetLastError())

constexpr int WAVE = 64;

// --------------------------------------------------------------------------- ctx
// Scratch arena: named slots that grow on demand (hipMalloc outside graph capture).
struct Scratch {
  void* ptr = nullptr;
  size_t bytes = 0;
};

enum ScratchSlot {
  SL_SORT_KEYS_A = 0, SL_SORT_KEYS_B, SL_SORT_VALS_B, SL_SORT_TMP, SL_PERM,
  SL_MB_X, SL_MB_XC, SL_MB_AUX, SL_STATS,
  SL_ACT_P0, SL_ACT_P1, SL_ACT_P2, SL_ACT_C0, SL_ACT_C1, SL_ACT_C2,
  SL_DACT_0, SL_DACT_1, SL_LN_P, SL_LN_C,
  SL_PARTIAL, SL_HEAD_PART, SL_NORM, SL_NORM2, SL_FWD_A, SL_FWD_B, SL_KEYS, SL_GRAD_P, SL_GRAD_C, SL_MEAN, SL_VALUE, SL_RO_NETS, SL_SAC, SL_LSTM, SL_LSTM_IDX, SL_STAGE, SL_OPT_A, SL_OPT_B, SL_STATS_ALL, SL_ZEROS, SL_STAT_PART, SL_LIDX, SL_COUNTS, SL_DIST_STATS, SL_OVERFLOW, SL_SCHED, SL_NV_ROWS, SL_WFRAG, SL_WFRAG_RO, SL_XMAX, SL_MB_GROUP_X, SL_MB_GROUP_AUX, SL_DZ0, SL_WFRAG_SAC, SL_ROW_REC, SL_RO_CRITIC_ES,
  SL_COUNT
};

// live per-kernel timing (bench.py roofline leg): HIP events around the launches of the
// instrumented kernels, recorded on the stream the kernel is launched on.
enum ProfKernel { PK_GEMM_FWD = 0, PK_GEMM_DX, PK_GEMM_DW, PK_DX_L1BWD,
                  // memory-bound kernels (rows with engine = 2, flops = 0, bytes = algorithmic HBM bytes; shape = (rows, width, 0))
                  PK_L1FWD, PK_HEAD_LOSS, PK_REDUCE,
                  PK_L12FWD, // first + second layer forward in one launch (l1fused.hip: k_l12fwd): engine 1, shape (rows, hidden[1], 512)
                  PK_TAIL,   // row-tile-local tail of a network's pass (ppo.hip: k_tail_bx): engine 1, shape (rows, 128, hidden[1])
                  PK_FWD2H,  // whole two-hidden-layer forward + head in one launch (fwd2h.hip: k_fwd2h): engine 1, shape (rows, 256, in_dim)
                  PK_COUNT };
constexpr int PROF_ENGINE_HBM = 2;
struct ProfRec {
  int kid, row;
  double flops, bytes;
  hipEvent_t e0, e1;
};
// one row per (kernel kind, engine, problem shape): EVERY launch is counted, every prof_sample-th launch OF THIS ROW carries
// events -- a per-row counter, so a periodic launch pattern (policy L2, L3, critic L2, L3, ...) cannot alias with the sampling
// stride and every shape is timed at the same rate
struct ProfRow {
  int kid, engine;        // engine: 0 exact-fp32 MFMA, 1 split-fp32 operands on the fp16 pipe
  int64_t M;
  int N, K;
  int64_t launches, timed;
  double ms, flops, bytes;   // over the timed launches
};
// Twin launches (grid.y == 2): the kernel's pointer arguments for blockIdx.y == 1 -- the second of two independent, equally
// shaped problems (SAC's twin critics, sac/flax/critic.py:44-53: a vmapped VectorCritic) in ONE launch.  Which four pointers
// these replace is stated at each kernel.
struct Twin { const void* p[4] = {nullptr, nullptr, nullptr, nullptr}; };

}  // namespace rlx

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device: a launcher's "already set" flag is one bit per
// device ordinal, not one per process (a process with contexts on two devices).
struct AttrOnce {
  uint64_t mask = 0;
  static int dev() { int d = 0; (void)hipGetDevice(&d); return d & 63; }
  bool done() const { return (mask >> dev()) & 1; }
  void mark() { mask |= 1ull << dev(); }
};

struct rlx_ctx {
  int device = 0;
  rlx::Scratch slots[3][rlx::SL_COUNT];   // bank 1: the critic's arenas when it runs on the side stream
  int bank = 0;                           // bank scratch() serves (host-side state)
  int opt_flip = 0;                       // rlx_clip_adam_step_f32 alternates two norm-partial buffers (calls on two streams)
  hipStream_t side = nullptr;             // second stream of the fused update (policy || critic)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_rows[2] = {nullptr, nullptr};   // pipelined PPO update: minibatch rows of parity p gathered (main stream)
  hipEvent_t ev_cdone[2] = {nullptr, nullptr};  //                        critic finished reading the rows of parity p (side stream)
  const float* dbg_sac_eps[2] = {nullptr, nullptr};   // test hook: N(0,1) draws of rlx_sac_update_f32 ([B, A] each) instead of the threefry stream
  bool l1fwd_mfma = true;                       // first-layer forward of the 512-wide LayerNorm/ELU shape on the matrix pipe (k_l1fwd_mfma)
  bool pipeline_updates = true;                 // rlx_ppo_update_f32: no per-update join, gathered rows double buffered
  // permutation generated ahead of the update that will consume it (rlx_ppo_prefetch_permutation)
  bool pf_valid = false;
  uint32_t pf_key_in[2] = {0, 0}, pf_key_out[2] = {0, 0};
  int pf_E = 0, pf_scheme = 0;
  int64_t pf_B = 0;
  hipEvent_t pf_done = nullptr;
  hipEvent_t ev_perm_free = nullptr;   // recorded when rlx_ppo_update_f32 has issued its last read of the permutation buffer
  bool perm_free_recorded = false;
  bool two_streams = true;                // rlx_dbg_set_option("two_streams", 0) serialises the nets again
  // Raw-observation operands of the split-fp16 kernels (the X tile of the fused first-layer backward, l1fused.hip): DEVICE word
  // holding the bit pattern of max |x| over the rows the pass reads (x_max_update, core.hip); the kernel derives a power-of-two
  // scale from it that puts max |x| at [1024, 2048) of fp16's range -- observations of any magnitude stay inside the engine's
  // window at full precision (gemm_bx.h: a FIXED x16 overflows at |x| >= 4094 and loses bits below 0.0078).  nullptr: x16.
  const uint32_t* l1_xmax = nullptr;
  const uint32_t* xmax_slot[2] = {nullptr, nullptr};   // set by the PPO update entries for their call: max |x| of the policy's / the critic's observation rows
  int lf_idle_cus = 0;                    // CUs the CU-exclusive fused first-layer backward (512 threads x 256 VGPRs) leaves to the OTHER chain's small kernels.
                                          // MEASURED at 32768-row minibatches, update period (profiles/r05_lf_idle_cus.txt): with the round-4 kernels 0 -> 448 us,
                                          // 32 -> 440, 64 -> 446; with this round's (fewer, smaller slab reductions queueing behind it) 0 -> 421, 32 -> 423, 85 -> 431
  bool dw_recompute = false;              // 1: the 512-wide first-layer activations are never stored -- k_l12fwd leaves the rows' LayerNorm statistics and the
                                          // layer-2 weight gradient rebuilds its operand (gemm_bx.hip: recomputed-operand producers).  Correct (same tests),
                                          // 134 MB less HBM traffic per network and update, and SLOWER: MEASURED update period at 32768 rows 425 -> 459 us
                                          // (4096 rows: 116 -> 126): two producer waves rebuilding 128 x 32 activations per stage are VALU-bound (~2 x the
                                          // consumers' MFMA time); off by default
  float* l12_stats = nullptr;             // set by the caller of a minibatch pass that wants that: [2][M] scratch for the statistics
  bool l12_ran = false;                   // mlp_trunk_fwd took the k_l12fwd path with the statistics (h1 was not stored)
  int l1_stats_handover = 1;              // PPO minibatch pass: 1 k_l12fwd always leaves the rows' LayerNorm mean | 1 / std ([2][M], next to h1) and the fused
                                          // first-layer backward of the same pass loads them (k_dx_l1bwd_stats) instead of rebuilding them from its
                                          // recomputed z1 -- one workgroup barrier and the sum / fold code less per row tile; 0 the earlier kernels.
                                          // Active only where both kernels are the split-operand LayerNorm forms with ln_row_once = 1 and this pass's
                                          // forward was k_l12fwd: there the two computations are the same code, so the results are bit-identical.
                                          // MEASURED (in-process A/B, 8 blocks of 5 iterations each): 65.36 vs 67.12 ms per iteration at 32768-row
                                          // minibatches (block-to-block sd 0.15 / 0.17), 107.10 vs 108.91 at 4096 rows
  int l1_wrap_refill = 1;                 // fused first-layer backward, handover form only: 1 k_dx_l1bwd_stats_wrap -- every 16-k block of the main product
                                          // refills its fragment slot unconditionally (the last two refills of a row tile fetch the first-layer image's two
                                          // blocks, which the z1 recompute then takes from registers), so no s_waitcnt vmcnt(0) is left in the K loop; 0
                                          // k_dx_l1bwd_stats.  Same operand words into the same MFMAs: bit-identical.  
  int64_t dx_l1bwd_wrap_launches = 0;     // launches of k_dx_l1bwd_stats_wrap since the context was created (the profiler row is k_dx_l1bwd's in both forms)
  int l12_prefetch = 1;                   // k_l12fwd, ln_row_once form at hidden[1] = 256 only: 1 k_l12fwd_pf -- the first-layer weight fragments of a row tile's z1
                                          // product are in registers when the tile starts (requested by the previous tile's layer-2 K loop and behind it; first
                                          // tile: at the top of the kernel), the next tile's observations are requested behind them and staged behind the K
                                          // loop, and nothing is reloaded from scratch at the tile top; 0 k_l12fwd.  Same operand words into the same MFMAs,
                                          // same stores: bit-identical.  
                                          // MEASURED (in-process A/B, 8 blocks of 5 iterations each): 62.52 vs 63.36 ms per iteration at 32768-row
                                          // minibatches (block-to-block sd 0.08 / 0.10); at 4096 rows 104.9 vs 106.2 in a drifting process (sd 0.7): not claimed
  int64_t l12fwd_pf_launches = 0;         // launches of k_l12fwd_pf since the context was created (the profiler row is k_l12fwd's in both forms)
  float* l1_hand_req = nullptr;           // set by a minibatch pass that wants the handover: [2][M] scratch k_l12fwd fills when dw_recompute does not
                                          // already make it write l12_stats (then that array serves both readers)
  const float* l1_hand[2] = {nullptr, nullptr};   // set by launch_l12fwd<ROW1>: the arrays it filled (twin: [1] the second network's); cleared with
                                          // l12_stats by the pass's scope, so a backward never reads what its own forward did not write
  bool dw_merge = true;                   // weight gradients of the two upper layers in one two-job launch when the tail kernel has produced both dZ (bx_launch_dw2)
  void* dbg_stamps = nullptr;             // test / tuning hook: device array of clock64() stamps written by instrumented kernels (fwd2h.hip)
  bool fwd2h = true;                      // 256-256 nets (SAC): the whole forward incl. the head in one launch per 32-row tile (fwd2h.hip)
  int gather_group_rows = 524288;         // whole-update calls: rows per gather launch (ppo.hip: gather_group_updates).  0 / <= minibatch: one
                                          // gather per update in rlx_ppo_update_f32's two-chain schedule only -- the twin schedule and both
                                          // data-parallel schedules have a floor of 32768 rows per launch.  MEASURED at configs[1] (in-process A/B, ms per iteration): 0: 70.95, 65536: 70.35,
                                          // 262144: 70.41, 524288 (one epoch): 70.03, 1048576: 70.00, the whole call: 70.18
  bool gather_records = true;             // whole-update calls: the rollout as aligned row records for the minibatch gathers (ppo.hip: k_pack_rows)
  bool l12_fused = true;                  // first + second layer forward in one launch when both split images are registered (k_l12fwd)
  int ppo_tail = -1;                      // PPO update: last hidden layer forward + head + loss + both input gradients in ONE launch per network (ppo.hip).
                                          // -1 (default): k_tail32_bx (32-row tiles) up to 8192 rows, k_tail_bx (64-row) above; 0 off; 1 / 2 force a form
  int tail32_waves = 8;                   // k_tail32_bx: waves per 32-row tile, 4 or 8 (same LDS: two or four waves per SIMD; bit-identical results).
                                          // MEASURED (in-process A/B, 8 blocks of 5 iterations each): 67.14 vs 68.34 ms per iteration at 32768-row
                                          // minibatches (block-to-block sd 0.19 / 0.24), 112.41 vs 115.96 at 4096 rows
  int tail32_lean = 1;                    // k_tail32_bx on eight waves: 1 runs k_tail32_bx_lean (head weights in LDS with 16 bytes of padding per eight
                                          // rows: conflict-free head reads; the serial sections on waves 4 / 5; 16-byte head-gradient partials); 0 the
                                          // earlier kernel.  No effect with tail32_waves = 4.  Every sum keeps its operands and order: bit-identical.
                                          // MEASURED (in-process A/B, 8 blocks of 5 iterations each): 60.51 vs 61.34 ms per iteration at 32768-row
                                          // minibatches (block-to-block sd 0.07 / 0.07); 102.80 vs 105.05 at 4096 rows in a drifting process (sd 0.80 /
                                          // 0.71: bar not cleared, no gain claimed there)
  int ln_row_once = 1;                    // k_dx_l1bwd<BX> / k_l12fwd: 1 every wave computes a row's LayerNorm mean and 1 / std ONCE (lanes 0-31, one row
                                          // each: ln_row_stats in l1fused.hip) and the per-row loops load them; 0 the earlier form, every lane
                                          // recomputes both for each of its 16 rows at every use.  Same operations in the same order: bit-identical.
                                          // MEASURED (in-process A/B, 8 blocks of 5 iterations each): 63.80 vs 65.65 ms per iteration at 32768-row
                                          // minibatches (block-to-block sd 0.08 / 0.13), 108.82 vs 110.85 at 4096 rows
  int ppo_twin = -1;                      // PPO update: policy || critic as twin launches (grid.y = 2) on ONE stream.  -1 (default): for
                                          // minibatches of 6144 to 16384 rows on one rank (below: two chains with grouped gathers), never with a real
                                          // RCCL communicator of more than one rank (its all-reduce would be exposed: twin_shapes_ok);
                                          // 0 never; 1 whenever the shapes allow it
  bool fused_recurrent_act = true;        // rlx_ppo_lstm_act_f32: torso + head + sampling + critic in one launch
  int num_cus = 256;
  void* defer = nullptr;                  // rlx::ReduceDefer* while a composite backward pass collects its slab reductions (mlp.h)
  bool prof_on = false;
  int prof_sample = 1;                    // instrument every prof_sample-th launch of each kernel (events cost ~2 % when every launch carries them)
  hipEvent_t prof_ref = nullptr;          // recorded at rlx_prof_begin: common time origin of all streams
  double prof_union_ms = 0.0;             // wall time during which at least one instrumented kernel was running
  std::vector<rlx::ProfRec> prof_recs;
  std::vector<rlx::ProfRow> prof_rows;
  std::vector<hipEvent_t> prof_pool;
  // hidden-layer GEMMs on the half-precision matrix pipe with split-fp32 operands (gemm_bx.h); 0 = exact-fp32 MFMA engine
  // everywhere.  Weight images are registered per scratch bank (bx_prepare_mlp / _nets / _mats).
  bool gemm_bx = true;
  float bx_gscale = 1.f;             // power-of-two scale of the gradient operands (dZ) of the pass being issued (gemm_bx.h: bx_grad_scale);
                                     // set by the update entry points for their backward passes, 1 otherwise
  // whole-update calls: the weight images of a bank's network stay registered from one minibatch pass to the next and the
  // clip + Adam kernel re-emits them from the parameters it has just written (k_bx_wfrag only runs for the first update)
  bool adam_emit = true;
  bool bx_keep[3] = {false, false, false};
  // weight images of the acting nets, valid between rlx_ppo_rollout_begin and the next parameter-changing call
  struct RoImages { bool valid = false; const float* params[2] = {nullptr, nullptr}; const void* img[2][3] = {}; int nt[2][3] = {}; } ro_img;
  int bx_force_mi = 0;               // test / tuning hook: 1 or 2 forces the 64- or 128-row block tile of the split-operand kernels
  int bx_debug = 0;                  // test hook: bit 16 / 32 / 64 / 128 keeps forward / input-gradient / weight-gradient / fused first-layer backward on the exact engine
  struct BxImage { const float* W; int trans, K, N; const void* img; };
  BxImage bx_img[3][32];   // (BX_MAX_JOBS, gemm_bx.h)
  int bx_n[3] = {0, 0, 0};
  bool disable_l1fused = false;      // test hook: fall back to k_gemm_dx + k_l1<bwd> + k_gemm_dw_skinny
  std::vector<char> ro_nets_shadow;  // host copy of the fused-rollout descriptor table
  // ---- data-parallel job (dist.hip): one process per GPU, envs sharded over the ranks
  int rank = 0, world = 1;
  void* comm = nullptr;                   // ncclComm_t (RCCL), created by rlx_ctx_create_dist when world > 1
  hipStream_t comm_stream = nullptr;      // every collective of this context is issued on this stream, in program order
  hipEvent_t comm_ev[32] = {};            // ready / done event ring (producer stream <-> comm stream)
  int comm_ev_pos = 0;
  rlx_allreduce_fn ar_hook = nullptr;     // test hook standing in for the collectives (rlx_dbg_set_allreduce_hook)
  void* ar_hook_user = nullptr;
  int ro_exit = 0;                        // tuning aid: k_rollout_step returns after a phase (option "ro_exit")
  int ro_persistent = 1;                  // rlx_ppo_rollout_f32: 1 k_rollout_steps -- ceil(T / ro_chunk_steps) launches of several acting steps each, where the
                                          // shape is inside that kernel's envelope (rollout.hip); 0 the T launches of k_rollout_step.  Bit-identical results.
  int ro_chunk_steps = 32;                // acting steps per launch of k_rollout_steps (option "rollout_chunk_steps", 1 .. 64)
  int64_t ro_persistent_launches = 0;     // launches of k_rollout_steps / of k_rollout_step since the context was created
  int64_t ro_step_launches = 0;
  const void* ro_critic_es = nullptr;     // the critic workgroups' episode-step counters of the last persistent rollout (counter "ro_critic_es_ptr")
  int64_t bx_window_fallbacks = 0;        // rollouts whose acting nets had a weight outside the fp16 window and ran on the exact engine (rollout.hip)
  int64_t ar_calls = 0;                   // all-reduces issued through dist_allreduce (communicator or hook) since the context was created
  // ---- SAC update (sac.hip): critic-loss chain on the caller's stream, policy-loss chain on `side`
  hipStream_t sac_st[2] = {nullptr, nullptr};
  hipEvent_t sac_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // SAC: the five networks' split weight images persist between calls (arena SL_WFRAG_SAC) and k_sac_optimizers rewrites them from the
  // parameters / Polyak targets it stores -- no k_bx_wfrag launch in the update, none in the acting call.  Opt-in PER CALL
  // (rlx_sac_hparams::keep_images): the caller states that the parameter vectors have only changed through rlx_sac_update_f32 since
  // its previous keep_images call; rlx_sac_invalidate_images (or any call with keep_images = 0) drops the images.
  struct SacImages {
    bool valid = false; const float *pp = nullptr, *qp = nullptr, *qt = nullptr; rlx_mlp_desc pd{}, qd{}; int64_t np = 0, nq2 = 0;
    // a library entry point other than rlx_sac_update_f32 is about to write [p, p + n): drop the images if it is one of the vectors
    void written(const float* p, int64_t n) {
      if (!valid) return;
      auto hit = [&](const float* b, int64_t m) { return b && p < b + m && b < p + n; };
      if (hit(pp, np) || hit(qp, nq2) || hit(qt, nq2)) valid = false;
    }
  } sac_img;
  const void* sac_img_arena = nullptr;
  int sac_twin = 1;                       // both critics of a pair in one launch per layer (sac.hip: twin_fwd / twin_bwd)
  float* sched_host[4] = {nullptr, nullptr, nullptr, nullptr};   // pinned staging ring of the per-update {lr, bc1, bc2} table
  hipEvent_t sched_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t sched_cap = 0;
  int sched_pos = 0;
  // ---- ESPO update (espo.hip): the device-side stop word is copied here after every chunk of epochs
  int espo_chunk = 2;                     // epochs submitted between two copies of the stop word (option "espo_chunk"); the result does not depend on it
  int32_t* espo_host = nullptr;           // pinned, one word per chunk in flight
  hipEvent_t espo_ev[3] = {nullptr, nullptr, nullptr};
  // prefetched rank-local minibatch rows (rlx_ppo_dist_prefetch)
  bool pf_dist = false;
  int pf_T = 0, pf_nl = 0, pf_ng = 0, pf_off = 0, pf_mb = 0;
};

namespace rlx {

// start / stop events of ONE instrumented launch (inactive unless rlx_prof_begin was called).  The launch itself goes
// through RLX_PLAUNCH, which hands the events to hipExtLaunchKernelGGL: they are stamped when the kernel starts and
// ends on the GPU, so the interval excludes the launch gap in front of it (events recorded around a launch do not).
struct ProfScope {
  rlx_ctx* ctx;
  hipStream_t st;
  int idx = -1;
  ProfScope(rlx_ctx* c, int kid, double flops, hipStream_t s, double bytes = 0.0, int64_t M = 0, int N = 0, int K = 0,
            int engine = 0);
  hipEvent_t ev0() const;
  hipEvent_t ev1() const;
};
// launch a kernel inside the scope of a ProfScope variable named `prof`
#define RLX_PLAUNCH(KERNEL, GRID, BLOCK, LDS, ST, ...)                                                              \
  do {                                                                                                            \
    if (prof.idx >= 0) hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, LDS, ST, prof.ev0(), prof.ev1(), 0, __VA_ARGS__); \
    else hipLaunchKernelGGL(KERNEL, GRID, BLOCK, LDS, ST, __VA_ARGS__);                                           \
  } while (0)

// ALGORITHMIC HBM bytes of a GEMM-shaped launch: every operand once (a[M,K] and b[K,N] read, c[M,N] written,
// read as well when c_rw)
inline double gemm_bytes(double M, double N, double K, int c_rw = 0) { return 4.0 * (M * K + K * N + M * N * (1 + c_rw)); }

// persistent all-zero device buffer of at least n floats (zeroed once, when it is (re)allocated)
const float* zeros_f32(rlx_ctx* ctx, size_t n);
// lazily creates ctx->side / ev_fork / ev_join (the second stream of the fused updates)
int ctx_side_stream(rlx_ctx* ctx);
int ctx_sac_streams(rlx_ctx* ctx);
// 2^-floor(log2 m) for a finite m > 0 (1 otherwise): divides a value's power-of-two magnitude out, exactly
__host__ __device__ __forceinline__ float x_pow2_inv(float m) {
  union { float f; uint32_t u; } c;
  c.f = m;
  const int e = (int)((c.u >> 23) & 0xffu);
  if (e == 0 || e == 0xff) return 1.f;
  int se = 254 - e;                                    // 2^-(e - 127)
  se = se < 27 ? 27 : (se > 227 ? 227 : se);
  c.u = (uint32_t)se << 23;
  return c.f;
}
// sets the gradient-operand scale of the split-operand kernels for the lifetime of a backward pass (gemm_bx.h: bx_grad_scale)
struct GradScaleScope {
  rlx_ctx* c;
  float prev;
  GradScaleScope(rlx_ctx* ctx, float s) : c(ctx), prev(ctx->bx_gscale) { ctx->bx_gscale = s; }
  ~GradScaleScope() { c->bx_gscale = prev; }
};
// returns nullptr (and sets error) on failure
void* scratch(rlx_ctx* ctx, ScratchSlot s, size_t bytes);
// slot[which] (SL_XMAX of bank 0, four words) <- bit pattern of max |x[0 .. n)| (two small launches on st); returns the word's
// device address through *out.  NaNs are ignored by the maximum (they reach the results through the data itself).
int x_max_update(rlx_ctx* ctx, const float* x, int64_t n, int which, hipStream_t st, const uint32_t** out);
struct XmaxScope {
  rlx_ctx* c;
  const uint32_t* prev;
  XmaxScope(rlx_ctx* ctx, const uint32_t* p) : c(ctx), prev(ctx->l1_xmax) { ctx->l1_xmax = p; }
  ~XmaxScope() { c->l1_xmax = prev; }
};
// power-of-two scale that maps max |x| (bit pattern mbits, finite and > 0; otherwise `fallback`) into [1024, 2048)
__host__ __device__ __forceinline__ float x_scale_from_max(uint32_t mbits, float fallback) {
  const int e = (int)((mbits >> 23) & 0xffu);          // biased exponent of max |x|
  if (e == 0 || e == 0xff) return fallback;            // zero / subnormal / inf / nan
  int se = 127 + 10 - (e - 127);                       // scale = 2^(10 - (e - 127))
  se = se < 27 ? 27 : (se > 227 ? 227 : se);           // keep the scale and its inverse normal: 2^-100 .. 2^100
  union { uint32_t u; float f; } c;
  c.u = (uint32_t)se << 23;
  return c.f;
}

// ------------------------------------------------------------------- MLP layout
struct LayerOff {
  int in, out;
  int64_t W, b, g, be;  // g/be = -1 when absent
};
struct MlpLayout {
  int n_hidden;
  LayerOff layer[4];
  LayerOff head;
  int64_t logstd;  // -1 when absent
  int64_t n_params;
};
inline MlpLayout make_layout(const rlx_mlp_desc& d) {
  MlpLayout L{};
  L.n_hidden = d.n_hidden;
  int64_t off = 0;
  int in = d.in_dim;
  for (int l = 0; l < d.n_hidden; ++l) {
    LayerOff& o = L.layer[l];
    o.in = in;
    o.out = d.hidden[l];
    o.W = off; off += (int64_t)in * o.out;
    o.b = off; off += o.out;
    o.g = o.be = -1;
    if (d.ln_first && l == 0) {
      o.g = off; off += o.out;
      o.be = off; off += o.out;
    }
    in = o.out;
  }
  L.head.in = in;
  L.head.out = d.out_dim;
  L.head.W = off; off += (int64_t)in * d.out_dim;
  L.head.b = off; off += d.out_dim;
  L.head.g = L.head.be = -1;
  L.logstd = -1;
  if (d.has_logstd) { L.logstd = off; off += d.out_dim; }
  L.n_params = off;
  return L;
}

// ------------------------------------------------------------- threefry (host+device)
__host__ __device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__host__ __device__ __forceinline__ void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
  const uint32_t ks0 = k0, ks1 = k1, ks2 = k0 ^ k1 ^ 0x1BD11BDAu;
  x0 += ks0; x1 += ks1;
#define RLX_TF_R(r) x0 += x1; x1 = rotl32(x1, r); x1 ^= x0;
  RLX_TF_R(13) RLX_TF_R(15) RLX_TF_R(26) RLX_TF_R(6)
  x0 += ks1; x1 += ks2 + 1u;
  RLX_TF_R(17) RLX_TF_R(29) RLX_TF_R(16) RLX_TF_R(24)
  x0 += ks2; x1 += ks0 + 2u;
  RLX_TF_R(13) RLX_TF_R(15) RLX_TF_R(26) RLX_TF_R(6)
  x0 += ks0; x1 += ks1 + 3u;
  RLX_TF_R(17) RLX_TF_R(29) RLX_TF_R(16) RLX_TF_R(24)
  x0 += ks1; x1 += ks2 + 4u;
  RLX_TF_R(13) RLX_TF_R(15) RLX_TF_R(26) RLX_TF_R(6)
  x0 += ks2; x1 += ks0 + 5u;
#undef RLX_TF_R
}

// jax `_random_bits(key, 32, [n])[i]`
__host__ __device__ __forceinline__ uint32_t random_bits_at(uint32_t k0, uint32_t k1, uint64_t i, uint64_t n,
                                                            int scheme) {
  if (scheme == RLX_THREEFRY_PARTITIONABLE) {
    uint32_t x0 = (uint32_t)(i >> 32), x1 = (uint32_t)i;
    threefry2x32(k0, k1, x0, x1);
    return x0 ^ x1;
  }
  // legacy: counts = iota(n) (zero padded to even), x0 = first half, x1 = second half
  const uint64_t h = (n + 1) / 2;
  const bool second = i >= h;
  const uint64_t j = second ? i - h : i;
  uint32_t x0 = (uint32_t)j;
  uint32_t x1 = (j + h < n) ? (uint32_t)(j + h) : 0u;
  threefry2x32(k0, k1, x0, x1);
  return second ? x1 : x0;
}

// host: jax.random.split(key, num)
inline void split_host(const uint32_t key[2], uint32_t* out, int num, int scheme) {
  if (scheme == RLX_THREEFRY_PARTITIONABLE) {
    for (int i = 0; i < num; ++i) {
      uint32_t x0 = 0, x1 = (uint32_t)i;
      threefry2x32(key[0], key[1], x0, x1);
      out[2 * i] = x0;
      out[2 * i + 1] = x1;
    }
  } else {
    const uint64_t n = 2ull * num;
    for (uint64_t i = 0; i < n; ++i) out[i] = random_bits_at(key[0], key[1], i, n, RLX_THREEFRY_LEGACY);
  }
}

// uniform [0,1) from 32 random bits (jax `uniform`, float32)
__host__ __device__ __forceinline__ float bits_to_unit(uint32_t bits) {
  union { uint32_t u; float f; } c;
  c.u = (bits >> 9) | 0x3F800000u;
  return c.f - 1.0f;
}

// XLA f32 ErfInv (M. Giles, single precision)
__device__ __forceinline__ float erfinv_f32(float x) {
  float w = -log1pf(-x * x);
  float p;
  if (w < 5.0f) {
    w = w - 2.5f;
    p = 2.81022636e-08f;
    p = 3.43273939e-07f + p * w;
    p = -3.5233877e-06f + p * w;
    p = -4.39150654e-06f + p * w;
    p = 0.00021858087f + p * w;
    p = -0.00125372503f + p * w;
    p = -0.00417768164f + p * w;
    p = 0.246640727f + p * w;
    p = 1.50140941f + p * w;
  } else {
    w = sqrtf(w) - 3.0f;
    p = -0.000200214257f;
    p = 0.000100950558f + p * w;
    p = 0.00134934322f + p * w;
    p = -0.00367342844f + p * w;
    p = 0.00573950773f + p * w;
    p = -0.0076224613f + p * w;
    p = 0.00943887047f + p * w;
    p = 1.00167406f + p * w;
    p = 2.83297682f + p * w;
  }
  return fabsf(x) == 1.0f ? copysignf(INFINITY, x) : p * x;
}

// jax.random.normal from 32 random bits
__device__ __forceinline__ float normal_from_bits(uint32_t bits) {
  const float lo = -0.99999994f;  // nextafter(-1, 0)
  float f = bits_to_unit(bits);
  float u = fmaxf(lo, f * (1.0f - lo) + lo);
  return 1.41421356237f * erfinv_f32(u);
}

// ------------------------------------------------------------------ wave helpers
// 64-lane all-reduce on the VALU only: 4 DPP steps inside each row of 16 lanes (quad_perm xor 1,
// xor 2, row_half_mirror, row_mirror), then v_permlane16_swap / v_permlane32_swap (gfx950) to fold
// the 4 rows.  No LDS crossbar (ds_bpermute / ds_swizzle) round trips: the shuffle form of this
// reduction costs ~6 dependent LDS-latency hops and dominated the LayerNorm kernels.
__device__ __forceinline__ float dpp_f(float v, const int ctrl_sel) {
  // ctrl_sel is a compile-time constant after inlining
  switch (ctrl_sel) {
    case 0: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    case 1: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    case 2: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    default: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true)); // row_mirror
  }
}
// Contiguous global -> LDS copy by the NT threads of a workgroup with up to eight loads in flight per thread.  (A plain
// `for (i = t; i < n; i += NT) dst[i] = src[i]` over a run-time count compiles to load, s_waitcnt vmcnt(0), ds_write per trip:
// one dependent L2 round trip per NT elements -- 8 us for the 35 KB first-layer kernel of the rollout step.)  Elements at or
// beyond n_valid are stored as zero.  T = float or float4 (16-byte aligned src / dst).
template <int NT, typename T>
__device__ __forceinline__ void lds_stage(T* __restrict__ dst, const T* __restrict__ src, int n, int n_valid, T zero) {
  for (int i0 = threadIdx.x; i0 < n; i0 += NT * 8) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + NT * u;
      v[u] = i < n_valid ? src[i] : zero;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + NT * u;
      if (i < n) dst[i] = v[u];
    }
  }
}
template <int NT>
__device__ __forceinline__ void lds_stage(float* __restrict__ dst, const float* __restrict__ src, int n) {
  lds_stage<NT, float>(dst, src, n, n, 0.f);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f(v, 0);
  v += dpp_f(v, 1);
  v += dpp_f(v, 2);
  v += dpp_f(v, 3);
  {
    const unsigned u = (unsigned)__float_as_int(v);
    const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = __int_as_float((int)r[0]) + __int_as_float((int)r[1]);
  }
  {
    const unsigned u = (unsigned)__float_as_int(v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    v = __int_as_float((int)r[0]) + __int_as_float((int)r[1]);
  }
  return v;
}

// FOUR half-wave sums for the price of two: lane l returns the sum over its 32-lane half of v[l & 3].  The xor-1 and
// xor-2 exchanges each halve the number of live values (a lane keeps the value its low bits select and hands the
// other one to its partner), then row_ror:8 / row_ror:4 fold the four quads of a 16-lane row (rotations keep l & 3)
// and v_permlane16_swap folds the two rows.  14 VALU instructions for 4 row sums instead of 4 x 7.
__device__ __forceinline__ float half_sum4(float v0, float v1, float v2, float v3, bool b0, bool b1) {
  const float k01 = b0 ? v1 : v0, g01 = b0 ? v0 : v1;
  const float k23 = b0 ? v3 : v2, g23 = b0 ? v2 : v3;
  const float w0 = k01 + dpp_f(g01, 0);   // v[b0] over the lane pair
  const float w1 = k23 + dpp_f(g23, 0);   // v[2 + b0]
  const float k = b1 ? w1 : w0, g = b1 ? w0 : w1;
  float x = k + dpp_f(g, 1);              // v[2 b1 + b0] over the quad
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xF, 0xF, true));   // row_ror:8
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xF, 0xF, true));   // row_ror:4
  const unsigned u = (unsigned)__float_as_int(x);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __int_as_float((int)r[0]) + __int_as_float((int)r[1]);
}

// 1 / x from v_rcp_f32 (1 ulp) and one Newton step: within half an ulp or so of the quotient in three instructions.  (__frcp_rn /
// the `/` operator expand to the ten-instruction IEEE division sequence -- v_div_scale, v_div_fmas, v_div_fixup -- which was a
// fifth of the instruction stream of the latency-bound recurrence kernels.)
__device__ __forceinline__ float rcp_fast(float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  return fmaf(fmaf(-x, r, 1.0f), r, r);
}

// ELU / tanh with ~1e-7 ABSOLUTE error (v_exp_f32 based); the 1e-5 parity bar is on losses and
// gradients, and the reference's own XLA:CPU expm1/tanh differ from libm at the same level.
__device__ __forceinline__ float expm1_fast(float z) {  // z <= 0
  const float e = __expf(z) - 1.0f;
  const float p = z * (1.0f + z * (0.5f + z * (0.16666667f + z * (0.041666668f + z * (0.0083333338f + z * (0.0013888889f + z * 0.00019841270f))))));
  return z > -0.35f ? p : e;
}
// Branch-free on purpose: both arms are evaluated on a clamped argument and merged with v_cndmask
// (a ternary around the transcendental arm becomes an exec-masked branch per element, which
// serialises the MFMA-accumulator epilogues).
template <int ACT>
__device__ __forceinline__ float act_fwd_t(float z) {
  if (ACT == RLX_ACT_TANH) {
    const float zc = fminf(fmaxf(z, -15.f), 15.f);
    const float t = 1.0f - 2.0f * rcp_fast(__expf(2.0f * zc) + 1.0f);
    const float z2 = zc * zc;
    const float p = zc * (1.0f + z2 * (-0.33333334f + z2 * (0.13333334f + z2 * (-0.053968254f + z2 * 0.021869488f))));
    return fabsf(zc) < 0.25f ? p : t;
  }
  if (ACT == RLX_ACT_ELU) {
    const float zn = fminf(z, 0.f);
    const float em = expm1_fast(zn);
    return z > 0.f ? z : em;
  }
  if (ACT == RLX_ACT_NONE) return z;
  return fmaxf(z, 0.f);
}
// derivative expressed with the PRE-activation y (kernels that recompute the forward only to get act'): ELU' is
// exp(min(y, 0)) -- one v_exp_f32, none of expm1's small-argument polynomial (elu(y) + 1 == exp(y) up to rounding)
template <int ACT>
__device__ __forceinline__ float act_grad_pre_t(float y) {
  if (ACT == RLX_ACT_TANH) {
    const float h = act_fwd_t<RLX_ACT_TANH>(y);
    return 1.f - h * h;
  }
  if (ACT == RLX_ACT_ELU) {
    const float e = __expf(fminf(y, 0.f));
    return y > 0.f ? 1.f : e;
  }
  if (ACT == RLX_ACT_NONE) return 1.f;
  return y > 0.f ? 1.f : 0.f;
}
template <int ACT>
__device__ __forceinline__ float act_grad_t(float h) {
  if (ACT == RLX_ACT_TANH) return 1.f - h * h;
  if (ACT == RLX_ACT_ELU) return h > 0.f ? 1.f : h + 1.f;
  if (ACT == RLX_ACT_NONE) return 1.f;
  return h > 0.f ? 1.f : 0.f;
}

// SiLU (torch.nn.SiLU: y * sigmoid(y)) and its derivative sigmoid(y) (1 + y (1 - sigmoid(y))), both from the pre-activation
__device__ __forceinline__ float silu_sigmoid(float y) { return rcp_fast(1.0f + __expf(-fminf(fmaxf(y, -80.f), 80.f))); }
__device__ __forceinline__ float silu_fwd(float y) { return y * silu_sigmoid(y); }
__device__ __forceinline__ float silu_grad(float y) {
  const float s = silu_sigmoid(y);
  return s * (1.0f + y * (1.0f - s));
}

__device__ __forceinline__ float act_fwd(float z, int act) {
  if (act == RLX_ACT_TANH) return act_fwd_t<RLX_ACT_TANH>(z);
  if (act == RLX_ACT_ELU) return act_fwd_t<RLX_ACT_ELU>(z);
  if (act == RLX_ACT_NONE) return z;
  if (act == RLX_ACT_SILU) return silu_fwd(z);
  return fmaxf(z, 0.f);
}
// derivative expressed with the activation OUTPUT h
__device__ __forceinline__ float act_grad_from_out(float h, int act) {
  if (act == RLX_ACT_TANH) return 1.f - h * h;
  if (act == RLX_ACT_ELU) return h > 0.f ? 1.f : h + 1.f;
  if (act == RLX_ACT_NONE) return 1.f;
  return h > 0.f ? 1.f : 0.f;
}

inline int div_up(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace rlx
