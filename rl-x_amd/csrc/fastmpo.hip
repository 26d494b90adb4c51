// fastmpo.hip -- FastMPO (rl_x/algorithms/fastmpo/flax_full_jit): MPO's E-step, M-step and dual step on one or two categorical critics
// whose target is the floor/ceil projection of the mean over K target-policy samples of the target critics' pmfs, with optax's
// clip_by_global_norm + adamw and Polyak targets for policy and critic.  One rlx_fastmpo_update_f32 call = the optimisation of one
// learning iteration (fastmpo.py:572-627): P rounds of G critic steps and one policy + dual step.
//
// Nothing here redoes a job another file does:
//   projection + cross-entropy   c51_body.h's c51_row (FastSAC's k_c51_loss is the other instantiation): k_fm_critic_loss below
//   sample + first layer of a target critic, E-step / M-step rows, dual step, gather, acting   mpo.hip's kernels (mpo_pass.h)
//   networks   net_pass.h's Chain of three blocks and a head (fm_chain lists the blocks of the three network kinds)
//   clip + adamw + Polyak   optim.hip's Adam launch (adam_body.h: clip_mode 0, weight decay, polyak_target)
// This file keeps the dataflow, the per-row noise keys and the small reduction that turns the critic step's rows into metrics.
//
// The target critics see K samples per state.  As in mpo.hip the first layer is never run on a K-fold materialised input: x W_obs
// + b is one GEMM per state row per critic, mp_sample_l1 adds clip(a) W_act and applies the block's norm and activation.  The E
// critics are served with one launch each (mpo.hip, k_mpo_sample_l1, says why).  Layers 2, 3 and the head of the K M target rows
// are GEMM stages of the library (split-operand images from 4096 rows on).  The actor's weight gradients stay on the exact engine
// (alpha ~ 1000).  Every cross-row sum is a fixed-order one-workgroup reduction: no float atomics, two identical
// calls give identical bits.  No host synchronisation inside the update.
//
// Noise (fastmpo.py:513-514, :582-584): row_keys = split(noise_key, P G B 3); critic step u, row b: normal(row_keys[(u B + b) 3],
// (K, A)); policy step: normal(row_keys[(u B + b) 3 + 2], (K, 2, A)) (the function takes two keys and draws from the second only).
// sac_sample.h's split_key_at addresses the row key.  JAX bit parity of these draws is not pinned by a fixture.
// CPU twin: tests/fastmpo_twin.py.
#include "c51_body.h"
#include "mpo_pass.h"
#include "sac_sample.h"

namespace rlx {

constexpr float FM_LN_EPS = 1e-6f;   // flax.linen.LayerNorm default
constexpr int FM_N_CRITIC_METRICS = 6, FM_N_POLICY_METRICS = 22;

// ------------------------------------------------------------------------------------------------------------- layouts
// kind 0 fastsac (policy.py:42-59, critic.py:25-43), 1 fasttd3 (policy.py:69-83, critic.py:46-61), 2 mpo (policy.py:102-117, critic.py:73-89)
static Chain fm_chain(int kind, int in, const int32_t* hidden, int out) {
  Chain L{};
  int64_t off = 0;
  L.n_hidden = 3;
  for (int l = 0; l < 3; ++l) {
    if (kind == 0) L.layer[l] = make_block(off, in, hidden[l], NORM_LAYER, RLX_ACT_SILU, FM_LN_EPS);
    else if (kind == 1) L.layer[l] = make_block(off, in, hidden[l], NORM_NONE, RLX_ACT_RELU);
    else if (l == 0) L.layer[l] = make_block(off, in, hidden[l], NORM_LAYER, RLX_ACT_TANH, FM_LN_EPS);
    else L.layer[l] = make_block(off, in, hidden[l], NORM_NONE, RLX_ACT_ELU);
    in = hidden[l];
  }
  L.head = make_block(off, in, out);
  L.n_params = off;
  return L;
}
static Chain fm_policy_layout(const rlx_fastmpo_desc& d) { return fm_chain(d.policy_kind, d.policy_obs_dim, d.policy_hidden, 2 * d.act_dim); }
static Chain fm_critic_layout(const rlx_fastmpo_desc& d) {
  return fm_chain(d.critic_kind, d.critic_obs_dim + d.act_dim, d.critic_hidden, d.nr_atoms);
}

static int fm_check_widths(int kind, const int32_t* hidden) {
  RLX_REQUIRE(kind >= 0 && kind <= 2, RLX_EINVAL, "rlx_fastmpo_desc: network kind 0 (fastsac), 1 (fasttd3) or 2 (mpo)");
  for (int l = 0; l < 3; ++l) {
    const int lim = kind == 1 || (kind == 2 && l > 0) ? 1024 : kind == 0 ? 768 : 512;
    RLX_REQUIRE(hidden[l] > 0 && hidden[l] % 64 == 0 && hidden[l] <= lim, RLX_EUNSUP,
                "rlx_fastmpo_desc: widths are multiples of 64, at most 1024 (768 behind LayerNorm + SiLU, 512 behind LayerNorm + tanh)");
  }
  return RLX_OK;
}
static int fm_check(const rlx_fastmpo_desc* d) {
  RLX_REQUIRE(d && d->policy_obs_dim > 0 && d->critic_obs_dim > 0, RLX_EINVAL, "rlx_fastmpo_desc: positive observation widths");
  RLX_REQUIRE(d->act_dim >= 1 && d->act_dim <= 64, RLX_EUNSUP, "rlx_fastmpo_desc: act_dim in 1..64 (one lane per action dimension)");
  RLX_REQUIRE(d->nr_atoms >= 2 && d->nr_atoms <= C51_MAXA, RLX_EUNSUP, "rlx_fastmpo_desc: nr_atoms in 2..128");
  RLX_REQUIRE(d->dual_critic == 0 || d->dual_critic == 1, RLX_EINVAL, "rlx_fastmpo_desc: dual_critic is 0 or 1");
  int rc = fm_check_widths(d->policy_kind, d->policy_hidden);
  if (!rc) rc = fm_check_widths(d->critic_kind, d->critic_hidden);
  return rc;
}
static int fm_check_hp(const rlx_fastmpo_desc* d, const rlx_fastmpo_hparams* hp) {
  RLX_REQUIRE(hp, RLX_EINVAL, "rlx_fastmpo_hparams: NULL");
  RLX_REQUIRE(hp->action_sampling_number >= 1 && hp->action_sampling_number <= 64, RLX_EUNSUP,
              "rlx_fastmpo_hparams: action_sampling_number in 1..64 (one lane per sample)");
  RLX_REQUIRE(hp->v_max > hp->v_min, RLX_EINVAL, "rlx_fastmpo_hparams: v_max > v_min");
  RLX_REQUIRE(hp->action_rescaling >= 0 && hp->action_rescaling <= 2, RLX_EINVAL, "rlx_fastmpo_hparams: action_rescaling 0 none, 1 normal, 2 fastsac");
  RLX_REQUIRE(!hp->clipped_double_q_learning || d->dual_critic, RLX_EINVAL,
              "rlx_fastmpo_hparams: clipped_double_q_learning needs dual_critic (default_config.py:54)");
  return RLX_OK;
}

// ------------------------------------------------------------------------------------------------------------- kernels
// The N(0, 1) draws of one step for M = H2 B stacked rows: out[(k M + r) A + j], r = h B + b, from the row's own key
// row_keys[(u B + b) 3 + which] of split(noise_key, count): element (k H2 + h) A + j of a (K, [2,] A) normal.
__global__ __launch_bounds__(256) void k_fm_noise(float* __restrict__ out, int64_t B, int K, int A, int H2, uint32_t k0, uint32_t k1,
                                                  int scheme, int64_t u, int which, uint32_t count) {
  const int64_t M = (int64_t)H2 * B, n = (int64_t)K * M * A;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e % A);
    const int64_t r = (e / A) % M;
    const int k = (int)(e / (A * M));
    const int64_t b = r % B;
    const int h = (int)(r / B);
    uint32_t s0, s1;
    split_key_at(k0, k1, (uint32_t)((u * B + b) * 3 + which), count, scheme, s0, s1);
    out[e] = normal_from_bits(random_bits_at(s0, s1, (uint64_t)(k * H2 + h) * A + j, (uint64_t)K * H2 * A, scheme));
  }
}

// FastMPO's instantiation of c51_row (fastmpo.py:314-379): E critics, the mean of K softmaxes, no entropy term; per row the loss
// (the sum over critics) and the mean / max / min over critics of the projected expectation
template <int E>
__global__ __launch_bounds__(256) void k_fm_critic_loss(C51Args a, float* __restrict__ loss_b, float* __restrict__ vmean_b,
                                                        float* __restrict__ vmax_b, float* __restrict__ vmin_b) {
  __shared__ float s_p[4][E][C51_MAXA], s_w[4][2][C51_MAXA];
  __shared__ int s_lu[4][2][C51_MAXA];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  if (b >= a.B) return;                                 // (whole waves leave: no workgroup barrier below)
  float v[E];
  const float loss = c51_row<E, true, false>(a, b, lane, s_p[w], s_w[w], s_lu[w], v);
  if (lane == 0) {
    loss_b[b] = loss;
    vmean_b[b] = E == 2 ? (v[0] + v[E - 1]) / 2.0f : v[0];
    vmax_b[b] = fmaxf(v[0], v[E - 1]);
    vmin_b[b] = fminf(v[0], v[E - 1]);
  }
}

// metrics[0..4] = {q_loss, q_mean, q_max, q_min, critic_learning_rate} (fastmpo.py:372-377, :595): batch means, one workgroup
__global__ __launch_bounds__(256) void k_fm_critic_finish(const float* __restrict__ loss_b, const float* __restrict__ vmean_b,
                                                          const float* __restrict__ vmax_b, const float* __restrict__ vmin_b, int64_t B,
                                                          float lr, float* __restrict__ metrics) {
  __shared__ float s_buf[4];
  const float invB = 1.0f / (float)B;
  const float l = mp_block_sum(loss_b, B, 1, s_buf) * invB;
  const float vm = mp_block_sum(vmean_b, B, 1, s_buf) * invB;
  const float vx = mp_block_sum(vmax_b, B, 1, s_buf) * invB;
  const float vn = mp_block_sum(vmin_b, B, 1, s_buf) * invB;
  if (threadIdx.x == 0) {
    metrics[0] = l;
    metrics[1] = vm;
    metrics[2] = vx;
    metrics[3] = vn;
    metrics[4] = lr;
  }
}

// ------------------------------------------------------------------------------------------------------------- passes
struct FmShape : MpShape { int E, Hmax; };   // Hmax: widest critic layer
static FmShape fm_shape(const rlx_fastmpo_desc& d, int O) {
  FmShape s;
  static_cast<MpShape&>(s) = mp_shape(fm_policy_layout(d), fm_critic_layout(d), O, d.policy_obs_dim, d.critic_obs_dim, d.act_dim, d.nr_atoms);
  s.E = d.dual_critic ? 2 : 1;
  s.Hmax = 0;
  for (int l = 0; l < 3; ++l) s.Hmax = s.LQ.layer[l].out > s.Hmax ? s.LQ.layer[l].out : s.Hmax;
  return s;
}

struct FmTargetBufs { float *zobs, *TH[3], *TZ, *tlog[2], *samp, *cost; };

// The E target critics on K samples of each of the M state rows xo [M, ldo] (thead: the target policy's head on the same rows):
// tlog[e] [K M, NA], samp [K M, A], cost [K M]
static int fm_target_pass(rlx_ctx* ctx, const FmShape& s, const float* tq, const float* xo, const float* thead, const float* eps, int64_t M,
                          int K, const rlx_fastmpo_hparams& hp, const FmTargetBufs& t, hipStream_t st) {
  const int64_t T = (int64_t)K * M;
  const Chain& L = s.LQ;
  int rc = RLX_OK;
  {   // split-operand images of the target critics' hidden layers 2 and 3 for the K-fold pass (from 4096 rows on)
    BxMat mats[4];
    int n = 0;
    for (int e = 0; e < s.E; ++e)
      for (int l = 1; l < 3; ++l) mats[n++] = BxMat{tq + e * L.n_params + L.layer[l].W, L.layer[l].in, L.layer[l].out, true, false};
    rc = net_images(ctx, mats, n, T, st);
    if (rc) return rc;
  }
  const MpRowMap map{T, M, 0, M, 0};
  for (int e = 0; e < s.E && !rc; ++e) {
    const float* p = tq + e * L.n_params;
    const Block& l0 = L.layer[0];
    rc = launch_gemm_fwd(ctx, xo, p + l0.W, p + l0.b, t.zobs, M, l0.out, s.Oc, RLX_ACT_NONE, st, s.ldo, nullptr);
    if (rc) break;
    rc = mp_sample_l1(thead, eps, eps, t.zobs, p + l0.W + (int64_t)s.Oc * l0.out, l0.g >= 0 ? p + l0.g : nullptr,
                      l0.be >= 0 ? p + l0.be : nullptr, t.TH[0], e == 0 ? t.samp : nullptr, e == 0 ? t.cost : nullptr, map, T, s.A, l0.out,
                      hp.policy_min_scale, hp.policy_init_scale, hp.action_clipping, l0.norm, l0.act, l0.eps, st);
    for (int l = 1; l < 3 && !rc; ++l) rc = block_fwd(ctx, L.layer[l], p, t.TH[l - 1], L.layer[l].in, t.TZ, t.TH[l], T, st);
    if (!rc) rc = fs_head_fwd(t.TH[2], p + L.head.W, p + L.head.b, t.tlog[e], T, L.head.in, s.NA, st);
  }
  bx_release_all(ctx);
  return rc;
}

static int fm_noise(float* out, int64_t B, int K, int A, int H2, const uint32_t key[2], int scheme, int64_t u, int which, uint32_t count,
                    hipStream_t st) {
  hipLaunchKernelGGL(k_fm_noise, dim3(elem_grid((int64_t)K * H2 * B * A)), dim3(256), 0, st, out, B, K, A, H2, key[0], key[1], scheme, u,
                     which, count);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int64_t rlx_fastmpo_param_count(const rlx_fastmpo_desc* d, int net) {
  if (!d || net < 0 || net > 2 || d->act_dim <= 0 || d->policy_obs_dim <= 0 || d->critic_obs_dim <= 0 || d->nr_atoms <= 0) return -1;
  if (net == 2) return 2 * (int64_t)d->act_dim + 2;
  for (int l = 0; l < 3; ++l)
    if (d->policy_hidden[l] <= 0 || d->critic_hidden[l] <= 0) return -1;
  if (d->policy_kind < 0 || d->policy_kind > 2 || d->critic_kind < 0 || d->critic_kind > 2) return -1;
  return net == 0 ? fm_policy_layout(*d).n_params : fm_critic_layout(*d).n_params;
}

int rlx_fastmpo_act_f32(rlx_ctx* ctx, const rlx_fastmpo_desc* desc, const float* pparams, const float* obs, int O, const int32_t* pidx,
                        uint32_t key_io[2], int scheme, float* action, float* processed_action, const float* low, const float* high,
                        int64_t N, int deterministic, const rlx_fastmpo_hparams* hp, void* stream) {
  RLX_REQUIRE(ctx && pparams && obs && key_io && action && processed_action && N > 0 && O > 0, RLX_EINVAL, "rlx_fastmpo_act_f32: bad args");
  int rc = fm_check(desc);
  if (!rc) rc = fm_check_hp(desc, hp);
  if (rc) return rc;
  RLX_REQUIRE(hp->action_rescaling != 1 || (low && high), RLX_EINVAL, "rlx_fastmpo_act_f32: action_rescaling normal needs low and high");
  RLX_REQUIRE(hp->action_rescaling != 2 || low, RLX_EINVAL, "rlx_fastmpo_act_f32: action_rescaling fastsac needs the action scale (in low)");
  RLX_REQUIRE(pidx || desc->policy_obs_dim == O, RLX_EINVAL, "rlx_fastmpo_act_f32: policy_obs_dim != O needs pidx");
  return mp_act_pass(ctx, fm_policy_layout(*desc), pparams, obs, O, pidx, key_io, scheme, action, processed_action, low, high, N, deterministic,
                     hp->policy_min_scale, hp->policy_init_scale, hp->action_clipping, hp->action_rescaling, (hipStream_t)stream);
}

int rlx_fastmpo_update_f32(rlx_ctx* ctx, const rlx_fastmpo_desc* desc, float* pparams, float* pm, float* pv, float* target_pparams,
                           float* qparams, float* qm, float* qv, float* target_qparams, float* duals, float* dm, float* dv,
                           const float* states, const float* next_states, int O, const int32_t* pidx, const int32_t* cidx,
                           const float* actions, const float* rewards, const float* dones, const float* truncations,
                           const float* effective_n_steps, int64_t B, const uint32_t noise_key[2], int scheme, int64_t* opt_count_io,
                           const float* critic_lr, const float* policy_lr, const float* dual_lr, const rlx_fastmpo_hparams* hp,
                           float* metrics_out, void* stream) {
  RLX_REQUIRE(ctx && pparams && pm && pv && target_pparams && qparams && qm && qv && target_qparams && duals && dm && dv && states &&
                  next_states && actions && rewards && dones && truncations && effective_n_steps && noise_key && opt_count_io &&
                  critic_lr && policy_lr && dual_lr && metrics_out && B > 0 && O > 0,
              RLX_EINVAL, "rlx_fastmpo_update_f32: bad args");
  int rc = fm_check(desc);
  if (!rc) rc = fm_check_hp(desc, hp);
  if (rc) return rc;
  const int P = hp->nr_policy_updates_per_step, G = hp->nr_critic_updates_per_policy_update;
  RLX_REQUIRE(P >= 1 && G >= 1, RLX_EINVAL, "rlx_fastmpo_update_f32: at least one policy round and one critic step per round");
  RLX_REQUIRE((int64_t)P * G * B * 3 < (int64_t)1 << 31, RLX_EUNSUP, "rlx_fastmpo_update_f32: P G B 3 row keys must fit 31 bits");
  RLX_REQUIRE(opt_count_io[0] >= 0 && opt_count_io[1] >= 0 && opt_count_io[2] >= 0, RLX_EINVAL, "rlx_fastmpo_update_f32: optimiser counts >= 0");
  RLX_REQUIRE((pidx || desc->policy_obs_dim == O) && (cidx || desc->critic_obs_dim == O), RLX_EINVAL,
              "rlx_fastmpo_update_f32: an observation width != O needs its column indices");
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  BxReleaseAll bx_rel{ctx};
  const FmShape s = fm_shape(*desc, O);
  const int A = s.A, NA = s.NA, E = s.E, K = hp->action_sampling_number;
  const int64_t R = 2 * B, T = (int64_t)K * R, nq = s.LQ.n_params, np = s.LP.n_params;
  const uint32_t key_count = (uint32_t)((int64_t)P * G * B * 3);
  // ---- arena (sized for the policy step's R = 2B state rows; the critic steps use the first B / K B rows)
  FmTargetBufs tb;
  float *xs, *xo, *xc, *thead, *ohead, *dhead, *eps, *qlog[2], *dqlog[2], *rowv[4], *gq, *gp;
  ChainBufs btp, bp, bq[2];
  MpRowOut ro;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    for (int l = 0; l < 3; ++l) tb.TH[l] = a.take((size_t)T * s.LQ.layer[l].out);
    tb.TZ = a.take((size_t)T * s.Hmax);
    for (int e = 0; e < 2; ++e) tb.tlog[e] = e < E ? a.take((size_t)T * NA) : nullptr;
    tb.samp = a.take((size_t)T * A);
    tb.cost = a.take(T);
    tb.zobs = a.take((size_t)R * s.LQ.layer[0].out);
    chain_carve(s.LP, R, a, &btp);
    chain_carve(s.LP, R, a, &bp);
    for (int e = 0; e < E; ++e) chain_carve(s.LQ, B, a, &bq[e]);
    xs = a.take((size_t)R * s.ldp);
    xo = a.take((size_t)R * s.ldo);
    xc = a.take((size_t)B * s.ldc);
    for (float** x : {&thead, &ohead, &dhead}) *x = a.take((size_t)R * 2 * A);
    eps = a.take((size_t)T * A);
    for (int e = 0; e < 2; ++e) {
      qlog[e] = e < E ? a.take((size_t)B * NA) : nullptr;
      dqlog[e] = e < E ? a.take((size_t)B * NA) : nullptr;
    }
    for (float*& x : rowv) x = a.take(B);
    for (float** x : {&ro.lse_q, &ro.e_q, &ro.lse_p, &ro.e_p, &ro.pgm, &ro.pgs, &ro.smin, &ro.smax, &ro.qmean}) *x = a.take(R);
    ro.klm = a.take((size_t)R * A);
    ro.kls = a.take((size_t)R * A);
    gq = a.take((size_t)E * nq);
    gp = a.take(np);
  });
  if (rc) return rc;
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (!sq) return RLX_ENOMEM;
  // the optimiser counts go back to the caller only when the whole call was submitted
  int64_t counts[3] = {opt_count_io[0], opt_count_io[1], opt_count_io[2]};
  const float max_norm = hp->max_grad_norm > 0.f ? hp->max_grad_norm : -1.f;
  float* m_critic = metrics_out;
  float* m_policy = metrics_out + FM_N_CRITIC_METRICS;
  for (int p = 0; p < P; ++p) {
    int64_t u = 0;
    for (int gi = 0; gi < G; ++gi) {
      u = (int64_t)p * G + gi;
      const float* s_u = states + u * B * O;
      const float* s2_u = next_states + u * B * O;
      // ---- critic step u (fastmpo.py:314-379, :586-596): target policy and target critics on s'
      rc = mp_gather(s2_u, s2_u, B, O, pidx, s.Op, nullptr, 0, 0, xs, s.ldp, B, st);
      if (!rc) rc = mp_gather(s2_u, s2_u, B, O, cidx, s.Oc, nullptr, 0, 0, xo, s.ldo, B, st);
      if (!rc) rc = mp_gather(s_u, s_u, B, O, cidx, s.Oc, actions + u * B * A, A, hp->action_clipping, xc, s.ldc, B, st);
      if (!rc) rc = chain_fwd(ctx, s.LP, target_pparams, xs, s.ldp, btp, thead, B, st);
      if (rc) return rc;
      const float* ec = ctx->dbg_sac_eps[0] ? ctx->dbg_sac_eps[0] + u * K * B * A : nullptr;
      if (!ec) {
        rc = fm_noise(eps, B, K, A, 1, noise_key, scheme, u, 0, key_count, st);
        if (rc) return rc;
        ec = eps;
      }
      rc = fm_target_pass(ctx, s, target_qparams, xo, thead, ec, B, K, *hp, tb, st);
      for (int e = 0; e < E && !rc; ++e) rc = chain_fwd(ctx, s.LQ, qparams + e * nq, xc, s.ldc, bq[e], qlog[e], B, st);
      if (rc) return rc;
      C51Args ca{};
      for (int e = 0; e < E; ++e) {
        ca.q[e] = qlog[e];
        ca.qn[e] = tb.tlog[e];
        ca.dq[e] = dqlog[e];
      }
      ca.rew = rewards + u * B; ca.dones = dones + u * B; ca.truncs = truncations + u * B; ca.nsteps = effective_n_steps + u * B;
      ca.B = B; ca.NA = NA; ca.K = K; ca.gamma = hp->gamma; ca.v_min = hp->v_min; ca.v_max = hp->v_max;
      ca.clipped = E == 2 && hp->clipped_double_q_learning; ca.tie_first = 1;
      if (E == 2) hipLaunchKernelGGL(k_fm_critic_loss<2>, dim3(div_up(B, 4)), dim3(256), 0, st, ca, rowv[0], rowv[1], rowv[2], rowv[3]);
      else hipLaunchKernelGGL(k_fm_critic_loss<1>, dim3(div_up(B, 4)), dim3(256), 0, st, ca, rowv[0], rowv[1], rowv[2], rowv[3]);
      RLX_LAUNCH_CHECK();
      {
        BwdPass bwd(ctx, B);
        rc = bwd.begin((size_t)E * chain_stage_floats(ctx, s.LQ, B, true));
        for (int e = 0; e < E && !rc; ++e)
          rc = chain_bwd(ctx, s.LQ, qparams + e * nq, xc, s.ldc, bq[e], dqlog[e], gq + e * nq, nullptr, 0, B, st);
        if (!rc) rc = bwd.finish(st);
        if (rc) return rc;
      }
      hipLaunchKernelGGL(k_fm_critic_finish, dim3(1), dim3(256), 0, st, (const float*)rowv[0], (const float*)rowv[1], (const float*)rowv[2],
                         (const float*)rowv[3], B, critic_lr[u], m_critic);
      RLX_LAUNCH_CHECK();
      {   // clip_by_global_norm + adamw over both critics, their Polyak update in the same launch
        const int nsq = launch_sumsq_partials(gq, E * nq, sq, st);
        RLX_LAUNCH_CHECK();
        rc = launch_clip_adam(qparams, gq, qm, qv, E * nq, sq, nsq, ++counts[0], critic_lr[u], max_norm, hp->adam_b1, hp->adam_b2,
                              hp->adam_eps, m_critic + 5, st, nullptr, nullptr, target_qparams, hp->critic_tau, hp->critic_weight_decay, 0);
        if (rc) return rc;
      }
    }
    // ---- policy and dual step on the round's last batch (fastmpo.py:381-482, :600-627): target nets on [s; s']
    const float* s_u = states + u * B * O;
    const float* s2_u = next_states + u * B * O;
    rc = mp_gather(s_u, s2_u, B, O, pidx, s.Op, nullptr, 0, 0, xs, s.ldp, R, st);
    if (!rc) rc = mp_gather(s_u, s2_u, B, O, cidx, s.Oc, nullptr, 0, 0, xo, s.ldo, R, st);
    if (!rc) rc = chain_fwd(ctx, s.LP, target_pparams, xs, s.ldp, btp, thead, R, st);
    if (rc) return rc;
    const float* ea = ctx->dbg_sac_eps[1] ? ctx->dbg_sac_eps[1] + (int64_t)p * K * R * A : nullptr;
    if (!ea) {
      rc = fm_noise(eps, B, K, A, 2, noise_key, scheme, u, 2, key_count, st);
      if (rc) return rc;
      ea = eps;
    }
    rc = fm_target_pass(ctx, s, target_qparams, xo, thead, ea, R, K, *hp, tb, st);
    if (!rc) rc = chain_fwd(ctx, s.LP, pparams, xs, s.ldp, bp, ohead, R, st);
    if (rc) return rc;
    {
      MpEstepArgs es{};
      es.tlogits[0] = tb.tlog[0]; es.tlogits[1] = tb.tlog[1]; es.E = E; es.qmin = hp->clipped_double_q_learning; es.alpha_mean_off = 1;
      es.cost = tb.cost; es.samp = tb.samp; es.thead = thead; es.ohead = ohead; es.duals = duals;
      es.R = R; es.S = K; es.A = A; es.NA = NA; es.v_min = hp->v_min; es.v_max = hp->v_max;
      es.min_scale = hp->policy_min_scale; es.init_scale = hp->policy_init_scale; es.feps = hp->float_epsilon; es.clip = hp->action_clipping;
      rc = mp_estep(es, dhead, ro, st);
      if (rc) return rc;
    }
    {
      // the actor's weight gradients stay on the exact fp32 engine: its head gradient carries alpha (mu - mu_t) / sigma_t^2 with
      // alpha ~ 1000 at the default init_log_alpha_stddev, which can leave the split engine's fp16 range (mpo.hip)
      ExactDwScope exact(ctx);
      FsDefer defer(ctx);
      rc = defer.begin(chain_stage_floats(ctx, s.LP, R, true));
      if (!rc) rc = chain_bwd(ctx, s.LP, pparams, xs, s.ldp, bp, dhead, gp, nullptr, 0, R, st);
      if (!rc) rc = defer.finish(st);
      if (rc) return rc;
    }
    {
      const int nsq = launch_sumsq_partials(gp, np, sq, st);
      RLX_LAUNCH_CHECK();
      rc = launch_clip_adam(pparams, gp, pm, pv, np, sq, nsq, ++counts[1], policy_lr[p], max_norm, hp->adam_b1, hp->adam_b2, hp->adam_eps,
                            m_policy + 20, st, nullptr, nullptr, target_pparams, hp->policy_tau, hp->policy_weight_decay, 0);
      if (rc) return rc;
    }
    MpDualArgs c;
    const int64_t dstep = ++counts[2];
    c.eps_np = hp->epsilon_non_parametric; c.eps_mu = hp->epsilon_parametric_mu; c.eps_sigma = hp->epsilon_parametric_sigma;
    c.eps_pen = hp->epsilon_penalty; c.feps = hp->float_epsilon; c.log_s = logf((float)K); c.max_norm = hp->max_grad_norm; c.lr = dual_lr[p];
    c.b1 = hp->adam_b1; c.b2 = hp->adam_b2; c.adam_eps = hp->adam_eps;
    c.bc1 = (float)(1.0 - std::pow((double)hp->adam_b1, (double)dstep));
    c.bc2 = (float)(1.0 - std::pow((double)hp->adam_b2, (double)dstep));
    c.min_log_temp = hp->min_log_temperature; c.min_log_alpha = hp->min_log_alpha; c.clip = hp->action_clipping;
    c.variant = 1; c.wd = hp->dual_weight_decay; c.lr_policy = policy_lr[p];
    rc = mp_dual(nullptr, nullptr, B, ro, R, A, duals, dm, dv, c, m_policy, st);
    if (rc) return rc;
  }
  for (int i = 0; i < 3; ++i) opt_count_io[i] = counts[i];
  return RLX_OK;
}

}  // extern "C"
