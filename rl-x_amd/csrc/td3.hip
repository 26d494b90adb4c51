// td3.hip -- TD3 and DDPG, the two deterministic-policy-gradient algorithms (rl_x/algorithms/td3/flax/td3.py:106-205,
// rl_x/algorithms/ddpg/flax/ddpg.py:104-166): a tanh policy without a log-std (td3/flax/policy.py:22-44) WITH a target copy, and two
// scalar ReLU critics (td3/flax/critic.py:17-53; DDPG: one, ddpg/flax/critic.py) on [critic obs | action].  What differs from
// sac.hip and the ensemble family:
//   acting      key, sub = split(key); a = clip(tanh(pi(s)) + epsilon normal(sub, (N, A)), -1, 1): ONE shape-wide draw (td3.py:107-112)
//   critic step keys = split(key, B + 1), key = keys[0], row i draws normal(keys[1 + i], (A,)) (:149-150, :126);
//               a' = clip(tanh(pi_target(s')) + clip(smoothing_epsilon n, +-smoothing_clip_value), -1, 1) (:125-128);
//               y = r + gamma (1 - term) min_e Q_target,e(s', a') (:130-132); loss = mean over batch AND critics of (q_e - y)^2
//               (:134, safe_mean at :145): d loss / d q_e = 2 (q_e - y) / (E B); plain Adam, no clipping (:156)
//   policy step loss = mean(-min_e Q_e(s, pi(s))) against the critics AFTER this call's critic step (:167-172): the reference's
//               variant, the min over both critics and not Q_1; jnp.min splits its gradient evenly among exact ties; plain Adam,
//               then Polyak of BOTH the critics and the policy (:190-194).  hp->policy_step = 0: critic step only, the targets stay
//   counters    two optax counts: a delayed policy step leaves the policy's behind the critics' (:72-79, :88, :95)
//   DDPG        hp->joint: one critic, no smoothing noise and no key; one joint loss whose policy gradient flows through the critic
//               BEFORE its step (stop_gradient(critic_params), ddpg.py:129-131); both Adam steps, then both Polyak steps (:155-160)
//
// Networks: rlx_mlp_desc as the ensemble family takes them (ReLU, no LayerNorm; sac_ens.h: ens_check_net), the policy with out_dim =
// act_dim (sac_ens.h: det_prologue).  A network is net_pass.h's Chain; passes of >= 4096 rows take the split-operand images
// (trunk_images), rebuilt in front of the policy step from the critics the critic step left.  Q values are laid out [E][B].
//
// Schedule of one call (no host synchronisation; the two critics' chains on two streams, fs_sched.h: FsFork, as fasttd3.hip runs
// its pair): critic step: online critics on (s, a) on the side stream || target policy on s' -> k_dpg_target_action -> target
// critics on (s', a'); k_dpg_critic_loss; one backward per stream under ONE deferred reduction; Adam of the critics (with the
// Polyak step when a policy step follows).  Policy step: policy on s -> k_dpg_target_action without noise -> one critic per stream
// on (s, pi(s)) -> k_dpg_policy_seed -> one input-gradient pass per stream -> k_td3_tanh_bwd -> the policy's backward, one deferred
// reduction; k_dpg_finish (the loss sums); Adam of the policy with its Polyak step.  With hp->joint the critics' Adam moves behind
// the policy's backward.  Every reduction runs in a fixed order without atomics: two identical calls give identical bits.
// CPU twin: tests/td3_twin.py (float64).  The reference's TD3 and DDPG are JAX only; see DESIGN.md 4.5 for what is pinned.
#include "dpg.h"
#include "sac_ens.h"

namespace rlx {

constexpr int DPG_MAXE = 2;

// ---------------------------------------------------------------------------------------------------------------- kernels
// sum of one double per thread over the workgroup: fixed tree, no atomics; every thread calls it
__device__ __forceinline__ double dpg_block_sum(double s, double* s_buf) {
  s_buf[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_buf[threadIdx.x] += s_buf[threadIdx.x + o];
    __syncthreads();
  }
  const double r = s_buf[0];
  __syncthreads();
  return r;
}

// Acting (td3.py:107-112, policy.py:39-44) from the policy's head output [N, A]: a = tanh(head); epsilon != 0: a = clip(a + epsilon
// normal(bits(sub, i A + j of N A)), -1, 1) -- the shape-wide draw; action = a (what the ring stores), processed = low + 0.5
// (clip(a, -1, 1) + 1)(high - low) (what the env gets)
__global__ __launch_bounds__(256) void k_dpg_act(const float* __restrict__ head, int64_t N, int A, float epsilon, uint32_t k0, uint32_t k1,
                                                 int scheme, const float* __restrict__ eps_inject, float* __restrict__ action,
                                                 float* __restrict__ processed, const float* __restrict__ low,
                                                 const float* __restrict__ high) {
  const int64_t n = N * A;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e % A);
    float a = tanhf(head[e]);
    if (epsilon != 0.f) {
      const float eps = eps_inject ? eps_inject[e] : normal_from_bits(random_bits_at(k0, k1, (uint64_t)e, (uint64_t)n, scheme));
      a = fminf(fmaxf(a + epsilon * eps, -1.0f), 1.0f);
    }
    action[e] = a;
    processed[e] = low[j] + 0.5f * (fminf(fmaxf(a, -1.0f), 1.0f) + 1.0f) * (high[j] - low[j]);
  }
}

// From a policy's head output [B, A] to the action columns [c0, c0 + A) of the critics' input rows (row stride ld), nothing in
// between reaching memory.  noise: the target action (td3.py:125-128) a' = clip(tanh(head) + clip(smooth_eps n, +-smooth_clip), -1,
// 1), n = eps_inject[i, j] (test hook) or normal(bits(split(key, count)[base + stride i], j of A)) -- the row's own key; without:
// a = tanh(head) (the policy step's action; DDPG's target action).  AP threads share a row, each derives the row's key once.
__global__ __launch_bounds__(256) void k_dpg_target_action(const float* __restrict__ head, float* __restrict__ x, int ld, int c0, int64_t B,
                                                           int A, int AP, int noise, EnsRowKeys keys, float smooth_eps, float smooth_clip,
                                                           const float* __restrict__ eps_inject) {
  const int rpb = 256 / AP;
  const int rl = threadIdx.x / AP, jl = threadIdx.x - rl * AP;
  const int64_t i = (int64_t)blockIdx.x * rpb + rl;
  if (i >= B) return;
  uint32_t s0 = 0, s1 = 0;
  if (noise && !eps_inject) split_key_at(keys.k0, keys.k1, keys.base + keys.stride * (uint32_t)i, keys.count, keys.scheme, s0, s1);
  for (int j = jl; j < A; j += AP) {
    float a = tanhf(head[i * A + j]);
    if (noise) {
      const float n = eps_inject ? eps_inject[i * A + j] : normal_from_bits(random_bits_at(s0, s1, (uint64_t)j, (uint64_t)A, keys.scheme));
      const float nz = fminf(fmaxf(n * smooth_eps, -smooth_clip), smooth_clip);
      a = fminf(fmaxf(a + nz, -1.0f), 1.0f);
    }
    x[i * ld + c0 + j] = a;
  }
}

// One thread per transition (td3.py:130-134): y_b = r_b + gamma (1 - term_b) min_e qn[e, b] over the E <= 2 targets; dq[e, b] =
// 2 (q[e, b] - y_b) / (E B); partial[block] = sum over the block's rows and the critics of (q - y)^2, in double.  y may be NULL.
__global__ __launch_bounds__(256) void k_dpg_critic_loss(const float* __restrict__ q, const float* __restrict__ qn, const float* __restrict__ rew,
                                                         const float* __restrict__ term, float* __restrict__ y, float* __restrict__ dq,
                                                         double* __restrict__ partial, int64_t B, int E, float gamma) {
  __shared__ double s_buf[256];
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double loss = 0.0;
  if (b < B) {
    float mn = qn[b];
    for (int e = 1; e < E; ++e) mn = fminf(mn, qn[(int64_t)e * B + b]);
    const float yb = rew[b] + gamma * (1.0f - term[b]) * mn;
    if (y) y[b] = yb;
    const float gs = 2.0f / ((float)B * (float)E);
    for (int e = 0; e < E; ++e) {
      const float d = q[(int64_t)e * B + b] - yb;
      dq[(int64_t)e * B + b] = gs * d;
      loss += (double)d * (double)d;
    }
  }
  const double s = dpg_block_sum(loss, s_buf);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One thread per transition (td3.py:170-172): mn = min_e qa[e, b]; seed[e, b] = d mean_b(-min_e) / d qa[e, b] = -[qa[e, b] == mn] /
// (B n_ties), the even split jnp.min's gradient takes among exact ties; partial[block] = sum of mn over the block's rows, in double
// (policy_loss = -q_value = -sum / B)
__global__ __launch_bounds__(256) void k_dpg_policy_seed(const float* __restrict__ qa, float* __restrict__ seed, double* __restrict__ partial,
                                                         int64_t B, int E) {
  __shared__ double s_buf[256];
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double v = 0.0;
  if (b < B) {
    float mn = qa[b];
    for (int e = 1; e < E; ++e) mn = fminf(mn, qa[(int64_t)e * B + b]);
    int ties = 0;
    for (int e = 0; e < E; ++e) ties += qa[(int64_t)e * B + b] == mn ? 1 : 0;
    const float s = -1.0f / ((float)B * (float)(ties > 0 ? ties : 1));
    for (int e = 0; e < E; ++e) seed[(int64_t)e * B + b] = qa[(int64_t)e * B + b] == mn ? s : 0.f;
    v = (double)mn;
  }
  const double s = dpg_block_sum(v, s_buf);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the block partials of the two losses, added in index order: out_q[0] = sum(part_q) / div_q (q_loss); out_p[0] = -mean, out_p[1] =
// mean of part_p over div_p (policy_loss, q_value).  Either pair may be absent (NULL).
__global__ __launch_bounds__(256) void k_dpg_finish(const double* __restrict__ part_q, int n_q, double div_q, float* __restrict__ out_q,
                                                    const double* __restrict__ part_p, int n_p, double div_p, float* __restrict__ out_p) {
  __shared__ double s_buf[256];
  if (part_q) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n_q; i += 256) s += part_q[i];
    s = dpg_block_sum(s, s_buf);
    if (threadIdx.x == 0) out_q[0] = (float)(s / div_q);
  }
  if (part_p) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n_p; i += 256) s += part_p[i];
    s = dpg_block_sum(s, s_buf);
    if (threadIdx.x == 0) {
      const float mean_q = (float)(s / div_p);
      out_p[0] = -mean_q;
      out_p[1] = mean_q;
    }
  }
}

// dpg.h: (da1 + da2) (1 - a^2), shared with fasttd3.hip
__global__ __launch_bounds__(256) void k_td3_tanh_bwd(const float* __restrict__ x, const float* __restrict__ da1, const float* __restrict__ da2,
                                                      int lda, int c0, float* __restrict__ dhead, int64_t M, int A) {
  const int64_t n = M * A;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / A;
    const int j = (int)(e - i * A);
    const float a = x[i * lda + c0 + j];
    const float da = da2 ? da1[i * lda + c0 + j] + da2[i * lda + c0 + j] : da1[i * lda + c0 + j];
    dhead[e] = da * (1.0f - a * a);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
int dpg_tanh_bwd(const float* x, const float* da1, const float* da2, int lda, int c0, float* dhead, int64_t M, int A, hipStream_t st) {
  hipLaunchKernelGGL(k_td3_tanh_bwd, dim3(elem_grid(M * A)), dim3(256), 0, st, x, da1, da2, lda, c0, dhead, M, A);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

static int dpg_target_action(const float* head, float* x, int ld, int c0, int64_t B, int A, bool noise, const EnsRowKeys& keys,
                             float smooth_eps, float smooth_clip, const float* eps_inject, hipStream_t st) {
  const int AP = ens_lanes_per_row(A);
  hipLaunchKernelGGL(k_dpg_target_action, dim3(div_up(B, 256 / AP)), dim3(256), 0, st, head, x, ld, c0, B, A, AP, noise ? 1 : 0, keys,
                     smooth_eps, smooth_clip, noise ? eps_inject : nullptr);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

static int dpg_check_hp(const rlx_td3_hparams& hp, const std::string& f) {
  RLX_REQUIRE(hp.nr_critics == 1 || hp.nr_critics == 2, RLX_EUNSUP, f + ": hp->nr_critics must be 1 or 2");
  RLX_REQUIRE(!hp.joint || (hp.nr_critics == 1 && hp.smoothing_epsilon == 0.f), RLX_EINVAL,
              f + ": hp->joint needs nr_critics == 1 and smoothing_epsilon == 0");
  RLX_REQUIRE(!hp.joint || hp.policy_step, RLX_EINVAL, f + ": hp->joint needs policy_step (the joint loss has both steps)");
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int rlx_td3_act_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, const float* pparams, const float* obs, uint32_t key_io[2], int scheme,
                    float epsilon, float* action, float* processed_action, int N, const float* low, const float* high, void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && obs && key_io && action && processed_action && low && high, RLX_EINVAL,
              "rlx_td3_act_f32: NULL pointer");
  RLX_REQUIRE(N > 0, RLX_EINVAL, "rlx_td3_act_f32: N must be positive");
  int rc = ens_check_net(*pdesc, "td3", "pdesc");
  if (rc) return rc;
  RLX_REQUIRE(pdesc->out_dim >= 1 && pdesc->out_dim <= 64, RLX_EUNSUP, "rlx_td3_act_f32: act_dim (pdesc->out_dim) must be in 1..64");
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain L = ens_layout(*pdesc);
  const int A = pdesc->out_dim, ldp = (pdesc->in_dim + 3) & ~3;
  ChainBufs b;
  float *xs, *h;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(L, N, a, &b);
    xs = a.take((size_t)N * ldp);
    h = a.take((size_t)N * A);
  });
  if (rc) return rc;
  rc = fs_concat(obs, pdesc->in_dim, nullptr, 0, xs, ldp, N, st);
  if (!rc) rc = chain_fwd(ctx, L, pparams, xs, ldp, b, h, N, st);
  if (rc) return rc;
  uint32_t ks[2] = {0, 0};
  if (epsilon != 0.f) next_key(key_io, ks, 1, scheme);      // key, subkey = split(key) (td3.py:108); evaluation leaves the key alone
  hipLaunchKernelGGL(k_dpg_act, dim3(elem_grid((int64_t)N * A)), dim3(256), 0, st, (const float*)h, (int64_t)N, A, epsilon, ks[0], ks[1], scheme,
                     ctx->dbg_sac_eps[0], action, processed_action, low, high);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int rlx_td3_losses_f32(rlx_ctx* ctx, const float* q, const float* q_next, const float* rewards, const float* terminations, int64_t B,
                       const rlx_td3_hparams* hp, float* y_out, float* dq_out, float* loss_out, void* stream) {
  RLX_REQUIRE(ctx && hp, RLX_EINVAL, "rlx_td3_losses_f32: ctx / hp is NULL");
  RLX_REQUIRE(q && q_next && rewards && terminations && dq_out && loss_out, RLX_EINVAL,
              "rlx_td3_losses_f32: NULL pointer (q, q_next, rewards, terminations, dq_out, loss_out)");
  RLX_REQUIRE(B > 0, RLX_EINVAL, "rlx_td3_losses_f32: B must be positive");
  RLX_REQUIRE(hp->nr_critics == 1 || hp->nr_critics == 2, RLX_EUNSUP, "rlx_td3_losses_f32: hp->nr_critics must be 1 or 2");
  hipStream_t st = (hipStream_t)stream;
  const int E = hp->nr_critics, nblk = div_up(B, 256);
  double* part = (double*)scratch(ctx, SL_STAGE, (size_t)nblk * sizeof(double));
  if (!part) return RLX_ENOMEM;
  hipLaunchKernelGGL(k_dpg_critic_loss, dim3(nblk), dim3(256), 0, st, q, q_next, rewards, terminations, y_out, dq_out, part, B, E, hp->gamma);
  RLX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_dpg_finish, dim3(1), dim3(256), 0, st, (const double*)part, nblk, (double)B * E, loss_out, (const double*)nullptr, 0, 1.0,
                     (float*)nullptr);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int rlx_td3_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, float* ptarget,
                       const rlx_mlp_desc* qdesc, float* qparams, float* qm, float* qv, float* qtarget, const float* states,
                       const float* next_states, const float* actions, const float* rewards, const float* terminations, int64_t B,
                       uint32_t key_io[2], int scheme, int64_t* q_opt_count_io, int64_t* pi_opt_count_io, const rlx_td3_hparams* hp,
                       float* metrics_out, void* stream) {
  const char* fn = "rlx_td3_update_f32";
  const std::string f(fn);
  RLX_REQUIRE(ctx && pdesc && pparams && pm && pv && ptarget && qdesc && qparams && qm && qv && qtarget && states && next_states && actions &&
                  rewards && terminations && key_io && q_opt_count_io && pi_opt_count_io && hp && metrics_out,
              RLX_EINVAL, f + ": NULL pointer");
  RLX_REQUIRE(B > 0, RLX_EINVAL, f + ": B must be positive");
  RLX_REQUIRE(B <= 0x7fffffffLL - 1, RLX_EUNSUP, f + ": B too large for the 32-bit key count B + 1");
  RLX_REQUIRE(ctx->world == 1, RLX_EUNSUP, f + ": no data-parallel form (the context's world size must be 1)");
  int rc = ens_check_net(*pdesc, "td3", "pdesc");
  if (rc) return rc;
  rc = ens_check_net(*qdesc, "td3", "qdesc");
  if (rc) return rc;
  rc = dpg_check_hp(*hp, f);
  if (rc) return rc;
  EnsDims d;
  rc = det_prologue(fn, *pdesc, *qdesc, states, next_states, hp->critic_states, hp->critic_next_states, &d);
  if (rc) return rc;
  const int E = hp->nr_critics, A = d.A, Op = d.Op, Oc = d.Oc, ldc = d.ldc, ldp = d.ldp;
  const bool joint = hp->joint != 0, pstep = hp->policy_step != 0;
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain LP = ens_layout(*pdesc), LQ = ens_layout(*qdesc);
  const int64_t np_ = LP.n_params, nq = LQ.n_params;
  const int nblk = div_up(B, 256);
  // ---- arena: the two policy passes, one buffer set for the targets' inference passes, one per online critic
  ChainBufs bpt, bpc, bi, bq[DPG_MAXE];
  float *xc, *xn, *xp, *xsn, *xsc, *hn, *hc, *dpi, *y, *qn, *q, *dq, *qa, *seed, *da, *gp, *gq, *part_q, *part_p;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(LP, B, a, &bpt);
    chain_carve(LP, B, a, &bpc);
    chain_carve(LQ, B, a, &bi);
    for (int e = 0; e < E; ++e) chain_carve(LQ, B, a, &bq[e]);
    for (float** x : {&xc, &xn, &xp}) *x = a.take((size_t)B * ldc);
    for (float** x : {&xsn, &xsc}) *x = a.take((size_t)B * ldp);
    for (float** x : {&hn, &hc, &dpi}) *x = a.take((size_t)B * A);
    y = a.take(B);
    for (float** x : {&qn, &q, &dq, &qa, &seed}) *x = a.take((size_t)E * B);
    da = a.take((size_t)E * B * ldc);
    gp = a.take(np_);
    gq = a.take((size_t)E * nq);
    for (float** x : {&part_q, &part_p}) *x = a.take(2 * (size_t)nblk);      // doubles (every arena buffer starts 256-byte aligned)
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc || !sq) return RLX_ENOMEM;
  // ---- the key (td3.py:149-150): TD3 splits it B + 1 ways whatever smoothing_epsilon is; DDPG's update takes none
  uint32_t key[2] = {key_io[0], key_io[1]};
  const EnsRowKeys rows{key_io[0], key_io[1], scheme, 1u, 1u, (uint32_t)(B + 1)};
  if (!joint) split_at_host(key_io, 0, (uint32_t)(B + 1), scheme, key);
  BxReleaseAll bx_all{ctx};
  const PlainAdamHp ahp{0.f, hp->adam_b1, hp->adam_b2, hp->adam_eps};
  FsFork fk(ctx, st);
  rc = fk.begin();
  if (rc) return rc;
  auto lane = [&](int e) { return e == 1 ? fk.side() : fk.main(); };   // critic 1 on the side stream (under scratch bank 1)
  {  // the images of the critic step's passes (joint: of the whole call, nothing is stepped in between)
    NetRef nets[2 + 2 * DPG_MAXE];
    int n = 0;
    nets[n++] = NetRef{ptarget, &LP, false};
    for (int e = 0; e < E; ++e) nets[n++] = NetRef{qtarget + e * nq, &LQ, false};
    for (int e = 0; e < E; ++e) nets[n++] = NetRef{qparams + e * nq, &LQ, true};
    if (joint) nets[n++] = NetRef{pparams, &LP, true};
    rc = trunk_images(ctx, nets, n, B, st);
    if (rc) return rc;
  }
  // ---- critic step (td3.py:116-160; ddpg.py:121-126): the online critics on (s, a) on the side stream; the target policy on s', the
  // smoothed target action and the target critics on (s', a') on the caller's
  rc = fs_concat(d.cs, Oc, actions, A, xc, ldc, B, st);
  if (!rc) rc = fk.fork();
  for (int e = 0; e < E && !rc; ++e) rc = chain_fwd(ctx, LQ, qparams + e * nq, xc, ldc, bq[e], q + (size_t)e * B, B, fk.side());
  if (!rc) rc = fs_concat(d.cn, Oc, nullptr, A, xn, ldc, B, fk.main());
  if (!rc) rc = fs_concat(next_states, Op, nullptr, 0, xsn, ldp, B, st);
  if (!rc) rc = chain_fwd(ctx, LP, ptarget, xsn, ldp, bpt, hn, B, st);
  if (!rc) rc = dpg_target_action(hn, xn, ldc, Oc, B, A, !joint, rows, hp->smoothing_epsilon, hp->smoothing_clip_value, ctx->dbg_sac_eps[0], st);
  for (int e = 0; e < E && !rc; ++e) rc = chain_fwd(ctx, LQ, qtarget + e * nq, xn, ldc, bi, qn + (size_t)e * B, B, st);
  if (!rc) rc = fk.join();
  if (rc) return rc;
  hipLaunchKernelGGL(k_dpg_critic_loss, dim3(nblk), dim3(256), 0, st, (const float*)q, (const float*)qn, rewards, terminations, y, dq,
                     (double*)part_q, B, E, hp->gamma);
  RLX_LAUNCH_CHECK();
  {  // one deferred reduction for both critics; the split-operand gradient scale is that of E B rows: |d loss / d q| ~ 2 |q - y| / (E B)
    BwdPass bwd(ctx, B * E);
    rc = bwd.begin(E * chain_stage_floats(ctx, LQ, B, true));
    if (!rc) rc = fk.fork();
    for (int e = E - 1; e >= 0 && !rc; --e)
      rc = chain_bwd(ctx, LQ, qparams + e * nq, xc, ldc, bq[e], dq + (size_t)e * B, gq + e * nq, nullptr, 0, B, lane(e));
    if (!rc) rc = fk.join();
    if (!rc) rc = bwd.finish(st);
    if (rc) return rc;
  }
  const int64_t qstep = *q_opt_count_io + 1, pistep = *pi_opt_count_io + 1;
  // plain Adam of the critics (td3.py:156) -- the Polyak step of a call with a policy step (:193) rides in the same launch: nothing
  // reads the critics' targets in between.  DDPG's comes after the policy's backward (ddpg.py:151-156).
  auto critic_adam = [&]() {
    return torch_clip_adam(qparams, gq, qm, qv, (int64_t)E * nq, sq, qstep, hp->lr_critic, ahp, metrics_out + 1, st, pstep ? qtarget : nullptr,
                           hp->tau);
  };
  if (!joint) {
    rc = critic_adam();
    if (rc) return rc;
  }
  if (pstep) {
    // ---- policy step (td3.py:164-199; ddpg.py:128-131): the policy on s, its action straight into the critics' input rows, one critic
    // per stream, the seeds, the critics' input gradients on the action columns, the policy's backward
    if (!joint) {
      NetRef nets[1 + DPG_MAXE];
      int n = 0;
      nets[n++] = NetRef{pparams, &LP, true};
      for (int e = 0; e < E; ++e) nets[n++] = NetRef{qparams + e * nq, &LQ, true};
      bx_release_all(ctx);
      rc = trunk_images(ctx, nets, n, B, st);
      if (rc) return rc;
    }
    rc = fs_concat(d.cs, Oc, nullptr, A, xp, ldc, B, st);
    if (!rc) rc = fs_concat(states, Op, nullptr, 0, xsc, ldp, B, st);
    if (!rc) rc = chain_fwd(ctx, LP, pparams, xsc, ldp, bpc, hc, B, st);
    if (!rc) rc = dpg_target_action(hc, xp, ldc, Oc, B, A, false, rows, 0.f, 0.f, nullptr, st);
    if (!rc) rc = fk.fork();
    for (int e = E - 1; e >= 0 && !rc; --e) rc = chain_fwd(ctx, LQ, qparams + e * nq, xp, ldc, bq[e], qa + (size_t)e * B, B, lane(e));
    if (!rc) rc = fk.join();
    if (rc) return rc;
    hipLaunchKernelGGL(k_dpg_policy_seed, dim3(nblk), dim3(256), 0, st, (const float*)qa, seed, (double*)part_p, B, E);
    RLX_LAUNCH_CHECK();
    {
      BwdPass bwd(ctx, B);   // seeds of 0 or -1 / (B n_ties); the policy's head gradient is ~ 1 / B per sample
      rc = bwd.begin(E * chain_stage_floats(ctx, LQ, B, false) + chain_stage_floats(ctx, LP, B, true));
      if (!rc) rc = fk.fork();
      for (int e = E - 1; e >= 0 && !rc; --e)
        rc = chain_bwd(ctx, LQ, qparams + e * nq, xp, ldc, bq[e], seed + (size_t)e * B, nullptr, da + (size_t)e * B * ldc, ldc, B, lane(e), Oc, A);
      if (!rc) rc = fk.join();
      if (!rc) rc = dpg_tanh_bwd(xp, da, E == 2 ? da + (size_t)B * ldc : nullptr, ldc, Oc, dpi, B, A, st);
      if (!rc) rc = chain_bwd(ctx, LP, pparams, xsc, ldp, bpc, dpi, gp, nullptr, 0, B, st);
      if (!rc) rc = bwd.finish(st);
      if (rc) return rc;
    }
  }
  if (joint) {
    rc = critic_adam();
    if (rc) return rc;
  }
  // metrics: [0] loss/q_loss, [1] gradients/critic_grad_norm; with a policy step [2] loss/policy_loss, [3] q_value/q_value, [4]
  // gradients/policy_grad_norm (else left alone)
  hipLaunchKernelGGL(k_dpg_finish, dim3(1), dim3(256), 0, st, (const double*)part_q, nblk, (double)B * E, metrics_out,
                     pstep ? (const double*)part_p : (const double*)nullptr, nblk, (double)B, metrics_out + 2);
  RLX_LAUNCH_CHECK();
  if (pstep) {   // plain Adam of the policy (td3.py:190), then its Polyak step (:194) in the same launch
    rc = torch_clip_adam(pparams, gp, pm, pv, np_, sq, pistep, hp->lr_policy, ahp, metrics_out + 4, st, ptarget, hp->tau);
    if (rc) return rc;
  }
  key_io[0] = key[0];
  key_io[1] = key[1];
  *q_opt_count_io += 1;
  if (pstep) *pi_opt_count_io += 1;
  return RLX_OK;
}

}  // extern "C"
