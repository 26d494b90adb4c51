// aqe.hip -- AQE, truncated-mean multi-head ensemble critics (rl_x/algorithms/aqe/flax/aqe.py:145-259): REDQ's high update-to-data
// `update` -- G = q_update_steps critic steps on G fresh batches, then ONE policy / entropy step -- over E critics with H =
// nr_heads_per_net outputs each (aqe/flax/critic.py: Dense(nr_heads_per_net) head).  What differs from redq.hip (aqe.py against
// redq/flax/redq.py):
//   keys        every step, critic or policy: keys = split(key, B + 1), key = keys[0], row b's noise key keys[1 + b] (aqe.py:231-232,
//               :245-246); there is no subset and no host shuffle
//   target      ALL E target networks are evaluated; their T = E H values of a transition are POOLED, sorted ascending, and the
//               mean of the first K = T - nr_dropped_q_values is taken (aqe.py:164-165; :58-59: the drop is from the pool, not per
//               net): y = r + gamma (1 - term) (that mean - alpha logp') (:167)
//   critic loss mean over batch and all T heads of (q - y)^2 (:169-171, safe_mean at :221): d loss / d q[e, b, h] =
//               2 (q[e, b, h] - y_b) / (B T)
//   policy loss alpha logp - mean over ALL T heads (:197-200): the constant seed -1 / (B T), as tqc.hip's; q_value is the mean of
//               the row means
// The loop, plain Adam and Polyak after every critic step (:236-237), the two counters, the metric means over the G steps (:242),
// the policy step on batch 0 with the critics from after the loop (:248) are redq.hip's.
//
// Networks: rlx_mlp_desc as tqc.hip takes them (ReLU, no LayerNorm; policy out_dim = 2 A; critics: E networks back to back, each
// in_dim = Oc + A, out_dim = H).  Q values are laid out [E][B][H], critic-major, as E head GEMMs leave them; flat index i = e H + h
// (`reshape(nr_total_q_values)`, aqe.py:165).  Passes of >= 4096 rows take the split-operand images (trunk_images), REBUILT in front
// of every critic step from the current parameters in the order of their use: the policy (forward), the E targets (forward), the E
// online critics (both directions); what does not fit the image builder's job table runs on the exact engine (net_pass.h).
//
// Schedule of one call (one stream, no host synchronisation): the key chain on the host; per critic step: policy on s'_i ->
// k_ens_sample -> E target chains (one buffer set) -> E online chains on (s_i, a_i) (E kept sets) -> k_aqe_target_loss ->
// k_ens_mean (slot i) -> E backward passes -> Adam + Polyak of all critics (norm to slot G + i); then the policy step: policy on s_0
// -> k_ens_sample -> per critic: forward on (s_0, a~) and AT ONCE its input gradient on the action columns from the constant seed
// (one buffer set serves all E) -> k_ens_atom_rowsum -> k_ens_policy_grad -> policy backward -> k_ens_finish (metrics, the means over
// the G steps, alpha's Adam step at the POLICY counter) -> Adam of the policy.  The k_ens_* kernels, the value indexing (ens_atom) and
// the wave-level bitonic sort (ens_sort) are sac_ens.h's, shared with tqc.hip and redq.hip.
// Every reduction runs in a fixed order without atomics: two identical calls give identical bits.
//
// Q values that are NaN are outside the contract, as in tqc.hip: the sort compares with fminf / fmaxf, which drop a NaN operand, so
// a row holding one loses it (and duplicates a neighbour) instead of propagating it.  +-inf values sort as values.
// CPU twin: tests/aqe_twin.py (float64).  The reference's AQE is JAX only; see DESIGN.md 4.5f for what is pinned.
#include "sac_ens.h"

namespace rlx {

constexpr int AQE_MAXT = 128;   // two values per lane of one wave (tqc.hip's cap)
constexpr int AQE_MAXE = 16;
constexpr int AQE_MAXG = 64;

// ---------------------------------------------------------------------------------------------------------------- kernels
// Target and critic loss of one transition in one launch (aqe.py:164-171).  One wave per transition, four per workgroup.
//   target  the row's T pooled target values, one per lane (two above 64; absent lanes hold +inf, which sorts behind every value),
//           sorted ascending; the sum of the K lowest over the wave in a fixed order, divided by K once;
//           y_b = r_b + gamma (1 - term_b) (that mean - alpha logp'_b)
//   loss    lane <-> online value i = e H + h: dq[e, b, h] = 2 (q - y_b) / (B T); loss_row[b] = mean_i (q_i - y_b)^2
// y / loss_row may be NULL.  No LDS, no scratch, no atomics.
__global__ __launch_bounds__(256) void k_aqe_target_loss(const float* __restrict__ q, const float* __restrict__ qn, const float* __restrict__ rew,
                                                         const float* __restrict__ term, const float* __restrict__ nlogp,
                                                         const float* __restrict__ log_alpha, float* __restrict__ y, float* __restrict__ dq,
                                                         float* __restrict__ loss_row, int64_t B, int H, int T, int K, float gamma) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  if (b >= B) return;                                   // (whole waves leave: no workgroup barrier below)
  const bool h0 = lane < T, h1 = lane + 64 < T;
  float v[2];
  v[0] = h0 ? ens_atom(qn, b, lane, B, H) : INFINITY;
  v[1] = h1 ? ens_atom(qn, b, lane + 64, B, H) : INFINITY;
  if (T > 64) ens_sort<2>(v, lane);
  else ens_sort<1>(v, lane);
  const float low = wave_sum((lane < K ? v[0] : 0.f) + (lane + 64 < K ? v[1] : 0.f));
  const float tmean = __shfl(low, 0, 64) / (float)K;    // every lane takes lane 0's sum: one value per row, whatever wave_sum leaves
  const float yb = rew[b] + gamma * (1.0f - term[b]) * (tmean - expf(log_alpha[0]) * nlogp[b]);
  if (y && lane == 0) y[b] = yb;
  const float gs = 2.0f / ((float)B * (float)T);
  float l = 0.f;
  if (h0) {
    const int64_t i0 = ens_atom_index(b, lane, B, H);
    const float d = q[i0] - yb;
    dq[i0] = gs * d;
    l = d * d;
  }
  if (h1) {
    const int64_t i1 = ens_atom_index(b, lane + 64, B, H);
    const float d = q[i1] - yb;
    dq[i1] = gs * d;
    l = fmaf(d, d, l);
  }
  if (loss_row) {                                       // (wave-uniform)
    const float loss = wave_sum(l);
    if (lane == 0) loss_row[b] = loss / (float)T;
  }
}

// row[b] = row[b] / T: the row mean over the T heads from k_ens_atom_rowsum's sum (rlx_aqe_losses_f32's meanq_out)
__global__ __launch_bounds__(256) void k_aqe_row_mean(float* __restrict__ row, int64_t B, int T) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < B) row[b] = row[b] / (float)T;
}

// ---------------------------------------------------------------------------------------------------------------- host
// ensemble_size E, nr_heads_per_net H, nr_dropped_q_values, q_update_steps G (aqe/flax/default_config.py:18-21)
static int aqe_check_hp(const rlx_aqe_hparams& hp, int* T_out, int* K_out) {
  RLX_REQUIRE(hp.ensemble_size >= 1, RLX_EINVAL, "aqe: hp->ensemble_size must be at least 1");
  RLX_REQUIRE(hp.ensemble_size <= AQE_MAXE, RLX_EUNSUP, "aqe: hp->ensemble_size at most 16");
  RLX_REQUIRE(hp.nr_heads_per_net >= 1, RLX_EINVAL, "aqe: hp->nr_heads_per_net must be at least 1");
  RLX_REQUIRE((int64_t)hp.ensemble_size * hp.nr_heads_per_net <= AQE_MAXT, RLX_EUNSUP,
              "aqe: hp->ensemble_size * hp->nr_heads_per_net (total q values) at most 128");
  const int T = hp.ensemble_size * hp.nr_heads_per_net;
  RLX_REQUIRE(hp.nr_dropped_q_values >= 0 && hp.nr_dropped_q_values < T, RLX_EINVAL,
              "aqe: hp->nr_dropped_q_values must be in [0, ensemble_size * nr_heads_per_net)");
  RLX_REQUIRE(hp.q_update_steps >= 1, RLX_EINVAL, "aqe: hp->q_update_steps must be at least 1");
  RLX_REQUIRE(hp.q_update_steps <= AQE_MAXG, RLX_EUNSUP, "aqe: hp->q_update_steps at most 64");
  *T_out = T;
  *K_out = T - hp.nr_dropped_q_values;
  return RLX_OK;
}

static int aqe_target_loss(const float* q, const float* qn, const float* rew, const float* term, const float* nlogp, const float* log_alpha,
                           int64_t B, int H, int T, int K, float gamma, float* y, float* dq, float* loss_row, float* loss_out, hipStream_t st) {
  hipLaunchKernelGGL(k_aqe_target_loss, dim3(div_up(B, 4)), dim3(256), 0, st, q, qn, rew, term, nlogp, log_alpha, y, dq, loss_row, B, H, T, K,
                     gamma);
  RLX_LAUNCH_CHECK();
  return loss_out ? ens_mean(loss_row, B, loss_out, st) : RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int rlx_aqe_losses_f32(rlx_ctx* ctx, const float* q, const float* q_next, const float* rewards, const float* terminations,
                       const float* next_logp, const float* log_alpha, const float* qa, int64_t B, const rlx_aqe_hparams* hp, float* y_out,
                       float* dq_out, float* loss_out, float* seed_out, float* meanq_out, void* stream) {
  RLX_REQUIRE(ctx && hp, RLX_EINVAL, "rlx_aqe_losses_f32: ctx / hp is NULL");
  RLX_REQUIRE(q && q_next && rewards && terminations && next_logp && log_alpha, RLX_EINVAL,
              "rlx_aqe_losses_f32: NULL input (q, q_next, rewards, terminations, next_logp, log_alpha)");
  RLX_REQUIRE(dq_out, RLX_EINVAL, "rlx_aqe_losses_f32: dq_out is NULL");
  RLX_REQUIRE(!qa || seed_out, RLX_EINVAL, "rlx_aqe_losses_f32: qa needs seed_out");
  RLX_REQUIRE(B > 0, RLX_EINVAL, "rlx_aqe_losses_f32: B must be positive");
  int T, K;
  const int rc = aqe_check_hp(*hp, &T, &K);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* loss_row = nullptr;
  if (loss_out) {
    loss_row = (float*)scratch(ctx, SL_STAGE, a64((size_t)B) * sizeof(float));
    if (!loss_row) return RLX_ENOMEM;
  }
  const int H = hp->nr_heads_per_net;
  int rc2 = aqe_target_loss(q, q_next, rewards, terminations, next_logp, log_alpha, B, H, T, K, hp->gamma, y_out, dq_out, loss_row, loss_out, st);
  if (rc2 || !qa) return rc2;
  rc2 = ens_fill(seed_out, (int64_t)B * T, -1.0f / ((float)B * (float)T), st);
  if (rc2 || !meanq_out) return rc2;
  rc2 = ens_atom_rowsum(qa, meanq_out, B, H, T, st);
  if (rc2) return rc2;
  hipLaunchKernelGGL(k_aqe_row_mean, dim3(div_up(B, 256)), dim3(256), 0, st, meanq_out, B, T);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int rlx_aqe_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, const rlx_mlp_desc* qdesc,
                       float* qparams, float* qm, float* qv, float* qtarget, float* log_alpha, float* am, float* av, const float* states,
                       const float* next_states, const float* actions, const float* rewards, const float* terminations, int64_t B,
                       uint32_t key_io[2], int scheme, int64_t* q_opt_count_io, int64_t* pi_opt_count_io, const rlx_aqe_hparams* hp,
                       float* metrics_out, void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && pm && pv && qdesc && qparams && qm && qv && qtarget && log_alpha && am && av && states &&
                  next_states && actions && rewards && terminations && key_io && q_opt_count_io && pi_opt_count_io && hp && metrics_out,
              RLX_EINVAL, "rlx_aqe_update_f32: NULL pointer");
  RLX_REQUIRE(B > 0, RLX_EINVAL, "rlx_aqe_update_f32: B must be positive");
  RLX_REQUIRE(B + 1 <= 0x7fffffffLL, RLX_EUNSUP, "rlx_aqe_update_f32: B too large for the 32-bit key count B + 1");
  int rc = ens_check_net(*pdesc, "aqe", "pdesc");
  if (rc) return rc;
  rc = ens_check_net(*qdesc, "aqe", "qdesc");
  if (rc) return rc;
  int T, K;
  rc = aqe_check_hp(*hp, &T, &K);
  if (rc) return rc;
  const int E = hp->ensemble_size, H = hp->nr_heads_per_net, G = hp->q_update_steps;
  EnsDims d;
  rc = ens_prologue("rlx_aqe_update_f32", *pdesc, *qdesc, H, "must equal hp->nr_heads_per_net", states, next_states, hp->critic_states,
                    hp->critic_next_states, &d);
  if (rc) return rc;
  const int A = d.A, Op = d.Op, Oc = d.Oc, ldc = d.ldc, ldp = d.ldp;
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain LP = ens_layout(*pdesc), LQ = ens_layout(*qdesc);
  const int64_t np_ = LP.n_params, nq = LQ.n_params;
  const size_t BH = (size_t)B * H;
  // ---- arena: the policy's passes; one buffer set for the inference passes of the critics (targets; online on (s_0, a~), whose
  // input gradient follows at once); E sets for the online critics on (s_i, a_i), whose backward waits for the loss
  ChainBufs bpn, bpc, bi, bq[AQE_MAXE];
  float *xc, *xn, *xp, *xsn, *xsc, *hn, *hc, *dpi, *lpn, *lpc, *qn, *q, *dq, *qa, *seed, *da, *y, *loss_row, *qa_row, *gp, *gq, *steps;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(LP, B, a, &bpn);
    chain_carve(LP, B, a, &bpc);
    chain_carve(LQ, B, a, &bi);
    for (int e = 0; e < E; ++e) chain_carve(LQ, B, a, &bq[e]);
    for (float** x : {&xc, &xn, &xp}) *x = a.take((size_t)B * ldc);
    for (float** x : {&xsn, &xsc}) *x = a.take((size_t)B * ldp);
    for (float** x : {&hn, &hc, &dpi}) *x = a.take((size_t)B * 2 * A);
    for (float** x : {&lpn, &lpc, &loss_row, &qa_row, &y}) *x = a.take(B);
    for (float** x : {&qn, &q, &dq, &qa}) *x = a.take((size_t)E * BH);
    seed = a.take(BH);
    da = a.take((size_t)E * B * ldc);
    gp = a.take(np_);
    gq = a.take((size_t)E * nq);
    steps = a.take(2 * (size_t)G);
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc || !sq) return RLX_ENOMEM;
  // ---- the key chain (aqe.py:231-232, :245-246), on the host: G times split(key, B + 1)[0], then once more for the policy step
  uint32_t step_key[AQE_MAXG + 1][2];                         // the key each step splits
  uint32_t key[2] = {key_io[0], key_io[1]};
  for (int i = 0; i <= G; ++i) {
    step_key[i][0] = key[0];
    step_key[i][1] = key[1];
    split_at_host(step_key[i], 0, (uint32_t)(B + 1), scheme, key);
  }
  BxReleaseAll bx_all{ctx};
  const SacSampleArgs sa = ens_sample_args(d, hp->log_std_min, hp->log_std_max, B);
  const PlainAdamHp ahp{0.f, hp->adam_b1, hp->adam_b2, hp->adam_eps};
  // ---- G critic steps (aqe.py:230-240)
  for (int i = 0; i < G; ++i) {
    const float* s2_i = next_states + (size_t)i * B * Op;
    const float* cs_i = d.cs + (size_t)i * B * Oc;
    const float* cn_i = d.cn + (size_t)i * B * Oc;
    const float* a_i = actions + (size_t)i * B * A;
    {  // the images of this step's passes, from the parameters as the previous step left them
      NetRef nets[1 + 2 * AQE_MAXE];
      int n = 0;
      nets[n++] = NetRef{pparams, &LP, false};
      for (int e = 0; e < E; ++e) nets[n++] = NetRef{qtarget + e * nq, &LQ, false};
      for (int e = 0; e < E; ++e) nets[n++] = NetRef{qparams + e * nq, &LQ, true};
      bx_release_all(ctx);
      rc = trunk_images(ctx, nets, n, B, st);
      if (rc) return rc;
    }
    // a', logp' from the policy on s'; all E targets on (s', a'); the E online critics on (s, a)
    const EnsRowKeys ki{step_key[i][0], step_key[i][1], scheme, 1u, 1u, (uint32_t)(B + 1)};
    rc = ens_policy_sample(ctx, d, LP, pparams, cn_i, s2_i, xn, xsn, bpn, hn, lpn, sa, ki,
                           ctx->dbg_sac_eps[0] ? ctx->dbg_sac_eps[0] + (size_t)i * B * A : nullptr, B, st);
    for (int e = 0; e < E && !rc; ++e) rc = chain_fwd(ctx, LQ, qtarget + e * nq, xn, ldc, bi, qn + e * BH, B, st);
    if (!rc) rc = fs_concat(cs_i, Oc, a_i, A, xc, ldc, B, st);
    for (int e = 0; e < E && !rc; ++e) rc = chain_fwd(ctx, LQ, qparams + e * nq, xc, ldc, bq[e], q + e * BH, B, st);
    if (!rc) rc = aqe_target_loss(q, qn, rewards + (size_t)i * B, terminations + (size_t)i * B, lpn, log_alpha, B, H, T, K, hp->gamma, y, dq,
                                  loss_row, steps + i, st);
    // one deferred reduction per critic; the split-operand gradient scale is that of B T rows: |d loss / d q| is ~ 2 |q - y| / (B T)
    for (int e = 0; e < E && !rc; ++e) {
      BwdPass bwd(ctx, B * T);
      rc = bwd.begin(chain_stage_floats(ctx, LQ, B, true));
      if (!rc) rc = chain_bwd(ctx, LQ, qparams + e * nq, xc, ldc, bq[e], dq + e * BH, gq + e * nq, nullptr, 0, B, st);
      if (!rc) rc = bwd.finish(st);
    }
    // plain Adam of all E critics with the Polyak step (aqe.py:236-237), at this step's learning rate and count
    if (!rc) rc = torch_clip_adam(qparams, gq, qm, qv, (int64_t)E * nq, sq, *q_opt_count_io + i + 1, hp->lr_critic + (float)i * hp->lr_critic_delta,
                                  ahp, steps + G + i, st, qtarget, hp->tau);
    if (rc) return rc;
  }
  // ---- policy / entropy step (aqe.py:245-251) on batch 0, with the critics from after the G steps
  {
    NetRef nets[1 + AQE_MAXE];
    int n = 0;
    nets[n++] = NetRef{pparams, &LP, true};
    for (int e = 0; e < E; ++e) nets[n++] = NetRef{qparams + e * nq, &LQ, true};
    bx_release_all(ctx);
    rc = trunk_images(ctx, nets, n, B, st);
    if (rc) return rc;
  }
  const EnsRowKeys kp{step_key[G][0], step_key[G][1], scheme, 1u, 1u, (uint32_t)(B + 1)};
  rc = ens_policy_sample(ctx, d, LP, pparams, d.cs, states, xp, xsc, bpc, hc, lpc, sa, kp, ctx->dbg_sac_eps[1], B, st);
  // the constant seed d(-mean over the T heads) / d q = -1 / (B T) needs no other critic's value: one buffer set serves all E
  if (!rc) rc = ens_fill(seed, (int64_t)BH, -1.0f / ((float)B * (float)T), st);
  if (rc) return rc;
  {
    BwdPass bwd(ctx, B);   // the policy's head gradient is ~ 1 / B per sample
    rc = bwd.begin(E * chain_stage_floats(ctx, LQ, B, false) + chain_stage_floats(ctx, LP, B, true));
    {
      GradScaleScope heads(ctx, bx_grad_scale(B * T));   // the critics' passes start from exactly 1 / (B T)
      for (int e = 0; e < E && !rc; ++e) {
        rc = chain_fwd(ctx, LQ, qparams + e * nq, xp, ldc, bi, qa + e * BH, B, st);
        if (!rc) rc = chain_bwd(ctx, LQ, qparams + e * nq, xp, ldc, bi, seed, nullptr, da + (size_t)e * B * ldc, ldc, B, st, Oc, A);
      }
    }
    if (rc) return rc;
    rc = ens_atom_rowsum(qa, qa_row, B, H, T, st);
    if (!rc) rc = ens_policy_grad(hc, xp, ldc, Oc, da, ldc, (int64_t)B * ldc, E, log_alpha, kp, dpi, B, A, hp->log_std_min, hp->log_std_max,
                                  ctx->dbg_sac_eps[1], st);
    if (!rc) rc = chain_bwd(ctx, LP, pparams, xsc, ldp, bpc, dpi, gp, nullptr, 0, B, st);
    if (!rc) rc = bwd.finish(st);
    if (rc) return rc;
  }
  // ---- metrics, alpha's and the policy's plain Adam steps at the policy counter (aqe.py:250-251)
  const int64_t pstep = *pi_opt_count_io + 1;
  float sched[3];
  adam_schedule_entry(sched, pstep, hp->lr_alpha, hp->adam_b1, hp->adam_b2);
  rc = ens_finish(qa_row, (int64_t)B * T, lpc, B, steps, G, log_alpha, am, av, metrics_out, hp->target_entropy, sched, hp->adam_b1, hp->adam_b2,
                  hp->adam_eps, st);
  if (!rc) rc = torch_clip_adam(pparams, gp, pm, pv, np_, sq, pstep, hp->lr_policy, ahp, metrics_out + 6, st);
  if (rc) return rc;
  key_io[0] = key[0];
  key_io[1] = key[1];
  *q_opt_count_io += G;
  *pi_opt_count_io += 1;
  return RLX_OK;
}

}  // extern "C"
