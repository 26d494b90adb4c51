// tqc.hip -- TQC, truncated quantile critics (rl_x/algorithms/tqc/flax/tqc.py:134-230): SAC's tanh-Gaussian policy, entropy
// coefficient, key schedule and three plain Adam steps with another critic -- an ensemble of E independent quantile networks with
// N atoms each (tqc/flax/critic.py:17-55).  What differs from sac.hip (tqc.py against sac/flax/sac.py):
//   target      the T = E N next-state atoms of the target networks are POOLED, sorted ascending, and the first K = T - E * dropped
//               are kept (tqc.py:155-159): y_k = r + gamma (1 - term) (z_(k) - alpha logp')
//   critic loss quantile Huber loss over all (online atom i, target k) pairs (tqc.py:161-170), tau_i = (i + 0.5) / T with the
//               flat index i = e N + n of q_atoms.reshape(nr_total_atoms); the online atoms are not sorted
//   policy loss alpha logp - mean over all T atoms of the frozen critics on (s, a_pi) (tqc.py:182-185)
//
// Networks: rlx_mlp_desc with act = RELU, ln_first = 0, has_logstd = 0 (flat layout: per layer W[in, out] row-major, b[out]; then
// the head).  Policy: out_dim = 2 A, head columns [0, A) the mean, [A, 2A) the raw log-std.  Critics: E networks back to back,
// each in_dim = Oc + A, out_dim = N.  A network is net_pass.h's Chain of plain blocks, as in fasttd3.hip: the library's GEMM stages,
// the split-operand engine for passes of >= 4096 rows (trunk_images; the fp16 window of fasttd3.hip's header applies), stage_dw for
// the weight gradients, dense_head.hip for the heads.  sac.hip's fused twin-critic kernels are not used: they assume two critics
// with one output each.
//
// Schedule of one update (one stream, no host synchronisation): policy on s' -> sample a', logp' -> E target chains -> k_tqc_target;
// E online chains on (s, a) -> k_tqc_qloss -> E backward passes; policy on s -> sample a~, logp -> per critic: forward on (s, a~),
// input gradient on the action columns from the constant seed -1 / (B T) -> k_ens_policy_grad -> policy backward; k_ens_atom_rowsum, k_ens_finish
// (metrics, the entropy coefficient's Adam step); plain Adam of the policy; plain Adam of all E critics with the Polyak step.
// The sample, the policy's head gradient, the means and the finish are sac_ens.hip's, shared with redq.hip; the noise keys are SAC's
// schedule 0: keys = split(key, 2B+1), key = keys[0], next-state / current-state noise of row i from keys[1 + 2i] / keys[2 + 2i]
// (tqc.py:211-212).  Every reduction runs in a fixed order: two identical calls give identical bits.
//
// Atoms that are NaN are outside the contract: the sort compares with fminf / fmaxf, which drop a NaN operand, so a row holding
// one loses it (and duplicates a neighbour) instead of propagating it.  +-inf atoms sort as values.
// CPU twin: tests/tqc_twin.py (float64).  The reference's TQC is JAX only; see DESIGN.md 4.5d for what is pinned.
#include "sac_ens.h"

namespace rlx {

constexpr int TQC_MAXT = 128;   // two atoms per lane of one wave (c51.hip's cap)
constexpr int TQC_MAXE = 8;

// ---------------------------------------------------------------------------------------------------------------- kernels
// Atom i = e N + n of row b lives at atoms[(e B + b) N + n] (ens_atom); the wave-level bitonic sort is ens_sort: both in sac_ens.h,
// shared with aqe.hip.
// y[b, k] = r_b + gamma (1 - term_b) (z_(k) - alpha logp'_b), k < K: the K smallest of the row's pooled T target atoms
// (tqc.py:155-158).  One wave per transition, four per workgroup; absent lanes hold +inf, which sorts behind every atom.
__global__ __launch_bounds__(256) void k_tqc_target(const float* __restrict__ zt, const float* __restrict__ rew, const float* __restrict__ term,
                                                    const float* __restrict__ nlogp, const float* __restrict__ log_alpha,
                                                    float* __restrict__ y, int64_t B, int N, int T, int K, float gamma) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  if (b >= B) return;                                   // (whole waves leave: no workgroup barrier below)
  float v[2];
  v[0] = lane < T ? ens_atom(zt, b, lane, B, N) : INFINITY;
  v[1] = lane + 64 < T ? ens_atom(zt, b, lane + 64, B, N) : INFINITY;
  if (T > 64) ens_sort<2>(v, lane);
  else ens_sort<1>(v, lane);
  const float disc = gamma * (1.0f - term[b]);
  const float ent = expf(log_alpha[0]) * nlogp[b];
  const float r = rew[b];
  if (lane < K) y[b * K + lane] = r + disc * (v[0] - ent);
  if (lane + 64 < K) y[b * K + lane + 64] = r + disc * (v[1] - ent);
}

// Quantile Huber loss of one transition over all (atom i, target k) pairs and its gradient (tqc.py:161-170): delta = y_k - q_i,
// h = |delta| <= kappa ? delta^2 / 2 : kappa (|delta| - kappa / 2), w = |tau_i - [delta < 0]|, tau_i = (i + 0.5) / T;
//   loss_row[b] = sum w h / kappa / (T K);   dq[b, i] = -(1 / (B T K)) sum_k w clamp(delta, -kappa, kappa) / kappa.
// One wave per transition; lane <-> atom i (two per lane above 64), target k broadcast from the lane that holds it.
__global__ __launch_bounds__(256) void k_tqc_qloss(const float* __restrict__ q, const float* __restrict__ y, float* __restrict__ dq,
                                                   float* __restrict__ loss_row, int64_t B, int N, int T, int K, float kappa) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  if (b >= B) return;                                   // (whole waves leave: no workgroup barrier below)
  const bool h0 = lane < T, h1 = lane + 64 < T;
  const float q0 = h0 ? ens_atom(q, b, lane, B, N) : 0.f, q1 = h1 ? ens_atom(q, b, lane + 64, B, N) : 0.f;
  const float y0 = lane < K ? y[b * K + lane] : 0.f, y1 = lane + 64 < K ? y[b * K + lane + 64] : 0.f;
  const float tau0 = ((float)lane + 0.5f) / (float)T, tau1 = ((float)(lane + 64) + 0.5f) / (float)T;
  float l0 = 0.f, l1 = 0.f, g0 = 0.f, g1 = 0.f;
  for (int k = 0; k < K; ++k) {
    const float yk = __shfl(k < 64 ? y0 : y1, k & 63, 64);
    {
      const float d = yk - q0, ad = fabsf(d);
      const float h = ad <= kappa ? 0.5f * d * d : kappa * (ad - 0.5f * kappa);
      const float wt = fabsf(tau0 - (d < 0.f ? 1.0f : 0.0f));
      l0 += wt * h;
      g0 += wt * fminf(fmaxf(d, -kappa), kappa);
    }
    if (T > 64) {
      const float d = yk - q1, ad = fabsf(d);
      const float h = ad <= kappa ? 0.5f * d * d : kappa * (ad - 0.5f * kappa);
      const float wt = fabsf(tau1 - (d < 0.f ? 1.0f : 0.0f));
      l1 += wt * h;
      g1 += wt * fminf(fmaxf(d, -kappa), kappa);
    }
  }
  const float inv_pairs = 1.0f / ((float)T * (float)K);
  const float gs = -inv_pairs / ((float)B * kappa);
  if (h0) dq[((int64_t)(lane / N) * B + b) * N + lane % N] = gs * g0;
  if (h1) dq[((int64_t)((lane + 64) / N) * B + b) * N + (lane + 64) % N] = gs * g1;
  const float loss = wave_sum((h0 ? l0 : 0.f) + (h1 ? l1 : 0.f));
  if (lane == 0) loss_row[b] = loss / kappa * inv_pairs;
}

// ---------------------------------------------------------------------------------------------------------------- host
// ensemble_size E, nr_atoms_per_net N, nr_dropped_atoms_per_net, huber_kappa (tqc/flax/default_config.py:18-21)
static int tqc_check_hp(const rlx_tqc_hparams& hp, int* T_out, int* K_out) {
  RLX_REQUIRE(hp.ensemble_size >= 1, RLX_EINVAL, "tqc: hp->ensemble_size must be at least 1");
  RLX_REQUIRE(hp.ensemble_size <= TQC_MAXE, RLX_EUNSUP, "tqc: hp->ensemble_size at most 8");
  RLX_REQUIRE(hp.nr_atoms_per_net >= 1, RLX_EINVAL, "tqc: hp->nr_atoms_per_net must be at least 1");
  RLX_REQUIRE((int64_t)hp.ensemble_size * hp.nr_atoms_per_net <= TQC_MAXT, RLX_EUNSUP,
              "tqc: hp->ensemble_size * hp->nr_atoms_per_net (total atoms) at most 128");
  RLX_REQUIRE(hp.nr_dropped_atoms_per_net >= 0 && hp.nr_dropped_atoms_per_net < hp.nr_atoms_per_net, RLX_EINVAL,
              "tqc: hp->nr_dropped_atoms_per_net must be in [0, nr_atoms_per_net)");
  RLX_REQUIRE(hp.huber_kappa > 0.f, RLX_EINVAL, "tqc: hp->huber_kappa must be positive");
  *T_out = hp.ensemble_size * hp.nr_atoms_per_net;
  *K_out = *T_out - hp.ensemble_size * hp.nr_dropped_atoms_per_net;
  return RLX_OK;
}

// y (tqc.py:155-158), the pair loss and its gradient (tqc.py:161-170) on given atoms; loss_row: B floats of scratch
static int tqc_loss(const float* q, const float* zt, const float* rew, const float* term, const float* nlogp, const float* log_alpha,
                    int64_t B, const rlx_tqc_hparams& hp, int T, int K, float* y, float* dq, float* loss_row, float* loss_out,
                    hipStream_t st) {
  const int N = hp.nr_atoms_per_net;
  hipLaunchKernelGGL(k_tqc_target, dim3(div_up(B, 4)), dim3(256), 0, st, zt, rew, term, nlogp, log_alpha, y, B, N, T, K, hp.gamma);
  RLX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_tqc_qloss, dim3(div_up(B, 4)), dim3(256), 0, st, q, (const float*)y, dq, loss_row, B, N, T, K, hp.huber_kappa);
  RLX_LAUNCH_CHECK();
  return ens_mean(loss_row, B, loss_out, st);
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int rlx_tqc_quantile_loss_f32(rlx_ctx* ctx, const float* q_atoms, const float* next_atoms, const float* rewards, const float* terminations,
                              const float* next_logp, const float* log_alpha, int64_t B, const rlx_tqc_hparams* hp, float* dq_out,
                              float* loss_out, float* y_out, void* stream) {
  RLX_REQUIRE(ctx && hp, RLX_EINVAL, "rlx_tqc_quantile_loss_f32: ctx / hp is NULL");
  RLX_REQUIRE(q_atoms && next_atoms && rewards && terminations && next_logp && log_alpha, RLX_EINVAL,
              "rlx_tqc_quantile_loss_f32: NULL input (q_atoms, next_atoms, rewards, terminations, next_logp, log_alpha)");
  RLX_REQUIRE(dq_out, RLX_EINVAL, "rlx_tqc_quantile_loss_f32: dq_out is NULL");
  RLX_REQUIRE(loss_out, RLX_EINVAL, "rlx_tqc_quantile_loss_f32: loss_out is NULL");
  RLX_REQUIRE(B > 0, RLX_EINVAL, "rlx_tqc_quantile_loss_f32: B must be positive");
  int T, K;
  const int rc = tqc_check_hp(*hp, &T, &K);
  if (rc) return rc;
  float* tmp = (float*)scratch(ctx, SL_STAGE, (a64((size_t)B) + a64((size_t)B * K)) * sizeof(float));
  if (!tmp) return RLX_ENOMEM;
  return tqc_loss(q_atoms, next_atoms, rewards, terminations, next_logp, log_alpha, B, *hp, T, K, y_out ? y_out : tmp + a64((size_t)B), dq_out,
                  tmp, loss_out, (hipStream_t)stream);
}

int rlx_tqc_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, const rlx_mlp_desc* qdesc,
                       float* qparams, float* qm, float* qv, float* qtarget, float* log_alpha, float* am, float* av, const float* states,
                       const float* next_states, const float* actions, const float* rewards, const float* terminations, int64_t B,
                       uint32_t key_io[2], int scheme, int64_t* opt_count_io, const rlx_tqc_hparams* hp, float* metrics_out, void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && pm && pv && qdesc && qparams && qm && qv && qtarget && log_alpha && am && av && states &&
                  next_states && actions && rewards && terminations && key_io && opt_count_io && hp && metrics_out,
              RLX_EINVAL, "rlx_tqc_update_f32: NULL pointer");
  RLX_REQUIRE(B > 0, RLX_EINVAL, "rlx_tqc_update_f32: B must be positive");
  RLX_REQUIRE(2 * B + 1 <= 0x7fffffffLL, RLX_EUNSUP, "rlx_tqc_update_f32: B too large for the 32-bit key count 2 B + 1");
  int rc = ens_check_net(*pdesc, "tqc", "pdesc");
  if (rc) return rc;
  rc = ens_check_net(*qdesc, "tqc", "qdesc");
  if (rc) return rc;
  int T, K;
  rc = tqc_check_hp(*hp, &T, &K);
  if (rc) return rc;
  const int E = hp->ensemble_size, N = hp->nr_atoms_per_net;
  EnsDims d;
  rc = ens_prologue("rlx_tqc_update_f32", *pdesc, *qdesc, N, "must equal hp->nr_atoms_per_net", states, next_states, hp->critic_states,
                    hp->critic_next_states, &d);
  if (rc) return rc;
  const int A = d.A, Oc = d.Oc, ldc = d.ldc, ldp = d.ldp;
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain LP = ens_layout(*pdesc), LQ = ens_layout(*qdesc);
  const int64_t np_ = LP.n_params, nq = LQ.n_params;
  const size_t BN = (size_t)B * N;
  // ---- arena: the policy's two passes, one buffer set for the inference passes of the critics (targets; online on (s, a~), whose
  // backward follows at once), E sets for the online critics on (s, a), whose backward waits for the loss
  ChainBufs bpn, bpc, bi, bq[TQC_MAXE];
  float *xc, *xn, *xp, *xsn, *xsc, *hn, *hc, *dpi, *lpn, *lpc, *zt, *q, *dq, *qa, *seed, *da, *y, *loss_row, *qa_row, *gp, *gq;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(LP, B, a, &bpn);
    chain_carve(LP, B, a, &bpc);
    chain_carve(LQ, B, a, &bi);
    for (int e = 0; e < E; ++e) chain_carve(LQ, B, a, &bq[e]);
    for (float** x : {&xc, &xn, &xp}) *x = a.take((size_t)B * ldc);
    for (float** x : {&xsn, &xsc}) *x = a.take((size_t)B * ldp);
    for (float** x : {&hn, &hc, &dpi}) *x = a.take((size_t)B * 2 * A);
    for (float** x : {&lpn, &lpc, &loss_row, &qa_row}) *x = a.take(B);
    for (float** x : {&zt, &q, &dq, &qa}) *x = a.take((size_t)E * BN);
    seed = a.take(BN);
    da = a.take((size_t)E * B * ldc);
    y = a.take((size_t)B * K);
    gp = a.take(np_);
    gq = a.take((size_t)E * nq);
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc || !sq) return RLX_ENOMEM;
  // keys = split(key, 2B+1); key = keys[0]; row i's noise from keys[1 + 2i] on s', keys[2 + 2i] on s (tqc.py:211-212: sac_key_index)
  const EnsRowKeys kn{key_io[0], key_io[1], scheme, 1u, 2u, sac_key_count(B, 0)}, kc{kn.k0, kn.k1, scheme, 2u, 2u, kn.count};
  split_at_host(key_io, 0, kn.count, scheme, key_io);
  // ---- split-operand images of the hidden layers (>= 4096 rows).  The image builder takes BX_MAX_JOBS jobs: the policy (both
  // directions), then the online critics (three passes each, both directions), then the targets (one pass each); what no longer
  // fits -- from six critics with three hidden layers on -- runs on the exact engine (trunk_images).
  BxReleaseAll bx_all{ctx};
  {
    NetRef nets[1 + 2 * TQC_MAXE];
    int n = 0;
    nets[n++] = NetRef{pparams, &LP, true};
    for (int e = 0; e < E; ++e) nets[n++] = NetRef{qparams + e * nq, &LQ, true};
    for (int e = 0; e < E; ++e) nets[n++] = NetRef{qtarget + e * nq, &LQ, false};
    rc = trunk_images(ctx, nets, n, B, st);
    if (rc) return rc;
  }
  const SacSampleArgs sa = ens_sample_args(d, hp->log_std_min, hp->log_std_max, B);
  // ---- critic loss (tqc.py:144-170): a', logp' from the policy on s'; the E target networks on (s', a'); the online ones on (s, a)
  rc = ens_policy_sample(ctx, d, LP, pparams, d.cn, next_states, xn, xsn, bpn, hn, lpn, sa, kn, ctx->dbg_sac_eps[0], B, st);
  for (int e = 0; e < E && !rc; ++e) rc = chain_fwd(ctx, LQ, qtarget + e * nq, xn, ldc, bi, zt + e * BN, B, st);
  if (!rc) rc = fs_concat(d.cs, Oc, actions, A, xc, ldc, B, st);
  for (int e = 0; e < E && !rc; ++e) rc = chain_fwd(ctx, LQ, qparams + e * nq, xc, ldc, bq[e], q + e * BN, B, st);
  if (!rc) rc = tqc_loss(q, zt, rewards, terminations, lpn, log_alpha, B, *hp, T, K, y, dq, loss_row, metrics_out, st);
  // one deferred reduction per critic: its table takes one network's segments, not eight networks'.  The split-operand gradient
  // scale is that of B T rows: |d loss / d atom| is at most 1 / (B T).
  for (int e = 0; e < E && !rc; ++e) {
    BwdPass bwd(ctx, B * T);
    rc = bwd.begin(chain_stage_floats(ctx, LQ, B, true));
    if (!rc) rc = chain_bwd(ctx, LQ, qparams + e * nq, xc, ldc, bq[e], dq + e * BN, gq + e * nq, nullptr, 0, B, st);
    if (!rc) rc = bwd.finish(st);
  }
  if (rc) return rc;
  // ---- policy loss (tqc.py:173-185): a~, logp from the policy on s; per frozen critic the atoms on (s, a~) and, from the constant
  // seed d(-mean atoms) / d atom = -1 / (B T), the input gradient on the action columns
  rc = ens_policy_sample(ctx, d, LP, pparams, d.cs, states, xp, xsc, bpc, hc, lpc, sa, kc, ctx->dbg_sac_eps[1], B, st);
  if (rc) return rc;
  rc = ens_fill(seed, (int64_t)BN, -1.0f / ((float)B * (float)T), st);
  if (rc) return rc;
  {
    BwdPass bwd(ctx, B);   // the policy's head gradient is ~ 1 / B per sample (up to ~ 2 e^log_std_max |eps| alpha / B)
    rc = bwd.begin(E * chain_stage_floats(ctx, LQ, B, false) + chain_stage_floats(ctx, LP, B, true));
    {
      GradScaleScope atoms(ctx, bx_grad_scale(B * T));   // the critics' passes start from exactly 1 / (B T)
      for (int e = 0; e < E && !rc; ++e) {
        rc = chain_fwd(ctx, LQ, qparams + e * nq, xp, ldc, bi, qa + e * BN, B, st);
        if (!rc) rc = chain_bwd(ctx, LQ, qparams + e * nq, xp, ldc, bi, seed, nullptr, da + (size_t)e * B * ldc, ldc, B, st, Oc, A);
      }
    }
    if (rc) return rc;
    rc = ens_policy_grad(hc, xp, ldc, Oc, da, ldc, (int64_t)B * ldc, E, log_alpha, kc, dpi, B, A, hp->log_std_min, hp->log_std_max,
                         ctx->dbg_sac_eps[1], st);
    if (!rc) rc = chain_bwd(ctx, LP, pparams, xsc, ldp, bpc, dpi, gp, nullptr, 0, B, st);
    if (!rc) rc = bwd.finish(st);
    if (rc) return rc;
  }
  // ---- metrics and the three plain Adam steps (tqc.py:218-228); the critics' launch also takes the Polyak step (tqc.py:223)
  const int64_t step = *opt_count_io + 1;
  float sched[3];
  adam_schedule_entry(sched, step, hp->lr_alpha, hp->adam_b1, hp->adam_b2);
  rc = ens_atom_rowsum(qa, qa_row, B, N, T, st);
  if (!rc) rc = ens_finish(qa_row, (int64_t)E * (int64_t)BN, lpc, B, nullptr, 0, log_alpha, am, av, metrics_out, hp->target_entropy, sched,
                           hp->adam_b1, hp->adam_b2, hp->adam_eps, st);
  const PlainAdamHp ahp{0.f, hp->adam_b1, hp->adam_b2, hp->adam_eps};
  if (!rc) rc = torch_clip_adam(pparams, gp, pm, pv, np_, sq, step, hp->lr_policy, ahp, metrics_out + 6, st);
  if (!rc) rc = torch_clip_adam(qparams, gq, qm, qv, (int64_t)E * nq, sq, step, hp->lr_critic, ahp, metrics_out + 7, st, qtarget, hp->tau);
  if (rc) return rc;
  *opt_count_io += 1;
  return RLX_OK;
}

}  // extern "C"
