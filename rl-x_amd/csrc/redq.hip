// redq.hip -- REDQ, randomized ensembled double Q-learning (rl_x/algorithms/redq/flax/redq.py:144-261): SAC's tanh-Gaussian policy
// and entropy coefficient with an ensemble of E scalar critics (redq/flax/critic.py:17-53) and a HIGH update-to-data `update`:
// G = q_update_steps critic steps on G fresh batches, then ONE policy / entropy step.  What differs from sac.hip and tqc.hip:
//   keys        critic step i: keys = split(key, B + 2), key = keys[0], sample_key = keys[1], row b's noise key keys[2 + b]
//               (redq.py:229-230); policy step: keys = split(key, B + 1), key = keys[0], row b's keys[1 + b] (:247-248)
//   target      m_indices = choice(sample_key, arange(E), (M,), replace=False) (:232-233) = permutation(sample_key, E)[:M]: one
//               sort round for 2 <= E <= 16, none for E = 1; y = r + gamma (1 - term) (min over the M SELECTED targets - alpha logp')
//   critic loss mean over batch AND ensemble of (q_e - y)^2 (:169, safe_mean at :219): d loss / d q[e, b] = 2 (q[e, b] - y_b) / (B E)
//   loop        every critic step is followed by plain Adam on all E critics and Polyak (:238-239); step i + 1 sees the new
//               parameters and targets; policy and alpha are untouched inside the loop; q_loss and critic_grad_norm are the means
//               over the G steps (:244)
//   policy loss alpha logp - min over ALL E critics (:195-198): the gradient goes to the minimising critic, split evenly among
//               exact ties as jnp.min's gradient does
//   counters    two: the critics' Adam counter advances by G per call, the policy's / alpha's by 1
//
// Networks: rlx_mlp_desc as tqc.hip takes them (ReLU, no LayerNorm; policy out_dim = 2 A; critics: E networks back to back, each
// in_dim = Oc + A, out_dim = 1).  Q values are laid out [E][B], critic-major, as E head GEMMs with one output leave them.  A network
// is net_pass.h's Chain; passes of >= 4096 rows take the split-operand images (trunk_images), which are REBUILT in front of every
// critic step from the current parameters: the policy (forward), the M selected targets, the E online critics (both directions), in
// the order of their use; what does not fit the image builder's job table runs on the exact engine (net_pass.h).  The image builder
// registers one list per launch, so the policy's two forward images are part of every step's list.
//
// Schedule of one call (one stream, no host synchronisation): the key chain and the G subsets on the host; per critic step: policy
// on s'_i -> k_ens_sample -> M target chains -> E online chains on (s_i, a_i) -> k_redq_critic_loss -> k_ens_mean (slot i) -> E
// backward passes -> Adam + Polyak of all critics (norm to slot i); then the policy step: policy on s_0 -> k_ens_sample -> E
// forward passes on (s_0, a~) into E kept buffer sets -> k_redq_policy_seed -> E input-gradient passes on the action columns ->
// k_ens_policy_grad -> policy backward -> k_ens_finish (metrics, the means over the G steps, alpha's Adam step at the POLICY
// counter) -> Adam of the policy.  The k_ens_* kernels are sac_ens.hip's, shared with tqc.hip.
// Every reduction runs in a fixed order without atomics: two identical calls give identical bits.
// CPU twin: tests/redq_twin.py (float64).  The reference's REDQ is JAX only; see DESIGN.md 4.5e for what is pinned.
// The update's body is redq_loop, which serves three entry points under a RedqLoopSpec (redq_loop.h); this schedule is theirs too.
// droq.hip: LayerNorm / dropout critics and its own key layout.  aqe.hip: H values per critic (q, dq, qa, seed are [E][B][H]), M = E
// targets in index order and no sample_key, k_aqe_target_loss for k_redq_critic_loss, and k_ens_fill + k_ens_atom_rowsum for
// k_redq_policy_seed.
#include "redq_loop.h"

namespace rlx {

// ---------------------------------------------------------------------------------------------------------------- kernels
// One thread per transition (redq.py:163-169): y_b = r_b + gamma (1 - term_b) (min_m qn[m, b] - alpha logp'_b) over the M selected
// target rows; dq[e, b] = 2 (q[e, b] - y_b) / (B E); loss_row[b] = mean_e (q[e, b] - y_b)^2.  y / loss_row may be NULL.
__global__ __launch_bounds__(256) void k_redq_critic_loss(const float* __restrict__ q, const float* __restrict__ qn, const float* __restrict__ rew,
                                                          const float* __restrict__ term, const float* __restrict__ nlogp,
                                                          const float* __restrict__ log_alpha, float* __restrict__ y, float* __restrict__ dq,
                                                          float* __restrict__ loss_row, int64_t B, int E, int M, float gamma) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float mn = qn[b];
  for (int m = 1; m < M; ++m) mn = fminf(mn, qn[(int64_t)m * B + b]);
  const float yb = rew[b] + gamma * (1.0f - term[b]) * (mn - expf(log_alpha[0]) * nlogp[b]);
  if (y) y[b] = yb;
  const float gs = 2.0f / ((float)B * (float)E);
  float loss = 0.f;
  for (int e = 0; e < E; ++e) {
    const float d = q[(int64_t)e * B + b] - yb;
    dq[(int64_t)e * B + b] = gs * d;
    loss = fmaf(d, d, loss);
  }
  if (loss_row) loss_row[b] = loss / (float)E;
}

// One thread per transition (redq.py:195-198): minq_row[b] = min_e qa[e, b]; seed[e, b] = d mean_b(-min_e) / d qa[e, b] =
// -[qa[e, b] == min] / (B n_ties), the even split jnp.min's gradient takes among exact ties.  minq_row may be NULL.
__global__ __launch_bounds__(256) void k_redq_policy_seed(const float* __restrict__ qa, float* __restrict__ seed, float* __restrict__ minq_row,
                                                          int64_t B, int E) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float mn = qa[b];
  for (int e = 1; e < E; ++e) mn = fminf(mn, qa[(int64_t)e * B + b]);
  int ties = 0;
  for (int e = 0; e < E; ++e) ties += qa[(int64_t)e * B + b] == mn ? 1 : 0;
  const float s = -1.0f / ((float)B * (float)(ties > 0 ? ties : 1));
  for (int e = 0; e < E; ++e) seed[(int64_t)e * B + b] = qa[(int64_t)e * B + b] == mn ? s : 0.f;
  if (minq_row) minq_row[b] = mn;
}

// ---------------------------------------------------------------------------------------------------------------- host
int redq_check_hp(const rlx_redq_hparams& hp, const char* algo) {
  const std::string a(algo);
  RLX_REQUIRE(hp.ensemble_size >= 1, RLX_EINVAL, a + ": hp->ensemble_size must be at least 1");
  RLX_REQUIRE(hp.ensemble_size <= REDQ_MAXE, RLX_EUNSUP, a + ": hp->ensemble_size at most 16");
  RLX_REQUIRE(hp.in_target_minimization_size >= 1 && hp.in_target_minimization_size <= hp.ensemble_size, RLX_EINVAL,
              a + ": hp->in_target_minimization_size must be in [1, ensemble_size]");
  RLX_REQUIRE(hp.q_update_steps >= 1, RLX_EINVAL, a + ": hp->q_update_steps must be at least 1");
  RLX_REQUIRE(hp.q_update_steps <= REDQ_MAXG, RLX_EUNSUP, a + ": hp->q_update_steps at most 64");
  return RLX_OK;
}

// permutation(sample_key, E)[:M] (jax _shuffle): ceil(3 ln E / ln(2^32 - 1)) rounds of {key, sub = split(key); stable sort by
// random_bits(sub, (E,))} -- one round for 2 <= E <= 16, none for E = 1
static void redq_subset(const uint32_t sample_key[2], int E, int M, int scheme, int32_t* idx_out) {
  uint32_t key[2] = {sample_key[0], sample_key[1]};
  int32_t idx[REDQ_MAXE];
  for (int e = 0; e < E; ++e) idx[e] = e;
  const int rounds = (int)ceil(3.0 * log((double)E) / log(4294967295.0));
  for (int r = 0; r < rounds; ++r) {
    uint32_t sub[2], nxt[2];
    split_at_host(key, 0, 2, scheme, nxt);
    split_at_host(key, 1, 2, scheme, sub);
    key[0] = nxt[0];
    key[1] = nxt[1];
    uint32_t bits[REDQ_MAXE];
    for (int e = 0; e < E; ++e) bits[e] = random_bits_at(sub[0], sub[1], (uint64_t)e, (uint64_t)E, scheme);
    for (int a = 1; a < E; ++a) {   // insertion sort: stable
      const uint32_t kb = bits[a];
      const int32_t ki = idx[a];
      int c = a - 1;
      for (; c >= 0 && bits[c] > kb; --c) {
        bits[c + 1] = bits[c];
        idx[c + 1] = idx[c];
      }
      bits[c + 1] = kb;
      idx[c + 1] = ki;
    }
  }
  for (int m = 0; m < M; ++m) idx_out[m] = idx[m];
}

int redq_critic_loss(const float* q, const float* qn, const float* rew, const float* term, const float* nlogp, const float* log_alpha,
                     int64_t B, const RedqLossDims& n, float gamma, float* y, float* dq, float* loss_row, float* loss_out, hipStream_t st) {
  hipLaunchKernelGGL(k_redq_critic_loss, dim3(div_up(B, 256)), dim3(256), 0, st, q, qn, rew, term, nlogp, log_alpha, y, dq, loss_row, B, n.E,
                     n.M, gamma);
  RLX_LAUNCH_CHECK();
  return loss_out ? ens_mean(loss_row, B, loss_out, st) : RLX_OK;
}

// the dropout keys of network j's pass in a step (NULL without dropout: the chain then never reads them)
static const DropKeys* redq_drop_keys(const RedqLoopSpec& spec, const uint32_t step_key[2], int scheme, RedqKeySlot slot, uint32_t count,
                                      int j, int E, DropKeys* at) {
  if (!(spec.critic_drop > 0.f)) return nullptr;
  *at = DropKeys{step_key[0], step_key[1], scheme, slot.base, slot.stride, count, j, E};
  return at;
}

int redq_loop(rlx_ctx* ctx, const RedqLoopSpec& spec, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
              const rlx_mlp_desc* qdesc, float* qparams, float* qm, float* qv, float* qtarget, float* log_alpha, float* am, float* av,
              const float* states, const float* next_states, const float* actions, const float* rewards, const float* terminations,
              int64_t B, uint32_t key_io[2], int scheme, int64_t* q_opt_count_io, int64_t* pi_opt_count_io, const rlx_redq_hparams* hp,
              float* metrics_out, int32_t* subsets_out, void* stream) {
  const std::string fn(spec.fn);
  RLX_REQUIRE(ctx && pdesc && pparams && pm && pv && qdesc && qparams && qm && qv && qtarget && log_alpha && am && av && states &&
                  next_states && actions && rewards && terminations && key_io && q_opt_count_io && pi_opt_count_io && hp && metrics_out,
              RLX_EINVAL, fn + ": NULL pointer");
  RLX_REQUIRE(B > 0, RLX_EINVAL, fn + ": B must be positive");
  const int64_t kc = spec.critic_keys_per_row, kp = spec.policy_keys_per_row;
  const int64_t own = spec.target_subset ? 2 : 1;   // a critic step's keys in front of the rows': key, and sample_key with a subset
  RLX_REQUIRE(B <= (0x7fffffffLL - own) / kc, RLX_EUNSUP,
              fn + ": B too large for the 32-bit key count " + (kc == 1 ? "B" : std::to_string(kc) + " B") + " + " + std::to_string(own));
  int rc = ens_check_net(*pdesc, spec.algo, "pdesc");
  if (rc) return rc;
  rc = ens_check_net(*qdesc, spec.algo, "qdesc");
  if (rc) return rc;
  rc = spec.check_hp(*hp, spec);
  if (rc) return rc;
  const int E = hp->ensemble_size, M = hp->in_target_minimization_size, G = hp->q_update_steps, H = spec.heads, T = E * H;
  const RedqLossDims dims{E, H, M, M * H - spec.dropped};
  EnsDims d;
  rc = ens_prologue(spec.fn, *pdesc, *qdesc, H, spec.heads_rule, states, next_states, hp->critic_states, hp->critic_next_states, &d);
  if (rc) return rc;
  const int A = d.A, Op = d.Op, Oc = d.Oc, ldc = d.ldc, ldp = d.ldp;
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain LP = ens_layout(*pdesc);
  const Chain LQ = make_chain(qdesc->in_dim, qdesc->hidden, qdesc->n_hidden, qdesc->out_dim, spec.critic_norm, RLX_ACT_RELU, spec.critic_eps,
                              spec.critic_drop);
  const uint32_t count_c = (uint32_t)(kc * B + own), count_p = (uint32_t)(kp * B + 1);   // the split counts of a critic / the policy step
  DropKeys dk;
  const int64_t np_ = LP.n_params, nq = LQ.n_params;
  const size_t BH = (size_t)B * H;
  // ---- arena: the policy's passes, one buffer set for the targets' inference passes, E sets for the online critics: their backward
  // waits for the loss in a critic step and for the seed -- which needs all E values -- in the policy step
  ChainBufs bpn, bpc, bi, bq[REDQ_MAXE];
  float *xc, *xn, *xp, *xsn, *xsc, *hn, *hc, *dpi, *lpn, *lpc, *qn, *q, *dq, *qa, *seed, *da, *y, *loss_row, *q_row, *gp, *gq, *steps;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(LP, B, a, &bpn);
    chain_carve(LP, B, a, &bpc);
    chain_carve(LQ, B, a, &bi);
    for (int e = 0; e < E; ++e) chain_carve(LQ, B, a, &bq[e]);
    for (float** x : {&xc, &xn, &xp}) *x = a.take((size_t)B * ldc);
    for (float** x : {&xsn, &xsc}) *x = a.take((size_t)B * ldp);
    for (float** x : {&hn, &hc, &dpi}) *x = a.take((size_t)B * 2 * A);
    for (float** x : {&lpn, &lpc, &loss_row, &q_row, &y}) *x = a.take(B);
    qn = a.take((size_t)M * BH);
    for (float** x : {&q, &dq, &qa, &seed}) *x = a.take((size_t)E * BH);
    da = a.take((size_t)E * B * ldc);
    gp = a.take(np_);
    gq = a.take((size_t)E * nq);
    steps = a.take(2 * (size_t)G);
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc || !sq) return RLX_ENOMEM;
  // ---- the key chain (redq.py:229-230, :247-248) and the G target subsets (:232-233; without one, every target in index order), all
  // on the host
  uint32_t step_key[REDQ_MAXG + 1][2];                        // the key each step splits
  int32_t subset[REDQ_MAXG][REDQ_MAXE];
  uint32_t key[2] = {key_io[0], key_io[1]};
  for (int i = 0; i < G; ++i) {
    uint32_t nxt[2];
    step_key[i][0] = key[0];
    step_key[i][1] = key[1];
    split_at_host(key, 0, count_c, scheme, nxt);
    if (spec.target_subset) {
      uint32_t sample_key[2];
      split_at_host(key, 1, count_c, scheme, sample_key);
      redq_subset(sample_key, E, M, scheme, subset[i]);
    } else {
      for (int m = 0; m < M; ++m) subset[i][m] = m;
    }
    key[0] = nxt[0];
    key[1] = nxt[1];
  }
  step_key[G][0] = key[0];
  step_key[G][1] = key[1];
  split_at_host(step_key[G], 0, count_p, scheme, key);
  BxReleaseAll bx_all{ctx};
  const SacSampleArgs sa = ens_sample_args(d, hp->log_std_min, hp->log_std_max, B);
  const PlainAdamHp ahp{0.f, hp->adam_b1, hp->adam_b2, hp->adam_eps};
  // ---- G critic steps (redq.py:228-242)
  for (int i = 0; i < G; ++i) {
    const float* s2_i = next_states + (size_t)i * B * Op;
    const float* cs_i = d.cs + (size_t)i * B * Oc;
    const float* cn_i = d.cn + (size_t)i * B * Oc;
    const float* a_i = actions + (size_t)i * B * A;
    {  // the images of this step's passes, from the parameters as the previous step left them
      NetRef nets[1 + 2 * REDQ_MAXE];
      int n = 0;
      nets[n++] = NetRef{pparams, &LP, false};
      for (int m = 0; m < M; ++m) nets[n++] = NetRef{qtarget + subset[i][m] * nq, &LQ, false};
      for (int e = 0; e < E; ++e) nets[n++] = NetRef{qparams + e * nq, &LQ, true};
      bx_release_all(ctx);
      rc = trunk_images(ctx, nets, n, B, st);
      if (rc) return rc;
    }
    // a', logp' from the policy on s'; the M selected targets on (s', a'); the E online critics on (s, a)
    const EnsRowKeys ki{step_key[i][0], step_key[i][1], scheme, spec.next_noise.base, spec.next_noise.stride, count_c};
    rc = ens_policy_sample(ctx, d, LP, pparams, cn_i, s2_i, xn, xsn, bpn, hn, lpn, sa, ki,
                           ctx->dbg_sac_eps[0] ? ctx->dbg_sac_eps[0] + (size_t)i * B * A : nullptr, B, st);
    for (int m = 0; m < M && !rc; ++m)   // (the m-th selected target is network m of its vmapped pass)
      rc = chain_fwd(ctx, LQ, qtarget + subset[i][m] * nq, xn, ldc, bi, qn + m * BH, B, st,
                     redq_drop_keys(spec, step_key[i], scheme, spec.target_drop, count_c, m, E, &dk));
    if (!rc) rc = fs_concat(cs_i, Oc, a_i, A, xc, ldc, B, st);
    for (int e = 0; e < E && !rc; ++e)
      rc = chain_fwd(ctx, LQ, qparams + e * nq, xc, ldc, bq[e], q + e * BH, B, st,
                     redq_drop_keys(spec, step_key[i], scheme, spec.online_drop, count_c, e, E, &dk));
    if (!rc) rc = spec.critic_loss(q, qn, rewards + (size_t)i * B, terminations + (size_t)i * B, lpn, log_alpha, B, dims, hp->gamma, y, dq,
                                   loss_row, steps + i, st);
    // one deferred reduction per critic; the split-operand gradient scale is that of B T rows: |d loss / d q| is ~ 2 |q - y| / (B T)
    for (int e = 0; e < E && !rc; ++e) {
      BwdPass bwd(ctx, B * T);
      rc = bwd.begin(chain_stage_floats(ctx, LQ, B, true));
      if (!rc) rc = chain_bwd(ctx, LQ, qparams + e * nq, xc, ldc, bq[e], dq + e * BH, gq + e * nq, nullptr, 0, B, st, 0, 0,
                              redq_drop_keys(spec, step_key[i], scheme, spec.online_drop, count_c, e, E, &dk));
      if (!rc) rc = bwd.finish(st);
    }
    // plain Adam of all E critics with the Polyak step (redq.py:238-239), at this step's learning rate and count
    if (!rc) rc = torch_clip_adam(qparams, gq, qm, qv, (int64_t)E * nq, sq, *q_opt_count_io + i + 1, hp->lr_critic + (float)i * hp->lr_critic_delta,
                                  ahp, steps + G + i, st, qtarget, hp->tau);
    if (rc) return rc;
  }
  // ---- policy / entropy step (redq.py:246-253) on batch 0, with the critics from after the G steps
  {
    NetRef nets[1 + REDQ_MAXE];
    int n = 0;
    nets[n++] = NetRef{pparams, &LP, true};
    for (int e = 0; e < E; ++e) nets[n++] = NetRef{qparams + e * nq, &LQ, true};
    bx_release_all(ctx);
    rc = trunk_images(ctx, nets, n, B, st);
    if (rc) return rc;
  }
  const EnsRowKeys kpol{step_key[G][0], step_key[G][1], scheme, spec.cur_noise.base, spec.cur_noise.stride, count_p};
  rc = ens_policy_sample(ctx, d, LP, pparams, d.cs, states, xp, xsc, bpc, hc, lpc, sa, kpol, ctx->dbg_sac_eps[1], B, st);
  for (int e = 0; e < E && !rc; ++e)
    rc = chain_fwd(ctx, LQ, qparams + e * nq, xp, ldc, bq[e], qa + e * BH, B, st,
                   redq_drop_keys(spec, step_key[G], scheme, spec.policy_drop, count_p, e, E, &dk));
  if (rc) return rc;
  if (spec.policy_min) {
    hipLaunchKernelGGL(k_redq_policy_seed, dim3(div_up(B, 256)), dim3(256), 0, st, (const float*)qa, seed, q_row, B, E);
    RLX_LAUNCH_CHECK();
  } else {
    rc = ens_fill(seed, (int64_t)E * BH, -1.0f / ((float)B * (float)T), st);
    if (!rc) rc = ens_atom_rowsum(qa, q_row, B, H, T, st);
    if (rc) return rc;
  }
  {
    BwdPass bwd(ctx, B);   // the policy's head gradient is ~ 1 / B per sample
    rc = bwd.begin(E * chain_stage_floats(ctx, LQ, B, false) + chain_stage_floats(ctx, LP, B, true));
    {  // the critics' passes: seeds of 0 or -1 / (B n_ties) under the minimum, of exactly -1 / (B T) under the mean
      GradScaleScope seeds(ctx, bx_grad_scale(spec.policy_min ? B : B * T));
      for (int e = 0; e < E && !rc; ++e)
        rc = chain_bwd(ctx, LQ, qparams + e * nq, xp, ldc, bq[e], seed + e * BH, nullptr, da + (size_t)e * B * ldc, ldc, B, st, Oc, A,
                       redq_drop_keys(spec, step_key[G], scheme, spec.policy_drop, count_p, e, E, &dk));
    }
    if (rc) return rc;
    rc = ens_policy_grad(hc, xp, ldc, Oc, da, ldc, (int64_t)B * ldc, E, log_alpha, kpol, dpi, B, A, hp->log_std_min, hp->log_std_max,
                         ctx->dbg_sac_eps[1], st);
    if (!rc) rc = chain_bwd(ctx, LP, pparams, xsc, ldp, bpc, dpi, gp, nullptr, 0, B, st);
    if (!rc) rc = bwd.finish(st);
    if (rc) return rc;
  }
  // ---- metrics, alpha's and the policy's plain Adam steps at the policy counter (redq.py:252-253)
  const int64_t pstep = *pi_opt_count_io + 1;
  float sched[3];
  adam_schedule_entry(sched, pstep, hp->lr_alpha, hp->adam_b1, hp->adam_b2);
  rc = ens_finish(q_row, spec.policy_min ? B : B * T, lpc, B, steps, G, log_alpha, am, av, metrics_out, hp->target_entropy, sched,
                  hp->adam_b1, hp->adam_b2, hp->adam_eps, st);
  if (!rc) rc = torch_clip_adam(pparams, gp, pm, pv, np_, sq, pstep, hp->lr_policy, ahp, metrics_out + 6, st);
  if (rc) return rc;
  key_io[0] = key[0];
  key_io[1] = key[1];
  *q_opt_count_io += G;
  *pi_opt_count_io += 1;
  if (subsets_out)
    for (int i = 0; i < G; ++i)
      for (int m = 0; m < M; ++m) subsets_out[i * M + m] = subset[i][m];
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int rlx_redq_subset_host(const uint32_t sample_key[2], int E, int M, int scheme, int32_t* idx_out) {
  RLX_REQUIRE(sample_key && idx_out, RLX_EINVAL, "rlx_redq_subset_host: NULL pointer");
  RLX_REQUIRE(E >= 1 && E <= REDQ_MAXE, RLX_EINVAL, "rlx_redq_subset_host: E must be in [1, 16]");
  RLX_REQUIRE(M >= 1 && M <= E, RLX_EINVAL, "rlx_redq_subset_host: M must be in [1, E]");
  redq_subset(sample_key, E, M, scheme, idx_out);
  return RLX_OK;
}

int rlx_redq_losses_f32(rlx_ctx* ctx, const float* q, const float* q_next_sel, const float* rewards, const float* terminations,
                        const float* next_logp, const float* log_alpha, const float* qa, int64_t B, const rlx_redq_hparams* hp, float* y_out,
                        float* dq_out, float* loss_out, float* seed_out, float* minq_out, void* stream) {
  RLX_REQUIRE(ctx && hp, RLX_EINVAL, "rlx_redq_losses_f32: ctx / hp is NULL");
  RLX_REQUIRE(q && q_next_sel && rewards && terminations && next_logp && log_alpha, RLX_EINVAL,
              "rlx_redq_losses_f32: NULL input (q, q_next_sel, rewards, terminations, next_logp, log_alpha)");
  RLX_REQUIRE(dq_out, RLX_EINVAL, "rlx_redq_losses_f32: dq_out is NULL");
  RLX_REQUIRE(!qa || seed_out, RLX_EINVAL, "rlx_redq_losses_f32: qa needs seed_out");
  RLX_REQUIRE(B > 0, RLX_EINVAL, "rlx_redq_losses_f32: B must be positive");
  const int rc = redq_check_hp(*hp, "redq");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* loss_row = nullptr;
  if (loss_out) {
    loss_row = (float*)scratch(ctx, SL_STAGE, a64((size_t)B) * sizeof(float));
    if (!loss_row) return RLX_ENOMEM;
  }
  const int E = hp->ensemble_size, M = hp->in_target_minimization_size;
  const int rc2 = redq_critic_loss(q, q_next_sel, rewards, terminations, next_logp, log_alpha, B, RedqLossDims{E, 1, M, M}, hp->gamma, y_out,
                                   dq_out, loss_row, loss_out, st);
  if (rc2 || !qa) return rc2;
  hipLaunchKernelGGL(k_redq_policy_seed, dim3(div_up(B, 256)), dim3(256), 0, st, qa, seed_out, minq_out, B, E);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int rlx_redq_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, const rlx_mlp_desc* qdesc,
                        float* qparams, float* qm, float* qv, float* qtarget, float* log_alpha, float* am, float* av, const float* states,
                        const float* next_states, const float* actions, const float* rewards, const float* terminations, int64_t B,
                        uint32_t key_io[2], int scheme, int64_t* q_opt_count_io, int64_t* pi_opt_count_io, const rlx_redq_hparams* hp,
                        float* metrics_out, int32_t* subsets_out, void* stream) {
  // one key per row: keys[2 + b] of B + 2 in a critic step, keys[1 + b] of B + 1 in the policy step; plain ReLU critics, no dropout
  const RedqLoopSpec spec{"rlx_redq_update_f32", "redq", NORM_NONE, 0.f, 0.f, 1, "must be 1", 0, true, true, redq_check_hp_of, redq_critic_loss,
                          1u, 1u, {2u, 1u}, {0u, 0u}, {0u, 0u}, {1u, 1u}, {0u, 0u}};
  return redq_loop(ctx, spec, pdesc, pparams, pm, pv, qdesc, qparams, qm, qv, qtarget, log_alpha, am, av, states, next_states, actions,
                   rewards, terminations, B, key_io, scheme, q_opt_count_io, pi_opt_count_io, hp, metrics_out, subsets_out, stream);
}

}  // extern "C"
