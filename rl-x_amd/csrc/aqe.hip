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
// The update's body is redq.hip's redq_loop (redq_loop.h), whose header describes the schedule; rlx_aqe_update_f32 states the above as
// a RedqLoopSpec.  In the loop's words: the E targets' passes share one buffer set, k_aqe_target_loss stands where
// k_redq_critic_loss does, and the policy step's seed is k_ens_fill with k_ens_atom_rowsum for q_value.
//
// Networks: rlx_mlp_desc as tqc.hip takes them (ReLU, no LayerNorm; policy out_dim = 2 A; critics: E networks back to back, each
// in_dim = Oc + A, out_dim = H).  Q values are laid out [E][B][H], critic-major, as E head GEMMs leave them; flat index i = e H + h
// (`reshape(nr_total_q_values)`, aqe.py:165).  The value indexing (ens_atom) and the wave-level bitonic sort (ens_sort) are
// sac_ens.h's, shared with tqc.hip.
//
// Q values that are NaN are outside the contract, as in tqc.hip: the sort compares with fminf / fmaxf, which drop a NaN operand, so
// a row holding one loses it (and duplicates a neighbour) instead of propagating it.  +-inf values sort as values.
// CPU twin: tests/aqe_twin.py (float64).  The reference's AQE is JAX only; see DESIGN.md 4.5f for what is pinned.
#include "redq_loop.h"

namespace rlx {

constexpr int AQE_MAXT = 128;   // two values per lane of one wave (tqc.hip's cap)

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
static int aqe_check_hp(int E, int H, int dropped, int G) {
  RLX_REQUIRE(E >= 1, RLX_EINVAL, "aqe: hp->ensemble_size must be at least 1");
  RLX_REQUIRE(E <= REDQ_MAXE, RLX_EUNSUP, "aqe: hp->ensemble_size at most 16");
  RLX_REQUIRE(H >= 1, RLX_EINVAL, "aqe: hp->nr_heads_per_net must be at least 1");
  RLX_REQUIRE((int64_t)E * H <= AQE_MAXT, RLX_EUNSUP, "aqe: hp->ensemble_size * hp->nr_heads_per_net (total q values) at most 128");
  RLX_REQUIRE(dropped >= 0 && dropped < E * H, RLX_EINVAL, "aqe: hp->nr_dropped_q_values must be in [0, ensemble_size * nr_heads_per_net)");
  RLX_REQUIRE(G >= 1, RLX_EINVAL, "aqe: hp->q_update_steps must be at least 1");
  RLX_REQUIRE(G <= REDQ_MAXG, RLX_EUNSUP, "aqe: hp->q_update_steps at most 64");
  return RLX_OK;
}
static int aqe_check_hp_of(const rlx_redq_hparams& hp, const RedqLoopSpec& spec) {   // as RedqLoopSpec::check_hp
  return aqe_check_hp(hp.ensemble_size, spec.heads, spec.dropped, hp.q_update_steps);
}

// every target is evaluated: n.M = n.E, T = E H values per transition on either side
static int aqe_target_loss(const float* q, const float* qn, const float* rew, const float* term, const float* nlogp, const float* log_alpha,
                           int64_t B, const RedqLossDims& n, float gamma, float* y, float* dq, float* loss_row, float* loss_out, hipStream_t st) {
  hipLaunchKernelGGL(k_aqe_target_loss, dim3(div_up(B, 4)), dim3(256), 0, st, q, qn, rew, term, nlogp, log_alpha, y, dq, loss_row, B, n.H,
                     n.E * n.H, n.K, gamma);
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
  const int E = hp->ensemble_size, H = hp->nr_heads_per_net;
  const int rc = aqe_check_hp(E, H, hp->nr_dropped_q_values, hp->q_update_steps);
  if (rc) return rc;
  const int T = E * H;
  hipStream_t st = (hipStream_t)stream;
  float* loss_row = nullptr;
  if (loss_out) {
    loss_row = (float*)scratch(ctx, SL_STAGE, a64((size_t)B) * sizeof(float));
    if (!loss_row) return RLX_ENOMEM;
  }
  int rc2 = aqe_target_loss(q, q_next, rewards, terminations, next_logp, log_alpha, B, RedqLossDims{E, H, E, T - hp->nr_dropped_q_values},
                            hp->gamma, y_out, dq_out, loss_row, loss_out, st);
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
  RLX_REQUIRE(hp, RLX_EINVAL, "rlx_aqe_update_f32: NULL pointer");
  const rlx_redq_hparams rhp{hp->gamma, hp->tau, hp->target_entropy, hp->log_std_min, hp->log_std_max, hp->lr_policy, hp->lr_critic,
                             hp->lr_critic_delta, hp->lr_alpha, hp->adam_b1, hp->adam_b2, hp->adam_eps, hp->ensemble_size,
                             hp->ensemble_size, hp->q_update_steps, hp->critic_states, hp->critic_next_states};
  // H outputs per critic; every target, in index order: no sample_key, one key per row at keys[1 + b] of B + 1 in every step; the
  // policy ascends the mean over all T values; no dropout
  const RedqLoopSpec spec{"rlx_aqe_update_f32", "aqe", NORM_NONE, 0.f, 0.f, hp->nr_heads_per_net, "must equal hp->nr_heads_per_net",
                          hp->nr_dropped_q_values, false, false, aqe_check_hp_of, aqe_target_loss, 1u, 1u,
                          {1u, 1u}, {0u, 0u}, {0u, 0u}, {1u, 1u}, {0u, 0u}};
  return redq_loop(ctx, spec, pdesc, pparams, pm, pv, qdesc, qparams, qm, qv, qtarget, log_alpha, am, av, states, next_states, actions,
                   rewards, terminations, B, key_io, scheme, q_opt_count_io, pi_opt_count_io, &rhp, metrics_out, nullptr, stream);
}

}  // extern "C"
