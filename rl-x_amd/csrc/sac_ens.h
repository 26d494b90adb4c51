// sac_ens.h -- what tqc.hip, redq.hip, aqe.hip and droq.hip share: SAC's tanh-Gaussian policy and entropy coefficient over an ensemble of E
// ReLU critics (plain; droq.hip's with Dropout and LayerNorm in every hidden block) on net_pass.h.  The kernels and their launchers are in sac_ens.hip; here are their declarations, the device
// helpers of the multi-output critics (value indexing, the wave-level bitonic sort) and the host helpers of an entry point: the
// descriptor rules, the shapes of a call, host key splitting, and the policy pass that ends in a sample.  An algorithm's file keeps
// its critic target and loss and its hyper-parameter check; the arena carve and the schedule are tqc.hip's own and, for the other three,
// redq.hip's redq_loop (redq_loop.h).
// (td3.hip, whose policy is deterministic, takes the descriptor rules -- det_prologue -- the row keys and the host key split only.)
#pragma once
#include "net_pass.h"
#include "sac_sample.h"

namespace rlx {

// the noise key of row i: split((k0, k1), count)[base + stride * i].  TQC is SAC's schedule 0 (sac_sample.h): (1 or 2, 2, 2B + 1);
// REDQ: (2, 1, B + 2) in a critic step, (1, 1, B + 1) in the policy step.  AQE: (1, 1, B + 1) in every step.  DroQ: (2, 3, 3B + 2)
// and (1, 2, 2B + 1); its dropout keys sit beside them (redq_loop.h, net_pass.h: DropKeys).
struct EnsRowKeys { uint32_t k0, k1; int scheme; uint32_t base, stride, count; };

// ---- sac_ens.hip
// tanh-Gaussian sample from the policy's head output [B, 2A] (sa: where the action and logp go, the clip, the injected noise; its
// mode stays non-zero: sac_sample.h's per-row noise form; its key fields are taken from `keys`)
int ens_sample(const float* head, SacSampleArgs sa, const EnsRowKeys& keys, int64_t B, hipStream_t st);
// d L / d(head output) of the policy from the action in xp [B, ld] at col_off and the E critics' input gradients da (E buffers of
// [B, ld_da], e_stride floats apart, each carrying its seed); keys: those of the sample that drew the action
int ens_policy_grad(const float* head, const float* xp, int ld, int col_off, const float* da, int ld_da, int64_t e_stride, int E,
                    const float* log_alpha, const EnsRowKeys& keys, float* d_out, int64_t B, int A, float ls_min, float ls_max,
                    const float* eps_inject, hipStream_t st);
// out[0] = mean of v[0 .. n): double accumulators, fixed order
int ens_mean(const float* v, int64_t n, float* out, hipStream_t st);
// metrics[1..5], [8], [9] (rlx_sac_update_f32's order) and the entropy coefficient's plain Adam step.  q_row: per row the summary of
// the critics on (s, a~), whose sum over q_div is q_value; lpc: logp [B].  steps != NULL: [G] q_loss then [G] critic gradient
// norm, whose means go to metrics[0] and [7]; NULL leaves those two alone.
int ens_finish(const float* q_row, int64_t q_div, const float* lpc, int64_t B, const float* steps, int G, float* log_alpha, float* am,
               float* av, float* metrics, float target_entropy, const float sched[3], float b1, float b2, float eps, hipStream_t st);
// row_sum[b] = sum of the row's T = E N values (atoms [E, B, N], T <= 128; one wave per transition, fixed order)
int ens_atom_rowsum(const float* atoms, float* row_sum, int64_t B, int N, int T, hipStream_t st);
// out[0 .. n) = v
int ens_fill(float* out, int64_t n, float v, hipStream_t st);

// ---- device helpers of the multi-output critics (tqc.hip's atoms, aqe.hip's heads)
// Value i = e N + n of row b lives at atoms[(e B + b) N + n]: critic-major, as E head GEMMs leave them.
__device__ __forceinline__ int64_t ens_atom_index(int64_t b, int i, int64_t B, int N) {
  const int e = i / N;
  return ((int64_t)e * B + b) * N + (i - e * N);
}
__device__ __forceinline__ float ens_atom(const float* __restrict__ atoms, int64_t b, int i, int64_t B, int N) {
  return atoms[ens_atom_index(b, i, B, N)];
}

// Ascending bitonic sort of up to 128 values held two per lane: element index = lane + 64 slot.  Stages with a partner distance
// below 64 exchange across lanes (__shfl_xor), the one stage at distance 64 exchanges the lane's own two slots.  Values only.
template <int SLOTS>
__device__ __forceinline__ void ens_sort(float (&v)[2], int lane) {
#pragma unroll
  for (int k = 2; k <= 64 * SLOTS; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j == 64) {   // (k == 128 only: every index has bit 7 clear, so the merge is ascending)
        const float lo = fminf(v[0], v[1]), hi = fmaxf(v[0], v[1]);
        v[0] = lo;
        v[1] = hi;
      } else {
        const bool lower = (lane & j) == 0;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
          const float o = __shfl_xor(v[s], j, 64);
          const bool asc = ((lane + 64 * s) & k) == 0;
          v[s] = (asc == lower) ? fminf(v[s], o) : fmaxf(v[s], o);
        }
      }
    }
  }
}

// ---- host helpers
// the networks these algorithms take: 1..3 plain ReLU blocks; algo: "tqc" / "redq" / "aqe", which: "pdesc" / "qdesc"
static inline int ens_check_net(const rlx_mlp_desc& d, const char* algo, const char* which) {
  const std::string who = std::string(algo) + ": " + which;
  RLX_REQUIRE(d.n_hidden >= 1 && d.n_hidden <= 3 && d.in_dim > 0 && d.out_dim > 0, RLX_EINVAL,
              who + " needs 1..3 hidden layers and positive widths");
  RLX_REQUIRE(d.act == RLX_ACT_RELU && !d.ln_first && !d.has_logstd, RLX_EINVAL,
              who + " must be act = RLX_ACT_RELU, ln_first = 0, has_logstd = 0");
  for (int l = 0; l < d.n_hidden; ++l)
    RLX_REQUIRE(d.hidden[l] > 0 && d.hidden[l] % 64 == 0 && d.hidden[l] <= 1024, RLX_EUNSUP,
                who + " hidden widths must be multiples of 64, at most 1024");
  return RLX_OK;
}
static inline Chain ens_layout(const rlx_mlp_desc& d) { return make_chain(d.in_dim, d.hidden, d.n_hidden, d.out_dim, NORM_NONE, RLX_ACT_RELU); }

// threads that share a row in the sample and policy-gradient kernels: the power of two at or above A, at most 64
static inline int ens_lanes_per_row(int A) {
  int ap = 1;
  while (ap < A && ap < 64) ap <<= 1;
  return ap;
}

struct PlainAdamHp { float max_grad_norm, adam_b1, adam_b2, adam_eps; };   // what torch_clip_adam reads; max_grad_norm <= 0: plain Adam

// jax.random.split(key, num)[i] on the host (out may be key: split_key_at takes the key words by value)
static inline void split_at_host(const uint32_t key[2], uint32_t i, uint32_t num, int scheme, uint32_t out[2]) {
  split_key_at(key[0], key[1], i, num, scheme, out[0], out[1]);
}

// the shapes of one update call: act_dim, the policy's and the critics' observation widths, the row strides of the critic and
// policy inputs, and the critics' observations (the sample kernels' launchers size their own grids)
struct EnsDims {
  int A, Op, Oc, ldc, ldp;
  const float *cs, *cn;
};
// the rules below the policy head's, at act_dim A
static inline int ens_dims(const std::string& f, int A, const rlx_mlp_desc& pd, const rlx_mlp_desc& qd, int q_out, const char* q_out_rule,
                           const float* states, const float* next_states, const float* critic_states, const float* critic_next_states,
                           EnsDims* d) {
  RLX_REQUIRE(qd.out_dim == q_out, RLX_EINVAL, f + ": qdesc->out_dim " + q_out_rule);
  RLX_REQUIRE(qd.in_dim > A, RLX_EINVAL, f + ": qdesc->in_dim must be critic obs + act_dim");
  const int Op = pd.in_dim, Oc = qd.in_dim - A;
  const bool asym = critic_states != nullptr;
  RLX_REQUIRE((critic_states != nullptr) == (critic_next_states != nullptr) && (asym || Oc == Op), RLX_EINVAL,
              f + ": critic obs width != policy obs width needs hp->critic_states AND hp->critic_next_states");
  *d = EnsDims{A, Op, Oc, (Oc + A + 3) & ~3, (Op + 3) & ~3, asym ? critic_states : states, asym ? critic_next_states : next_states};
  return RLX_OK;
}
// The descriptor rules that tie the policy to the critics, under the entry point's name fn; q_out / q_out_rule: the critics' output
// width and how the message states it.  critic_states / critic_next_states: hp's (both or neither).
static inline int ens_prologue(const char* fn, const rlx_mlp_desc& pd, const rlx_mlp_desc& qd, int q_out, const char* q_out_rule,
                               const float* states, const float* next_states, const float* critic_states,
                               const float* critic_next_states, EnsDims* d) {
  const std::string f(fn);
  RLX_REQUIRE(pd.out_dim % 2 == 0, RLX_EINVAL, f + ": pdesc->out_dim must be 2 * act_dim");
  const int A = pd.out_dim / 2;
  RLX_REQUIRE(A <= 64, RLX_EUNSUP, f + ": act_dim (pdesc->out_dim / 2) at most 64");
  return ens_dims(f, A, pd, qd, q_out, q_out_rule, states, next_states, critic_states, critic_next_states, d);
}
// The same for a deterministic policy (td3.hip): the head is the action's pre-activation, out_dim == act_dim, no log-std half
static inline int det_prologue(const char* fn, const rlx_mlp_desc& pd, const rlx_mlp_desc& qd, const float* states, const float* next_states,
                               const float* critic_states, const float* critic_next_states, EnsDims* d) {
  const std::string f(fn);
  RLX_REQUIRE(pd.out_dim >= 1 && pd.out_dim <= 64, RLX_EUNSUP, f + ": act_dim (pdesc->out_dim) must be in 1..64");
  return ens_dims(f, pd.out_dim, pd, qd, 1, "must be 1", states, next_states, critic_states, critic_next_states, d);
}
// the fields of SacSampleArgs that hold for a whole call
static inline SacSampleArgs ens_sample_args(const EnsDims& d, float ls_min, float ls_max, int64_t B) {
  SacSampleArgs sa;
  sa.mode = 1; sa.ld_out = d.ldc; sa.col_off = d.Oc; sa.A = d.A;
  sa.ls_min = ls_min; sa.ls_max = ls_max; sa.N_global = B;
  return sa;
}
// The policy on pobs, sampled into a critic input: xq [B, ldc] = [cobs | a ~ pi(pobs) | 0], logp [B].  xs [B, ldp], bp and h
// [B, 2A] keep the policy's input, activations and head output for its backward.
static inline int ens_policy_sample(rlx_ctx* ctx, const EnsDims& d, const Chain& LP, const float* pparams, const float* cobs,
                                    const float* pobs, float* xq, float* xs, const ChainBufs& bp, float* h, float* logp, SacSampleArgs sa,
                                    const EnsRowKeys& keys, const float* eps_inject, int64_t B, hipStream_t st) {
  int rc = fs_concat(cobs, d.Oc, nullptr, d.A, xq, d.ldc, B, st);
  if (!rc) rc = fs_concat(pobs, d.Op, nullptr, 0, xs, d.ldp, B, st);
  if (!rc) rc = chain_fwd(ctx, LP, pparams, xs, d.ldp, bp, h, B, st);
  if (rc) return rc;
  sa.act_out = xq; sa.logp = logp; sa.eps_inject = eps_inject;
  return ens_sample(h, sa, keys, B, st);
}

}  // namespace rlx
