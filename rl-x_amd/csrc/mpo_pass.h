// mpo_pass.h -- the kernels of mpo.hip that fastmpo.hip runs too, behind host launchers: the sample + first-layer kernel of a target
// critic, the E-step / M-step row kernel, the dual step, the input gather and the acting step.  One implementation each; MPO
// (mpo/pytorch) and FastMPO (fastmpo/flax_full_jit) differ in the arguments below.
#pragma once
#include "net_pass.h"

namespace rlx {

// fixed-order sum of x[i * stride] over i < n by one 256-thread workgroup (every thread gets the result); s_buf: 4 floats of LDS
__device__ __forceinline__ float mp_block_sum(const float* __restrict__ x, int64_t n, int64_t stride, float* s_buf) {
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += x[i * stride];
  acc = wave_sum(acc);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_buf[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (s_buf[0] + s_buf[1]) + (s_buf[2] + s_buf[3]);
}

// Which state row and which noise a target row t of k_mpo_sample_l1 reads: rows t < n0 take the stacked state row off0 + t % m0
// and the draw eps0[t]; rows t >= n0, u = t - n0, the row off1 + u % m1 and the draw eps1[u].
struct MpRowMap { int64_t n0, m0, off0, m1, off1; };

// The target critic's first layer for T sampled actions (one launch per critic): samp [T, A] and cost [T] may be NULL (a second
// critic's launch: the first one wrote them).  norm / act / eps: the first block's (LayerNorm, SiLU), (none, ReLU) or (LayerNorm,
// tanh); H a multiple of 64 up to what norm_act takes for that block: 768, 1024 (no norm), 512.
int mp_sample_l1(const float* thead, const float* eps0, const float* eps1, const float* Zobs, const float* Wa, const float* g,
                 const float* be, float* H1, float* samp, float* cost, const MpRowMap& map, int64_t T, int A, int H, float min_scale,
                 float init_scale, int clip, int norm, int act, float eps, hipStream_t st);

// Per-row outputs of the E-step kernel (R rows each); the KL terms are [R, A]; qmean (mean over the samples of q; may be NULL)
struct MpRowOut { float *lse_q, *e_q, *lse_p, *e_p, *pgm, *pgs, *smin, *smax, *klm, *kls, *qmean; };

struct MpEstepArgs {
  const float* tlogits[2];   // the E target critics' logits [S R, NA]
  int E, qmin;               // q of a sample: the critic's own (E 1), the min over critics (qmin) or their mean
  int alpha_mean_off;        // where alpha_mean's log lies in the duals: 1 + A (MPO computes it from log_alpha_stddev, mpo.py:202), 1 (FastMPO)
  const float *cost, *samp, *thead, *ohead, *duals;
  int64_t R;
  int S, A, NA;
  float v_min, v_max, min_scale, init_scale, feps;
  int clip;
};
int mp_estep(const MpEstepArgs& a, float* dhead, const MpRowOut& out, hipStream_t st);

struct MpDualArgs {
  float eps_np, eps_mu, eps_sigma, eps_pen, feps, log_s, max_norm, lr, b1, b2, adam_eps, bc1, bc2, min_log_temp, min_log_alpha;
  int clip;
  // variant 0: MPO (mpo.py:238-247) -- alpha_mean from log_alpha_stddev (log_alpha_mean has no gradient), torch's clip_grad_norm_ over
  // the duals that have a gradient, Adam, 17 metrics.  variant 1: FastMPO (fastmpo.py:427-457, :609-620) -- alpha_mean from
  // log_alpha_mean, optax.clip_by_global_norm, adamw with weight decay wd on all four duals, the 22 policy-step metrics.
  int variant = 0;
  float wd = 0.f, lr_policy = 0.f;
};
int mp_dual(const float* ce, const float* q, int64_t B, const MpRowOut& ro, int64_t R, int A, float* duals, float* dm, float* dv,
            const MpDualArgs& c, float* metrics, hipStream_t st);

// out[i, c] = src_i[idx ? idx[c] : c] for c < n_idx (src_i = s0 row i for i < B0, else s1 row i - B0), then the A action columns
// act[i] (clamped to [-1, 1] when clip) when act != NULL; zero up to the row pitch ld
int mp_gather(const float* s0, const float* s1, int64_t B0, int O, const int32_t* idx, int n_idx, const float* act, int A, int clip,
              float* out, int ld, int64_t M, hipStream_t st);
// action = mean + std eps (or mean) from the head [N, 2A]; processed = clamp when clip; then rescale 1: low + 0.5 (p + 1)(high - low),
// rescale 2 ("fastsac", fastmpo/flax_full_jit/policy.py:135-136): p * low[j] (low holds the action scale)
int mp_act(const float* head, const float* eps, int64_t N, int A, float min_scale, float init_scale, int deterministic, int clip,
           int rescale, const float* low, const float* high, float* action, float* proc, hipStream_t st);

// The acting pass both algorithms share: policy columns of obs [N, O] -> the chain LP -> head [N, 2A] -> mp_act.  key, subkey =
// split(key) unless deterministic or the draws are injected (rlx_dbg_set_sac_noise)
int mp_act_pass(rlx_ctx* ctx, const Chain& LP, const float* pparams, const float* obs, int O, const int32_t* pidx, uint32_t key_io[2],
                int scheme, float* action, float* proc, const float* low, const float* high, int64_t N, int deterministic, float min_scale,
                float init_scale, int clip, int rescale, hipStream_t st);

// the two networks of an update and the row pitches of their inputs (multiples of four floats, zero padded)
struct MpShape {
  Chain LP, LQ;
  int O, A, Op, Oc, NA, ldp, ldc, ldo;   // ldc: [critic obs | action] rows; ldo: critic obs only
};
static inline MpShape mp_shape(const Chain& LP, const Chain& LQ, int O, int Op, int Oc, int A, int NA) {
  MpShape s;
  s.LP = LP; s.LQ = LQ; s.O = O; s.A = A; s.Op = Op; s.Oc = Oc; s.NA = NA;
  s.ldp = (Op + 3) & ~3;
  s.ldc = (Oc + A + 3) & ~3;
  s.ldo = (Oc + 3) & ~3;
  return s;
}

}  // namespace rlx
