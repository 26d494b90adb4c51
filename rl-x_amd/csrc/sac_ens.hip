// sac_ens.hip -- the kernels tqc.hip, redq.hip and aqe.hip share (sac_ens.h declares their launchers): the tanh-Gaussian sample of
// the update, the policy's head gradient, a fixed-order mean, the metrics with the entropy coefficient's Adam step, and -- for the
// critics with several outputs (tqc.hip, aqe.hip) -- the row sum over all of a transition's values and a constant fill.
#include "sac_ens.h"

namespace rlx {

// tanh-Gaussian sample of the update from the policy's head output [B, 2A], built from sac_sample.h as k_sac_sample is, with the
// row's own noise key (EnsRowKeys).  One thread per (row, action dim); a row's log-prob terms meet in LDS and one lane adds them in
// index order.  Dynamic LDS: (256 / AP) A floats.
__global__ __launch_bounds__(256) void k_ens_sample(const float* __restrict__ head, SacSampleArgs sa, int64_t B, int AP, uint32_t base,
                                                    uint32_t stride, uint32_t count) {
  extern __shared__ float s_term[];
  const int A = sa.A;
  const int rpb = 256 / AP;
  const int rl = threadIdx.x / AP, jl = threadIdx.x - rl * AP;
  const int64_t i = (int64_t)blockIdx.x * rpb + rl;
  if (i < B) {
    uint32_t s0, s1;
    split_key_at(sa.k0, sa.k1, base + stride * (uint32_t)i, count, sa.scheme, s0, s1);
    for (int j = jl; j < A; j += AP) s_term[rl * A + j] = sac_sample_elem(sa, s0, s1, i, j, head[i * 2 * A + j], head[i * 2 * A + A + j]);
  }
  __syncthreads();
  if (i < B && jl == 0) {
    float lp = 0.f;
    for (int j = 0; j < A; ++j) lp += s_term[rl * A + j];
    sa.logp[i] = lp;
  }
}

// d L / d(head output) of the policy (tqc.py:173-185, redq.py:183-198), SAC's gradient with dQ/da summed over the E critics (da: E
// buffers of [B, ld_da], e_stride floats apart, action columns at col_off; each already carries its seed: TQC's -1 / (B T), REDQ's
// zero where the critic is not the row's minimum):
//   d_u = (alpha / B * 2a / (1 - a^2 + 1e-6) + sum_e dQ_e/da) (1 - a^2);  d_mean = d_u;
//   d_logstd = [raw inside the clip] (d_u std eps - alpha / B)
__global__ __launch_bounds__(256) void k_ens_policy_grad(const float* __restrict__ head, const float* __restrict__ xp, int ld, int col_off,
                                                         const float* __restrict__ da, int ld_da, int64_t e_stride, int E,
                                                         const float* __restrict__ log_alpha, EnsRowKeys keys, float* __restrict__ d_out,
                                                         int64_t B, int A, int AP, float ls_min, float ls_max,
                                                         const float* __restrict__ eps_inject) {
  const int rpb = 256 / AP;
  const int rl = threadIdx.x / AP, jl = threadIdx.x - rl * AP;
  const int64_t i = (int64_t)blockIdx.x * rpb + rl;
  if (i >= B) return;
  const float alpha = expf(log_alpha[0]);
  const int scheme = keys.scheme;
  uint32_t s0, s1;
  split_key_at(keys.k0, keys.k1, keys.base + keys.stride * (uint32_t)i, keys.count, scheme, s0, s1);
  const float invB = 1.0f / (float)B;
  for (int j = jl; j < A; j += AP) {
    const float raw = head[i * 2 * A + A + j];
    const float ls = fminf(fmaxf(raw, ls_min), ls_max);
    const float eps = eps_inject ? eps_inject[i * A + j] : normal_from_bits(random_bits_at(s0, s1, (uint64_t)j, (uint64_t)A, scheme));
    const float a = xp[i * ld + col_off + j];
    const float om = 1.0f - a * a;
    float dqa = 0.f;
    for (int e = 0; e < E; ++e) dqa += da[e * e_stride + i * ld_da + col_off + j];
    const float du = (alpha * invB * 2.0f * a / (om + 1e-6f) + dqa) * om;
    d_out[i * 2 * A + j] = du;
    const bool inside = raw > ls_min && raw < ls_max;
    d_out[i * 2 * A + A + j] = inside ? du * expf(ls) * eps - alpha * invB : 0.f;
  }
}

// sum of v[0 .. n) over one workgroup: double accumulators, fixed order, no atomics
__device__ __forceinline__ double ens_block_sum(const float* __restrict__ v, int64_t n, double* s_buf) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)v[i];
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
__global__ __launch_bounds__(256) void k_ens_mean(const float* __restrict__ v, int64_t n, float* __restrict__ out) {
  __shared__ double s_buf[256];
  const double s = ens_block_sum(v, n, s_buf);
  if (threadIdx.x == 0) out[0] = (float)(s / (double)n);
}

// metrics (rlx_sac_update_f32's order) and the entropy coefficient's gradient with its plain Adam step (tqc.py:188, :220;
// redq.py:201, :253; the arithmetic of adam_body.h's adam_element without clipping).  q_row: per row the sum of TQC's T atoms
// (q_div = E B N), of AQE's T heads (q_div = B T) or REDQ's min over the E critics (q_div = B) on (s, a~); lpc: logp [B].
// steps != NULL (REDQ, AQE): [G] q_loss then [G] gradient norm of the critic steps, added in index order (redq.py:244).
__global__ __launch_bounds__(256) void k_ens_finish(const float* __restrict__ q_row, int64_t q_div, const float* __restrict__ lpc, int64_t B,
                                                    const float* __restrict__ steps, int G, float* __restrict__ log_alpha,
                                                    float* __restrict__ am, float* __restrict__ av, float* __restrict__ metrics,
                                                    float target_entropy, float lr, float bc1, float bc2, float b1, float b2, float eps) {
  __shared__ double s_buf[256];
  const double sq = ens_block_sum(q_row, B, s_buf);
  const double sl = ens_block_sum(lpc, B, s_buf);
  if (threadIdx.x != 0) return;
  if (steps) {
    double ql = 0.0, gn = 0.0;
    for (int i = 0; i < G; ++i) {
      ql += (double)steps[i];
      gn += (double)steps[G + i];
    }
    metrics[0] = (float)(ql / (double)G);                   // loss/q_loss: mean over the G steps
    metrics[7] = (float)(gn / (double)G);                   // gradients/critic_grad_norm: mean over the G steps
  }
  const float mean_q = (float)(sq / (double)q_div), mean_lp = (float)(sl / (double)B);
  const float la = log_alpha[0];
  const float alpha = expf(la);
  const float entropy = -mean_lp;
  const float ga = alpha * (entropy - target_entropy);      // d mean(alpha_g (entropy - target)) / d log_alpha
  metrics[1] = alpha * mean_lp - mean_q;                    // loss/policy_loss
  metrics[2] = ga;                                          // loss/entropy_loss
  metrics[3] = entropy;                                     // entropy/entropy
  metrics[4] = alpha;                                       // entropy/alpha
  metrics[5] = mean_q;                                      // q_value/q_value
  metrics[8] = sqrtf(ga * ga);                              // gradients/entropy_grad_norm
  metrics[9] = 0.f;
  const float mi = fmaf(b1, am[0], (1.f - b1) * ga);
  const float vi = fmaf(b2, av[0], ((1.f - b2) * ga) * ga);
  am[0] = mi;
  av[0] = vi;
  log_alpha[0] = fmaf(-lr, (mi / bc1) / (sqrtf(vi / bc2) + eps), la);
}

// row_sum[b] = sum of the row's T values (one wave per transition): the policy loss's mean over all atoms / heads, per row
__global__ __launch_bounds__(256) void k_ens_atom_rowsum(const float* __restrict__ atoms, float* __restrict__ row_sum, int64_t B, int N, int T) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  if (b >= B) return;                                   // (whole waves leave: no workgroup barrier below)
  const float v = wave_sum((lane < T ? ens_atom(atoms, b, lane, B, N) : 0.f) + (lane + 64 < T ? ens_atom(atoms, b, lane + 64, B, N) : 0.f));
  if (lane == 0) row_sum[b] = v;
}

__global__ __launch_bounds__(256) void k_ens_fill(float* __restrict__ out, int64_t n, float v) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- launchers
int ens_atom_rowsum(const float* atoms, float* row_sum, int64_t B, int N, int T, hipStream_t st) {
  hipLaunchKernelGGL(k_ens_atom_rowsum, dim3(div_up(B, 4)), dim3(256), 0, st, atoms, row_sum, B, N, T);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int ens_fill(float* out, int64_t n, float v, hipStream_t st) {
  hipLaunchKernelGGL(k_ens_fill, dim3(elem_grid(n)), dim3(256), 0, st, out, n, v);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int ens_sample(const float* head, SacSampleArgs sa, const EnsRowKeys& keys, int64_t B, hipStream_t st) {
  const int AP = ens_lanes_per_row(sa.A);
  sa.k0 = keys.k0; sa.k1 = keys.k1; sa.scheme = keys.scheme;
  hipLaunchKernelGGL(k_ens_sample, dim3(div_up(B, 256 / AP)), dim3(256), (size_t)(256 / AP) * sa.A * sizeof(float), st, head, sa, B, AP,
                     keys.base, keys.stride, keys.count);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int ens_policy_grad(const float* head, const float* xp, int ld, int col_off, const float* da, int ld_da, int64_t e_stride, int E,
                    const float* log_alpha, const EnsRowKeys& keys, float* d_out, int64_t B, int A, float ls_min, float ls_max,
                    const float* eps_inject, hipStream_t st) {
  const int AP = ens_lanes_per_row(A);
  hipLaunchKernelGGL(k_ens_policy_grad, dim3(div_up(B, 256 / AP)), dim3(256), 0, st, head, xp, ld, col_off, da, ld_da, e_stride, E, log_alpha,
                     keys, d_out, B, A, AP, ls_min, ls_max, eps_inject);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int ens_mean(const float* v, int64_t n, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_ens_mean, dim3(1), dim3(256), 0, st, v, n, out);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int ens_finish(const float* q_row, int64_t q_div, const float* lpc, int64_t B, const float* steps, int G, float* log_alpha, float* am,
               float* av, float* metrics, float target_entropy, const float sched[3], float b1, float b2, float eps, hipStream_t st) {
  hipLaunchKernelGGL(k_ens_finish, dim3(1), dim3(256), 0, st, q_row, q_div, lpc, B, steps, G, log_alpha, am, av, metrics, target_entropy,
                     sched[0], sched[1], sched[2], b1, b2, eps);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

}  // namespace rlx
