// c51_body.h -- the categorical ("C51") critic step of one batch row as a device function: the l / u / weight tables, the ordered
// two-pass projection, the expectations, the clipped choice and the cross-entropy with its logit gradient.  One implementation,
// instantiated by k_c51_loss (c51.hip: FastSAC, fastsac.py:144-213) and by k_fm_critic_loss (fastmpo.hip: FastMPO,
// fastmpo.py:314-379).
//
// One wave per row, lane <-> atom (two atoms per lane up to 128 atoms).  The projection is the reference's two scatter-add passes
// made deterministic: output bin i walks the source atoms j in ascending order and adds (u_j - b_j) p_j where l_j == i, then
// (b_j - l_j) p_j where u_j == i -- the order a sequential index_add_ produces, with no atomics.  The l / u / weight tables are
// shared by the E target networks (they depend on the transition only).
#pragma once
#include "common.h"

namespace rlx {

constexpr int C51_MAXA = 128;

__device__ __forceinline__ float c51_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float c51_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// softmax / log-softmax of one row held two atoms per lane (x0: atom lane, x1: atom lane + 64; absent atoms = -inf)
__device__ __forceinline__ void c51_softmax2(float x0, float x1, float& p0, float& p1, float& lse) {
  const float m = c51_wave_max(fmaxf(x0, x1));
  const float e0 = expf(x0 - m), e1 = expf(x1 - m);
  const float s = c51_wave_sum(e0 + e1);
  p0 = e0 / s;
  p1 = e1 / s;
  lse = m + logf(s);
}

// torch.linspace(v_min, v_max, NA)[j]: start + j * step for the first half, end - (NA - 1 - j) * step for the second
__device__ __forceinline__ float c51_support(float v_min, float v_max, int NA, int j) {
  const float step = (v_max - v_min) / (float)(NA - 1);
  return j < NA / 2 ? v_min + step * (float)j : v_max - step * (float)(NA - 1 - j);
}

struct C51Args {
  const float* q[2];     // the online critics' logits [B, NA]
  const float* qn[2];    // the target critics' logits: [B, NA], or with KMEAN [K B, NA] (sample k of row b at k B + b)
  float* dq[2];          // d loss / d q
  const float *rew, *dones, *truncs, *nsteps;
  const float *nlogp, *log_alpha;   // the entropy term's operands (ENTROPY only)
  int64_t B;
  int NA, K;
  float gamma, v_min, v_max;
  int clipped;           // every critic takes the projection whose expectation is smaller (E == 2)
  int tie_first;         // the first projection wins a tie (fastmpo.py:359 `<=`; fastsac.py:196 `<`)
};

// Row b of the step.  E: number of critics; KMEAN: the target pmf is the mean over K softmaxes instead of one softmax per critic;
// ENTROPY: the reward carries -discount alpha next_log_prob.  s_p [E][C51_MAXA], s_w [2][C51_MAXA], s_lu [2][C51_MAXA]: this wave's
// LDS.  Returns the row's loss (the sum over critics) and leaves each projection's expectation in v.
template <int E, bool KMEAN, bool ENTROPY>
__device__ __forceinline__ float c51_row(const C51Args& a, int64_t b, int lane, float (*s_p)[C51_MAXA], float (*s_w)[C51_MAXA],
                                         int (*s_lu)[C51_MAXA], float (&v)[E]) {
  const int NA = a.NA;
  const float v_min = a.v_min, v_max = a.v_max;
  const float ninf = -INFINITY;
  const int j0 = lane, j1 = lane + 64;
  const bool h0 = j0 < NA, h1 = j1 < NA;
  // ---- next-state distributions of the target networks
  float pn[E][2];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    float lse;
    if (KMEAN) {
      pn[e][0] = pn[e][1] = 0.f;
      for (int k = 0; k < a.K; ++k) {
        const float* row = a.qn[e] + ((int64_t)k * a.B + b) * NA;
        float p0, p1;
        c51_softmax2(h0 ? row[j0] : ninf, h1 ? row[j1] : ninf, p0, p1, lse);
        pn[e][0] += p0;
        pn[e][1] += p1;
      }
      pn[e][0] = pn[e][0] / (float)a.K;
      pn[e][1] = pn[e][1] / (float)a.K;
    } else {
      c51_softmax2(h0 ? a.qn[e][b * NA + j0] : ninf, h1 ? a.qn[e][b * NA + j1] : ninf, pn[e][0], pn[e][1], lse);
    }
  }
  // ---- where every atom of the support lands (fastsac.py:147-162, fastmpo.py:325-343)
  const float delta_z = (v_max - v_min) / (float)(NA - 1);
  const float bootstrap = 1.0f - a.dones[b] * (1.0f - a.truncs[b]);
  const float discount = powf(a.gamma, a.nsteps[b]) * bootstrap;
  float r = a.rew[b];
  if (ENTROPY) r = a.rew[b] - discount * expf(a.log_alpha[0]) * a.nlogp[b];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const int j = hh ? j1 : j0;
    if (j < NA) {
      const float z = c51_support(v_min, v_max, NA, j);
      const float tz = fminf(fmaxf(r + discount * z, v_min), v_max);
      const float bb = (tz - v_min) / delta_z;
      int l = (int)floorf(bb), u = (int)ceilf(bb);
      const bool is_int = l == u;
      const bool lm = is_int && l > 0, um = is_int && l == 0;
      if (lm) l -= 1;
      if (um) u += 1;
      s_lu[0][j] = l;
      s_lu[1][j] = u;
      s_w[0][j] = (float)u - bb;
      s_w[1][j] = bb - (float)l;
#pragma unroll
      for (int e = 0; e < E; ++e) s_p[e][j] = pn[e][hh];
    }
  }
  // (same-wave LDS writes are visible to the wave's later reads: no barrier)
  // ---- projection: bin i collects in the order of a sequential index_add_
  float t[E][2];
#pragma unroll
  for (int e = 0; e < E; ++e) t[e][0] = t[e][1] = 0.f;
  for (int pass = 0; pass < 2; ++pass)
    for (int j = 0; j < NA; ++j) {
      const int tgt = s_lu[pass][j];
      const float wj = s_w[pass][j];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float ae = s_p[e][j] * wj;
        if (tgt == j0) t[e][0] += ae;
        if (tgt == j1) t[e][1] += ae;
      }
    }
  // ---- expectations and the double-Q selection (fastsac.py:192-201, fastmpo.py:356-363)
  const float z0 = c51_support(v_min, v_max, NA, j0), z1 = c51_support(v_min, v_max, NA, j1);
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = c51_wave_sum((h0 ? t[e][0] * z0 : 0.f) + (h1 ? t[e][1] * z1 : 0.f));
  if (E == 2 && a.clipped) {
    const bool first = a.tie_first ? v[0] <= v[E - 1] : v[0] < v[E - 1];
    const float c0 = first ? t[0][0] : t[E - 1][0], c1 = first ? t[0][1] : t[E - 1][1];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      t[e][0] = c0;
      t[e][1] = c1;
    }
  }
  // ---- cross-entropy against the online critics' logits and its gradient (fastsac.py:203-209, fastmpo.py:366-369)
  float loss = 0.f;
  const float invB = 1.0f / (float)a.B;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float* q = a.q[e];
    float* dq = a.dq[e];
    const float x0 = h0 ? q[b * NA + j0] : ninf, x1 = h1 ? q[b * NA + j1] : ninf;
    float s0, s1, lz;
    c51_softmax2(x0, x1, s0, s1, lz);
    const float tsum = c51_wave_sum((h0 ? t[e][0] : 0.f) + (h1 ? t[e][1] : 0.f));
    loss += c51_wave_sum((h0 ? -t[e][0] * (x0 - lz) : 0.f) + (h1 ? -t[e][1] * (x1 - lz) : 0.f));
    if (h0) dq[b * NA + j0] = (s0 * tsum - t[e][0]) * invB;
    if (h1) dq[b * NA + j1] = (s1 * tsum - t[e][1]) * invB;
  }
  return loss;
}

}  // namespace rlx
