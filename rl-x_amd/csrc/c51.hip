// c51.hip -- the distributional ("C51", categorical) critic step of FastSAC: projected target distributions, double-Q selection,
// cross-entropy loss and its gradient w.r.t. the critics' logits, in one launch + one small reduction.
// Reference: rl_x/algorithms/fastsac/pytorch/fastsac.py:144-213 (closure critic_and_entropy_loss_fn); CPU twin: oracle/c51.py.
//
// One wave per sample (four samples per workgroup), lane <-> atom (two atoms per lane up to 128 atoms).  The projection is the
// reference's two index_add_ passes made deterministic: output bin i walks the source atoms j in ascending order and adds
// (u_j - b_j) p_j where l_j == i, then (b_j - l_j) p_j where u_j == i -- the order a sequential index_add_ produces, with no atomics.
// The row's arithmetic is c51_body.h's c51_row, which fastmpo.hip instantiates too.
#include "c51_body.h"

namespace rlx {

// FastSAC's instantiation of c51_row: two critics, one softmax per target critic, the entropy term, ties go to the second
__global__ __launch_bounds__(256) void k_c51_loss(C51Args a, float* __restrict__ loss_b, float* __restrict__ v1_b) {
  __shared__ float s_p[4][2][C51_MAXA], s_w[4][2][C51_MAXA];
  __shared__ int s_lu[4][2][C51_MAXA];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  if (b >= a.B) return;                                 // (whole waves leave: no workgroup barrier below)
  float v[2];
  const float loss = c51_row<2, false, true>(a, b, lane, s_p[w], s_w[w], s_lu[w], v);
  if (lane == 0) {
    loss_b[b] = loss;
    v1_b[b] = v[0];
  }
}

// out = {mean_b loss_b (= q1_loss + q2_loss), min_b v1, max_b v1, 0}; one workgroup, fixed order
__global__ __launch_bounds__(256) void k_c51_finish(const float* __restrict__ loss_b, const float* __restrict__ v1_b, int64_t B,
                                                    float* __restrict__ out) {
  __shared__ double s_s[256];
  __shared__ float s_mn[256], s_mx[256];
  double s = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = threadIdx.x; i < B; i += 256) {
    s += (double)loss_b[i];
    mn = fminf(mn, v1_b[i]);
    mx = fmaxf(mx, v1_b[i]);
  }
  s_s[threadIdx.x] = s; s_mn[threadIdx.x] = mn; s_mx[threadIdx.x] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s_s[threadIdx.x] += s_s[threadIdx.x + o];
      s_mn[threadIdx.x] = fminf(s_mn[threadIdx.x], s_mn[threadIdx.x + o]);
      s_mx[threadIdx.x] = fmaxf(s_mx[threadIdx.x], s_mx[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(s_s[0] / (double)B);
    out[1] = s_mn[0];
    out[2] = s_mx[0];
    out[3] = 0.f;
  }
}

}  // namespace rlx

extern "C" {

int rlx_c51_critic_loss_f32(rlx_ctx* ctx, const float* q1_logits, const float* q2_logits, const float* q1_next_logits,
                            const float* q2_next_logits, const float* rewards, const float* dones, const float* truncations,
                            const float* effective_n_steps, const float* next_log_probs, const float* log_alpha, int64_t B,
                            int nr_atoms, float gamma, float v_min, float v_max, int clipped_double_q, float* d_q1_logits,
                            float* d_q2_logits, float* out4, void* stream) {
  RLX_REQUIRE(ctx && q1_logits && q2_logits && q1_next_logits && q2_next_logits && rewards && dones && truncations &&
                  effective_n_steps && next_log_probs && log_alpha && d_q1_logits && d_q2_logits && out4,
              RLX_EINVAL, "rlx_c51_critic_loss_f32: NULL pointer");
  RLX_REQUIRE(B > 0 && nr_atoms >= 2 && nr_atoms <= rlx::C51_MAXA && v_max > v_min, RLX_EINVAL,
              "rlx_c51_critic_loss_f32: need B > 0, 2 <= nr_atoms <= 128, v_max > v_min");
  hipStream_t st = (hipStream_t)stream;
  float* tmp = (float*)rlx::scratch(ctx, rlx::SL_STAGE, (size_t)2 * B * sizeof(float));
  if (!tmp) return RLX_ENOMEM;
  rlx::C51Args a{};
  a.q[0] = q1_logits; a.q[1] = q2_logits; a.qn[0] = q1_next_logits; a.qn[1] = q2_next_logits;
  a.dq[0] = d_q1_logits; a.dq[1] = d_q2_logits;
  a.rew = rewards; a.dones = dones; a.truncs = truncations; a.nsteps = effective_n_steps;
  a.nlogp = next_log_probs; a.log_alpha = log_alpha;
  a.B = B; a.NA = nr_atoms; a.K = 1; a.gamma = gamma; a.v_min = v_min; a.v_max = v_max;
  a.clipped = clipped_double_q; a.tie_first = 0;
  hipLaunchKernelGGL(rlx::k_c51_loss, dim3(rlx::div_up(B, 4)), dim3(256), 0, st, a, tmp, tmp + B);
  RLX_LAUNCH_CHECK();
  hipLaunchKernelGGL(rlx::k_c51_finish, dim3(1), dim3(256), 0, st, tmp, tmp + B, B, out4);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

}  // extern "C"
