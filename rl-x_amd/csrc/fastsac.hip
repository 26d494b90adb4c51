// fastsac.hip -- FastSAC update steps (rl_x/algorithms/fastsac/pytorch/fastsac.py:105-241, :323-329): distributional (C51) twin
// critics, tanh-Gaussian policy with a tanh-mapped log-std and an action scale, AdamW, Polyak targets.
//
// Networks (policy.py:46-57, q_network.py:27-38): every hidden layer is Dense -> LayerNorm (torch: eps 1e-5) -> SiLU, then a
// Dense head -- rlx_lnmlp_desc.  They are composed from the library's GEMM stages (launch_gemm_fwd / stage_dx / stage_dw: the
// exact-fp32 MFMA engine below 4096 rows, the split-operand engine from there on -- trunk_images, net_pass.h), the dense-head
// kernels of dense_head.hip and the row-wise LayerNorm + activation kernels of ln_kernels.h (k_ln_act_wide: widths up to 768,
// eps argument, SiLU' from the recomputed pre-activation).  A network is a Chain of such blocks: its carve, forward, backward
// and stage-arena size, with the arena, grids and key splitting, are net_pass.h's, shared with fasttd3.hip, reppo.hip, mpo.hip
// and espo.hip; this file keeps the descriptor check, the losses and the update's streams.  CPU twin: oracle/fastsac.py,
// pinned by outputs of the reference's own modules and closures (tests/golden/reference_fastsac.npz).
//
// Noise: the reference draws with torch's CUDA generator (Normal.rsample), which no other implementation reproduces; the
// library uses its counter RNG (threefry, the key split per call like rlx_sac_*), and rlx_dbg_set_sac_noise injects a given
// eps for parity tests.
#include "net_pass.h"

namespace rlx {

constexpr float FS_LN_EPS = 1e-5f;          // torch.nn.LayerNorm default
constexpr float FS_LOG_SQRT_2PI = 0.91893853320467274178f;

static int ln_check(const rlx_lnmlp_desc& d) {
  RLX_REQUIRE(d.n_hidden >= 1 && d.n_hidden <= 4 && d.in_dim > 0 && d.out_dim > 0, RLX_EINVAL, "rlx_lnmlp_desc: 1..4 hidden layers, positive widths");
  for (int l = 0; l < d.n_hidden; ++l)
    RLX_REQUIRE(d.hidden[l] > 0 && d.hidden[l] % 64 == 0 && d.hidden[l] <= 768, RLX_EUNSUP,
                "rlx_lnmlp_desc: hidden widths must be multiples of 64, at most 768 (the LayerNorm kernel holds a row in one wave)");
  return RLX_OK;
}

static Chain ln_layout(const rlx_lnmlp_desc& d) {
  return make_chain(d.in_dim, d.hidden, d.n_hidden, d.out_dim, NORM_LAYER, RLX_ACT_SILU, FS_LN_EPS);
}

// ---------------------------------------------------------------------------------------------------------------- kernels
// (the dense heads and the [obs | action] concat: dense_head.hip)
// policy.get_action_and_log_prob (policy.py:75-90) from the head output [M, 2A] = [mean | raw log-std]: one thread per
// (row, action dim); the log-prob terms of a row are added in index order by one lane.  act_out: row stride ld, first column c0.
__global__ __launch_bounds__(256) void k_fs_sample(const float* __restrict__ head, const float* __restrict__ scale, uint32_t k0,
                                                   uint32_t k1, int scheme, const float* __restrict__ eps_inject,
                                                   float* __restrict__ act_out, int ld, int c0, float* __restrict__ logp, int64_t M,
                                                   int A, float ls_min, float ls_max, int deterministic, int64_t row_off,
                                                   int64_t M_global) {
  extern __shared__ float s_term[];   // [rows per block][A]
  const int rpb = 256 / A > 0 ? 256 / A : 1;
  const int rl = threadIdx.x / A, j = threadIdx.x - rl * A;
  const int64_t i = (int64_t)blockIdx.x * rpb + rl;
  const bool on = rl < rpb && i < M;
  if (on) {
    const float mean = head[i * 2 * A + j];
    const float ls = ls_min + 0.5f * (ls_max - ls_min) * (tanhf(head[i * 2 * A + A + j]) + 1.0f);
    const float sd = expf(ls);
    float eps = 0.f;
    if (!deterministic) {
      eps = eps_inject ? eps_inject[i * A + j]
                       : normal_from_bits(random_bits_at(k0, k1, (uint64_t)(i + row_off) * A + j, (uint64_t)M_global * A, scheme));
    }
    const float raw = mean + sd * eps;
    const float t = tanhf(raw);
    const float sc = scale[j];
    act_out[i * ld + c0 + j] = t * sc;
    const float d = raw - mean;
    s_term[rl * A + j] = -(d * d) / (2.0f * sd * sd) - ls - FS_LOG_SQRT_2PI - logf((1.0f - t * t) + 1e-6f) - logf(sc + 1e-6f);
  }
  if (!logp) return;
  __syncthreads();
  if (on && j == 0) {
    float lp = 0.f;
    for (int q = 0; q < A; ++q) lp += s_term[rl * A + q];
    logp[i] = lp;
  }
}

// policy loss seeds (fastsac.py:109-127): expected values q_k = sum_j softmax(l_k)_j z_j, q = (q1 + q2) / 2 or min(q1, q2),
// loss_b = alpha log_prob_b - q_b; d loss / d l_kj = -(w_k / B) p_kj (z_j - q_k).  One wave per row; partial[block] = sum of loss_b.
__global__ __launch_bounds__(256) void k_fs_policy_seed(const float* __restrict__ l1, const float* __restrict__ l2,
                                                        const float* __restrict__ logp, const float* __restrict__ log_alpha,
                                                        float* __restrict__ d1, float* __restrict__ d2, float* __restrict__ partial,
                                                        int64_t M, int NA, float v_min, float v_max, int clipped, float inv_b) {
  __shared__ float s_loss[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  const float dz = (v_max - v_min) / (float)(NA - 1);
  float loss = 0.f;
  if (row < M) {
    float q[2], p[2][4];
    const float* lg[2] = {l1 + row * NA, l2 + row * NA};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float v[4], mx = -3.4e38f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int a = lane + 64 * u;
        v[u] = a < NA ? lg[k][a] : -3.4e38f;
        mx = fmaxf(mx, v[u]);
      }
      mx = wave_max(mx);
      float se = 0.f, sq = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int a = lane + 64 * u;
        p[k][u] = a < NA ? expf(v[u] - mx) : 0.f;
        se += p[k][u];
        sq += p[k][u] * (v_min + dz * (float)a);
      }
      se = wave_sum(se);
      sq = wave_sum(sq);
      q[k] = sq / se;
#pragma unroll
      for (int u = 0; u < 4; ++u) p[k][u] /= se;
    }
    float w1 = 0.5f, w2 = 0.5f, qv = (q[0] + q[1]) * 0.5f;
    if (clipped) {
      w1 = q[0] <= q[1] ? 1.f : 0.f;      // torch.minimum: the gradient goes to the smaller one (to the first on a tie)
      w2 = 1.f - w1;
      qv = fminf(q[0], q[1]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int a = lane + 64 * u;
      if (a < NA) {
        const float z = v_min + dz * (float)a;
        d1[row * NA + a] = -(w1 * inv_b) * p[0][u] * (z - q[0]);
        d2[row * NA + a] = -(w2 * inv_b) * p[1][u] * (z - q[1]);
      }
    }
    loss = expf(log_alpha[0]) * logp[row] - qv;
  }
  if (lane == 0) s_loss[w] = loss;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
}

// d loss / d head [M, 2A] of the policy (chain through the tanh squashing, the action scale and the tanh-mapped log-std):
// da1 + da2 = d loss / d action from the two critics' input gradients (row stride lda, first column c0); the log-prob term
// carries alpha / B.
__global__ __launch_bounds__(256) void k_fs_policy_grad(const float* __restrict__ head, const float* __restrict__ scale,
                                                        const float* __restrict__ eps_inject, uint32_t k0, uint32_t k1, int scheme,
                                                        const float* __restrict__ da1, const float* __restrict__ da2, int lda, int c0,
                                                        const float* __restrict__ log_alpha, float* __restrict__ dhead, int64_t M, int A,
                                                        float ls_min, float ls_max, float inv_b, int64_t row_off, int64_t M_global) {
  const int64_t n = M * A;
  const float ab = expf(log_alpha[0]) * inv_b;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / A;
    const int j = (int)(e - i * A);
    const float mean = head[i * 2 * A + j];
    const float th = tanhf(head[i * 2 * A + A + j]);
    const float half = 0.5f * (ls_max - ls_min);
    const float ls = ls_min + half * (th + 1.0f);
    const float sd = expf(ls);
    const float eps = eps_inject ? eps_inject[i * A + j]
                                 : normal_from_bits(random_bits_at(k0, k1, (uint64_t)(i + row_off) * A + j, (uint64_t)M_global * A, scheme));
    const float t = tanhf(mean + sd * eps);
    const float om = 1.0f - t * t;
    // d loss / d t: through the action, and through -log(1 - t^2 + 1e-6) of the log-prob
    const float dt = (da1[i * lda + c0 + j] + da2[i * lda + c0 + j]) * scale[j] + ab * (2.0f * t / (om + 1e-6f));
    const float draw = dt * om;
    // the Gaussian term -(raw - mean)^2 / (2 sd^2) equals -eps^2 / 2: no dependence on mean or log-std
    dhead[i * 2 * A + j] = draw;
    const float dls = draw * eps * sd - ab;
    dhead[i * 2 * A + A + j] = dls * half * (1.0f - th * th);
  }
}

// entropy-coefficient step (fastsac.py:226-239, entropy_coefficient.py:25-30) + the scalars of the critic step:
// entropy = -mean(next_log_prob); loss = exp(log_alpha) (entropy - target); AdamW on log_alpha.
// metrics: [0] q_loss [1] entropy_loss [2] q_min [3] q_max [4] entropy [5] (critic grad norm, by the Adam launch) [6] entropy grad norm ^ 2 [7] alpha
__global__ __launch_bounds__(256) void k_fs_alpha_step(const float* __restrict__ logp, int64_t M, float* __restrict__ log_alpha,
                                                       float* __restrict__ am, float* __restrict__ av, const float* __restrict__ c51_out,
                                                       float target_entropy, float lr, float wd, float b1, float b2, float eps, float bc1,
                                                       float bc2, float* __restrict__ metrics) {
  __shared__ float s_buf[4];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < M; i += 256) acc += logp[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_buf[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float entropy = -((s_buf[0] + s_buf[1]) + (s_buf[2] + s_buf[3])) / (float)M;
    const float la = log_alpha[0], alpha = expf(la);
    const float g = alpha * (entropy - target_entropy);
    metrics[0] = c51_out[0];
    metrics[1] = g;                 // the loss has the same value as its derivative with respect to log_alpha
    metrics[2] = c51_out[1];
    metrics[3] = c51_out[2];
    metrics[4] = entropy;
    metrics[6] = g * g;
    metrics[7] = alpha;
    const float mi = b1 * am[0] + (1.f - b1) * g, vi = b2 * av[0] + (1.f - b2) * g * g;
    am[0] = mi;
    av[0] = vi;
    log_alpha[0] = la * (1.0f - lr * wd) - lr * ((mi / bc1) / (sqrtf(vi / bc2) + eps));
  }
}

__global__ __launch_bounds__(256) void k_fs_policy_metrics(const float* __restrict__ partial, int n, const float* __restrict__ log_alpha,
                                                           float inv_b, float* __restrict__ metrics) {
  __shared__ float s_buf[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_buf[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    metrics[0] = ((s_buf[0] + s_buf[1]) + (s_buf[2] + s_buf[3])) * inv_b;   // policy loss
    metrics[1] = expf(log_alpha[0]);                                          // alpha used by this step
  }
}

static int fs_sample(const float* head, const float* scale, const uint32_t ks[2], int scheme, const float* inject, float* act_out, int ld,
                     int c0, float* logp, int64_t M, int A, const rlx_fastsac_hparams& hp, int deterministic, int64_t row_off,
                     int64_t M_global, hipStream_t st) {
  RLX_REQUIRE(A >= 1 && A <= 256, RLX_EUNSUP, "fastsac: 1 <= act_dim <= 256");
  const int rpb = 256 / A;
  hipLaunchKernelGGL(k_fs_sample, dim3(div_up(M, rpb)), dim3(256), (size_t)rpb * A * sizeof(float), st, head, scale, ks[0], ks[1], scheme,
                     inject, act_out, ld, c0, logp, M, A, hp.log_std_min, hp.log_std_max, deterministic, row_off, M_global);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

// ReplayBuffer.sample (replay_buffer.py:34-96) for given start rows idx_t and env columns idx_e: the n-step return over the
// steps up to the first done, gamma^k discounts, the number of steps that counted, next state / done / truncation of the step
// where the window ends (first done or first truncation, else the last step); with a full ring the newest row counts as
// truncated unless it is done (:49-55).  One wave per sample: lane 0 scans the window, all lanes copy the rows.
__global__ __launch_bounds__(256) void k_fs_nstep_sample(const float* __restrict__ rs, const float* __restrict__ rns,
                                                         const float* __restrict__ ra, const float* __restrict__ rr,
                                                         const float* __restrict__ rd, const float* __restrict__ rt, int capacity,
                                                         int nr_envs, int O, int A, int n_steps, float gamma, int last_idx,
                                                         const int32_t* __restrict__ idx_t, const int32_t* __restrict__ idx_e, int64_t B,
                                                         float* __restrict__ os, float* __restrict__ ons, float* __restrict__ oa,
                                                         float* __restrict__ orw, float* __restrict__ od, float* __restrict__ otr,
                                                         float* __restrict__ on) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  const int t0 = idx_t[i], e = idx_e[i];
  int ft = t0;
  if (lane == 0) {
    auto trunc_at = [&](int t) {
      const float tr = rt[(int64_t)t * nr_envs + e];
      return (n_steps > 1 && t == last_idx) ? (rd[(int64_t)t * nr_envs + e] > 0.f ? tr : 1.0f) : tr;
    };
    float rew, eff;
    if (n_steps == 1) {
      rew = rr[(int64_t)t0 * nr_envs + e];
      eff = 1.0f;
    } else {
      float mask = 1.0f;
      rew = 0.f;
      eff = 0.f;
      int first_done = n_steps - 1, first_trunc = n_steps - 1;
      bool fd = false, ftr = false;
      for (int k = 0; k < n_steps; ++k) {
        const int t = (t0 + k) % capacity;
        const float d = rd[(int64_t)t * nr_envs + e];
        rew += rr[(int64_t)t * nr_envs + e] * mask * powf(gamma, (float)k);
        eff += mask;
        if (!fd && d > 0.f) { first_done = k; fd = true; }
        if (!ftr && trunc_at(t) > 0.f) { first_trunc = k; ftr = true; }
        mask *= 1.0f - d;
      }
      ft = (t0 + (first_done < first_trunc ? first_done : first_trunc)) % capacity;
    }
    orw[i] = rew;
    on[i] = eff;
    od[i] = rd[(int64_t)ft * nr_envs + e];
    otr[i] = trunc_at(ft);
  }
  ft = __shfl(ft, 0, 64);
  const float* s0 = rs + ((int64_t)t0 * nr_envs + e) * O;
  const float* s1 = rns + ((int64_t)ft * nr_envs + e) * O;
  for (int c = lane; c < O; c += 64) {
    os[i * O + c] = s0[c];
    ons[i * O + c] = s1[c];
  }
  const float* a0 = ra + ((int64_t)t0 * nr_envs + e) * A;
  for (int c = lane; c < A; c += 64) oa[i * A + c] = a0[c];
}

static int fs_check(const rlx_lnmlp_desc& pd, const rlx_lnmlp_desc& qd, const rlx_fastsac_hparams& hp, int* A_out, int* Oc_out) {
  int rc = ln_check(pd);
  if (rc) return rc;
  rc = ln_check(qd);
  if (rc) return rc;
  RLX_REQUIRE(pd.out_dim % 2 == 0, RLX_EINVAL, "fastsac: policy out_dim must be 2 * act_dim ([mean | log_std])");
  const int A = pd.out_dim / 2;
  RLX_REQUIRE(qd.in_dim > A && qd.out_dim == hp.nr_atoms && hp.nr_atoms >= 2 && hp.nr_atoms <= 128, RLX_EINVAL,
              "fastsac: critic in_dim = critic obs + act, out_dim = nr_atoms (2..128)");
  RLX_REQUIRE(hp.v_max > hp.v_min && hp.log_std_max > hp.log_std_min, RLX_EINVAL, "fastsac: v_max > v_min and log_std_max > log_std_min");
  *A_out = A;
  *Oc_out = qd.in_dim - A;
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int64_t rlx_lnmlp_param_count(const rlx_lnmlp_desc* d) {
  if (!d || d->n_hidden < 1 || d->n_hidden > 4) return -1;
  return ln_layout(*d).n_params;
}

int rlx_lnmlp_fwd_f32(rlx_ctx* ctx, const rlx_lnmlp_desc* d, const float* params, const float* x, int ldx, float* out, int64_t M,
                      void* stream) {
  RLX_REQUIRE(ctx && d && params && x && out && M > 0 && ldx >= (d ? d->in_dim : 1), RLX_EINVAL, "rlx_lnmlp_fwd_f32: bad args");
  int rc = ln_check(*d);
  if (rc) return rc;
  bx_release_all(ctx);
  const Chain L = ln_layout(*d);
  const int ldp = (d->in_dim + 3) & ~3;
  ChainBufs b;
  float* xp;                         // the rows at a 16-byte pitch, when the caller's are not
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(L, M, a, &b);
    xp = a.take((size_t)M * ldp);
  });
  if (rc) return rc;
  if (ldx % 4 != 0 || ldx < ldp) {   // the GEMM stages read 16-byte pieces: rows at a pitch that is a multiple of four, zero padded
    RLX_REQUIRE(ldx == d->in_dim, RLX_EUNSUP, "rlx_lnmlp_fwd_f32: a row stride that is not a multiple of 4 must equal in_dim");
    rc = fs_concat(x, d->in_dim, nullptr, 0, xp, ldp, M, (hipStream_t)stream);
    if (rc) return rc;
    x = xp;
    ldx = ldp;
  }
  return chain_fwd(ctx, L, params, x, ldx, b, out, M, (hipStream_t)stream);
}

int rlx_fastsac_replay_sample_f32(rlx_ctx* ctx, const float* ring_states, const float* ring_next_states, const float* ring_actions,
                                  const float* ring_rewards, const float* ring_dones, const float* ring_truncations, int capacity,
                                  int nr_envs, int obs_dim, int act_dim, int n_steps, float gamma, int pos, int size,
                                  const int32_t* idx_t, const int32_t* idx_e, int64_t B, float* states, float* next_states,
                                  float* actions, float* rewards, float* dones, float* truncations, float* effective_n_steps,
                                  void* stream) {
  RLX_REQUIRE(ctx && ring_states && ring_next_states && ring_actions && ring_rewards && ring_dones && ring_truncations && idx_t && idx_e &&
                  states && next_states && actions && rewards && dones && truncations && effective_n_steps,
              RLX_EINVAL, "rlx_fastsac_replay_sample_f32: NULL pointer");
  RLX_REQUIRE(B > 0 && capacity > 0 && nr_envs > 0 && obs_dim > 0 && act_dim > 0 && n_steps >= 1 && n_steps <= capacity && size >= 1 &&
                  size <= capacity && pos >= 0 && pos < capacity,
              RLX_EINVAL, "rlx_fastsac_replay_sample_f32: bad sizes");
  const int last_idx = size >= capacity ? (pos + capacity - 1) % capacity : -1;
  hipLaunchKernelGGL(k_fs_nstep_sample, dim3(div_up(B, 4)), dim3(256), 0, (hipStream_t)stream, ring_states, ring_next_states, ring_actions,
                     ring_rewards, ring_dones, ring_truncations, capacity, nr_envs, obs_dim, act_dim, n_steps, gamma, last_idx, idx_t, idx_e, B,
                     states, next_states, actions, rewards, dones, truncations, effective_n_steps);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int rlx_fastsac_act_f32(rlx_ctx* ctx, const rlx_lnmlp_desc* pdesc, const float* pparams, const float* obs, const float* action_scale,
                        uint32_t key_io[2], int scheme, float* action, int N, int deterministic, int row_offset, int N_global,
                        const rlx_fastsac_hparams* hp, void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && obs && action_scale && key_io && action && hp && N > 0 && N_global >= N, RLX_EINVAL,
              "rlx_fastsac_act_f32: bad args");
  int rc = ln_check(*pdesc);
  if (rc) return rc;
  RLX_REQUIRE(pdesc->out_dim % 2 == 0, RLX_EINVAL, "rlx_fastsac_act_f32: policy out_dim must be 2 * act_dim");
  const int A = pdesc->out_dim / 2;
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain L = ln_layout(*pdesc);
  const int ldp = (pdesc->in_dim + 3) & ~3;
  ChainBufs b;
  float *head, *xs;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(L, N, a, &b);
    head = a.take((size_t)N * 2 * A);
    xs = a.take((size_t)N * ldp);
  });
  if (rc) return rc;
  rc = fs_concat(obs, pdesc->in_dim, nullptr, 0, xs, ldp, N, st);
  if (!rc) rc = chain_fwd(ctx, L, pparams, xs, ldp, b, head, N, st);
  if (rc) return rc;
  uint32_t sub[2] = {0, 0};
  if (!deterministic) next_key(key_io, sub, 1, scheme);      // key, subkey = split(key)
  return fs_sample(head, action_scale, sub, scheme, ctx->dbg_sac_eps[0], action, A, 0, nullptr, N, A, *hp, deterministic, row_offset,
                   N_global, st);
}

int rlx_fastsac_critic_update_f32(rlx_ctx* ctx, const rlx_lnmlp_desc* pdesc, const float* pparams, const rlx_lnmlp_desc* qdesc,
                                  float* qparams, float* qm, float* qv, float* qtarget, float* log_alpha, float* am, float* av,
                                  const float* states, const float* next_states, const float* critic_states,
                                  const float* critic_next_states, const float* actions, const float* rewards, const float* dones,
                                  const float* truncations, const float* effective_n_steps, const float* action_scale, int64_t B,
                                  uint32_t key_io[2], int scheme, int64_t* opt_count_io, const rlx_fastsac_hparams* hp,
                                  float* metrics_out, void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && qdesc && qparams && qm && qv && qtarget && log_alpha && am && av && states && next_states &&
                  actions && rewards && dones && truncations && effective_n_steps && action_scale && key_io && opt_count_io && hp &&
                  metrics_out && B > 0,
              RLX_EINVAL, "rlx_fastsac_critic_update_f32: bad args");
  int A, Oc;
  int rc = fs_check(*pdesc, *qdesc, *hp, &A, &Oc);
  if (rc) return rc;
  RLX_REQUIRE((critic_states != nullptr) == (critic_next_states != nullptr) && (critic_states || Oc == pdesc->in_dim), RLX_EINVAL,
              "rlx_fastsac_critic_update_f32: critic obs width != policy obs width needs critic_states AND critic_next_states");
  const float* cs = critic_states ? critic_states : states;
  const float* cn = critic_next_states ? critic_next_states : next_states;
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain LP = ln_layout(*pdesc), LQ = ln_layout(*qdesc);
  const int64_t nq = LQ.n_params;
  const int NA = hp->nr_atoms, ldc = (Oc + A + 3) & ~3;
  // ---- arena: policy activations, one set for the two target passes (inference), two sets for the online critics
  const int ldp = (pdesc->in_dim + 3) & ~3;
  ChainBufs bp, bt, b1, b2;
  float *xc, *xn, *head, *lt1, *lt2, *l1, *l2, *d1, *d2, *lpn, *gq, *xs, *c51o;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(LP, B, a, &bp);
    chain_carve(LQ, B, a, &bt);
    chain_carve(LQ, B, a, &b1);
    chain_carve(LQ, B, a, &b2);
    xc = a.take((size_t)B * ldc);
    xn = a.take((size_t)B * ldc);
    head = a.take((size_t)B * 2 * A);
    for (float** l : {&lt1, &lt2, &l1, &l2, &d1, &d2}) *l = a.take((size_t)B * NA);
    lpn = a.take(B);
    gq = a.take(2 * nq);
    xs = a.take((size_t)B * ldp);                               // policy observations at a 16-byte row pitch
    c51o = a.take(4);
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc || !sq) return RLX_ENOMEM;
  uint32_t ks[2];
  next_key(key_io, ks, 1, scheme);                              // key, subkey = split(key)
  BxReleaseAll bx_all{ctx};
  {
    const NetRef nets[5] = {{pparams, &LP, false}, {qtarget, &LQ, false}, {qtarget + nq, &LQ, false}, {qparams, &LQ, true}, {qparams + nq, &LQ, true}};
    rc = trunk_images(ctx, nets, 5, B, st);
    if (rc) return rc;
  }
  // Two streams: the policy on s' + both target critics on (s', a') on the caller's stream, both online critics on (s, a) on the
  // side stream; after the C51 loss one critic's backward on each.  (Every pass is a chain of one-wave launches -- 8192 rows are
  // 128 row tiles -- so the halves overlap almost for free.)
  FsFork fk(ctx, st);
  rc = fk.begin();
  if (rc) return rc;
  rc = fs_concat(cs, Oc, actions, A, xc, ldc, B, st);
  if (!rc) rc = fk.fork();
  // ---- online critics on (s, a)
  if (!rc) rc = chain_fwd(ctx, LQ, qparams, xc, ldc, b1, l1, B, fk.side());
  if (!rc) rc = chain_fwd(ctx, LQ, qparams + nq, xc, ldc, b2, l2, B, fk.side());
  // ---- next action and log-prob from the policy (no gradient), target critics on (s', a')
  if (!rc) rc = fs_concat(cn, Oc, nullptr, A, xn, ldc, B, fk.main());
  if (!rc) rc = fs_concat(next_states, pdesc->in_dim, nullptr, 0, xs, ldp, B, st);
  if (!rc) rc = chain_fwd(ctx, LP, pparams, xs, ldp, bp, head, B, st);
  if (!rc) rc = fs_sample(head, action_scale, ks, scheme, ctx->dbg_sac_eps[0], xn, ldc, Oc, lpn, B, A, *hp, 0, 0, B, st);
  if (!rc) rc = chain_fwd(ctx, LQ, qtarget, xn, ldc, bt, lt1, B, st);
  if (!rc) rc = chain_fwd(ctx, LQ, qtarget + nq, xn, ldc, bt, lt2, B, st);
  if (!rc) rc = fk.join();
  // ---- the C51 loss and its logit gradients
  if (!rc) rc = rlx_c51_critic_loss_f32(ctx, l1, l2, lt1, lt2, rewards, dones, truncations, effective_n_steps, lpn, log_alpha, B, NA, hp->gamma,
                                        hp->v_min, hp->v_max, hp->clipped_double_q, d1, d2, c51o, stream);
  if (rc) return rc;
  {
    BwdPass bwd(ctx, B);   // d logits ~ 1 / B
    rc = bwd.begin(2 * chain_stage_floats(ctx, LQ, B, true));
    if (!rc) rc = fk.fork();
    if (!rc) rc = chain_bwd(ctx, LQ, qparams + nq, xc, ldc, b2, d2, gq + nq, nullptr, 0, B, fk.side());
    if (!rc) rc = chain_bwd(ctx, LQ, qparams, xc, ldc, b1, d1, gq, nullptr, 0, B, fk.main());
    if (!rc) rc = fk.join();
    if (!rc) rc = bwd.finish(st);
    if (rc) return rc;
  }
  // ---- entropy coefficient (uses alpha BEFORE its own step inside the C51 target: the launch order above), then AdamW + Polyak
  const int64_t step = *opt_count_io + 1;
  const float bc1 = (float)(1.0 - pow((double)hp->adam_b1, (double)step)), bc2 = (float)(1.0 - pow((double)hp->adam_b2, (double)step));
  hipLaunchKernelGGL(k_fs_alpha_step, dim3(1), dim3(256), 0, st, (const float*)lpn, B, log_alpha, am, av, (const float*)c51o,
                     hp->target_entropy, hp->lr_alpha, hp->weight_decay, hp->adam_b1, hp->adam_b2, hp->adam_eps, bc1, bc2, metrics_out);
  RLX_LAUNCH_CHECK();
  rc = torch_clip_adam(qparams, gq, qm, qv, 2 * nq, sq, step, hp->lr_critic, *hp, metrics_out + 5, st, qtarget, hp->tau, hp->weight_decay);
  if (rc) return rc;
  *opt_count_io += 1;
  return RLX_OK;
}

int rlx_fastsac_policy_update_f32(rlx_ctx* ctx, const rlx_lnmlp_desc* pdesc, float* pparams, float* pm, float* pv,
                                  const rlx_lnmlp_desc* qdesc, const float* qparams, const float* log_alpha, const float* states,
                                  const float* critic_states, const float* action_scale, int64_t B, uint32_t key_io[2], int scheme,
                                  int64_t* opt_count_io, const rlx_fastsac_hparams* hp, float* metrics_out, void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && pm && pv && qdesc && qparams && log_alpha && states && action_scale && key_io && opt_count_io &&
                  hp && metrics_out && B > 0,
              RLX_EINVAL, "rlx_fastsac_policy_update_f32: bad args");
  int A, Oc;
  int rc = fs_check(*pdesc, *qdesc, *hp, &A, &Oc);
  if (rc) return rc;
  RLX_REQUIRE(critic_states || Oc == pdesc->in_dim, RLX_EINVAL,
              "rlx_fastsac_policy_update_f32: critic obs width != policy obs width needs critic_states");
  const float* cs = critic_states ? critic_states : states;
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain LP = ln_layout(*pdesc), LQ = ln_layout(*qdesc);
  const int64_t np_ = LP.n_params, nq = LQ.n_params;
  const int NA = hp->nr_atoms, ldc = (Oc + A + 3) & ~3;
  const int nblk = div_up(B, 4);
  const int ldp = (pdesc->in_dim + 3) & ~3;
  ChainBufs bp, b1, b2;
  float *xp, *dx1, *dx2, *head, *dhead, *l1, *l2, *d1, *d2, *lp, *part, *gp, *xs;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(LP, B, a, &bp);
    chain_carve(LQ, B, a, &b1);
    chain_carve(LQ, B, a, &b2);
    for (float** x : {&xp, &dx1, &dx2}) *x = a.take((size_t)B * ldc);
    head = a.take((size_t)B * 2 * A);
    dhead = a.take((size_t)B * 2 * A);
    for (float** l : {&l1, &l2, &d1, &d2}) *l = a.take((size_t)B * NA);
    lp = a.take(B);
    part = a.take(nblk);
    gp = a.take(np_);
    xs = a.take((size_t)B * ldp);                               // policy observations at a 16-byte row pitch
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc || !sq) return RLX_ENOMEM;
  uint32_t ks[2];
  next_key(key_io, ks, 1, scheme);                              // key, subkey = split(key)
  const float inv_b = 1.0f / (float)B;
  BxReleaseAll bx_all{ctx};
  {
    const NetRef nets[3] = {{pparams, &LP, true}, {qparams, &LQ, true}, {qparams + nq, &LQ, true}};
    rc = trunk_images(ctx, nets, 3, B, st);
    if (rc) return rc;
  }
  // policy on s, sampled action into the critics' input rows, both critics, seeds
  rc = fs_concat(cs, Oc, nullptr, A, xp, ldc, B, st);
  if (!rc) rc = fs_concat(states, pdesc->in_dim, nullptr, 0, xs, ldp, B, st);
  if (!rc) rc = chain_fwd(ctx, LP, pparams, xs, ldp, bp, head, B, st);
  if (!rc) rc = fs_sample(head, action_scale, ks, scheme, ctx->dbg_sac_eps[1], xp, ldc, Oc, lp, B, A, *hp, 0, 0, B, st);
  FsFork fk(ctx, st);
  if (!rc) rc = fk.begin();
  if (!rc) rc = fk.fork();
  if (!rc) rc = chain_fwd(ctx, LQ, qparams + nq, xp, ldc, b2, l2, B, fk.side());
  if (!rc) rc = chain_fwd(ctx, LQ, qparams, xp, ldc, b1, l1, B, fk.main());
  if (!rc) rc = fk.join();
  if (rc) return rc;
  hipLaunchKernelGGL(k_fs_policy_seed, dim3(nblk), dim3(256), 0, st, (const float*)l1, (const float*)l2, (const float*)lp, log_alpha, d1, d2,
                     part, B, NA, hp->v_min, hp->v_max, hp->clipped_double_q, inv_b);
  RLX_LAUNCH_CHECK();
  {
    BwdPass bwd(ctx, B);
    rc = bwd.begin(2 * chain_stage_floats(ctx, LQ, B, false) + chain_stage_floats(ctx, LP, B, true));
    if (rc) return rc;
    // the critics' input gradients (no parameter gradients; one critic per stream), then the policy's backward
    rc = fk.fork();
    if (!rc) rc = chain_bwd(ctx, LQ, qparams + nq, xp, ldc, b2, d2, nullptr, dx2, ldc, B, fk.side(), Oc, A);
    if (!rc) rc = chain_bwd(ctx, LQ, qparams, xp, ldc, b1, d1, nullptr, dx1, ldc, B, fk.main(), Oc, A);
    if (!rc) rc = fk.join();
    if (rc) return rc;
    int grid = div_up(B * A, 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(k_fs_policy_grad, dim3(grid), dim3(256), 0, st, (const float*)head, action_scale, ctx->dbg_sac_eps[1], ks[0], ks[1],
                       scheme, (const float*)dx1, (const float*)dx2, ldc, Oc, log_alpha, dhead, B, A, hp->log_std_min, hp->log_std_max, inv_b,
                       (int64_t)0, B);
    RLX_LAUNCH_CHECK();
    rc = chain_bwd(ctx, LP, pparams, xs, ldp, bp, dhead, gp, nullptr, 0, B, st);
    if (!rc) rc = bwd.finish(st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_fs_policy_metrics, dim3(1), dim3(256), 0, st, (const float*)part, nblk, log_alpha, inv_b, metrics_out);
  RLX_LAUNCH_CHECK();
  rc = torch_clip_adam(pparams, gp, pm, pv, np_, sq, *opt_count_io + 1, hp->lr_policy, *hp, metrics_out + 2, st, nullptr, 0.f, hp->weight_decay);
  if (rc) return rc;
  *opt_count_io += 1;
  return RLX_OK;
}

}  // extern "C"
