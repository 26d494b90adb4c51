// fasttd3.hip -- FastTD3 update steps (rl_x/algorithms/fasttd3/pytorch/fasttd3.py:105-225, :316-324): distributional (C51) twin
// critics with clipped double Q, a deterministic tanh policy with per-env Gaussian exploration noise, target-policy smoothing,
// AdamW, Polyak targets.  No entropy term and no target policy.
//
// Networks (policy.py:38-47, q_network.py:28-36): plain Dense -> ReLU trunks and a Dense head -- rlx_mlp_desc with act = RELU,
// ln_first = 0, has_logstd = 0 (flat layout: per layer W[in, out] row-major, b[out]; then the head), hidden widths multiples of
// 64 up to 1024 (td3_check: the PPO / SAC check mlp_check_desc stays as it is).  A network is net_pass.h's Chain of plain blocks:
// the library's GEMM stages with the fused bias + ReLU epilogue (launch_gemm_fwd) and the ReLU' input-gradient epilogue
// (stage_dx), the split-operand engine for passes of >= 4096 rows (trunk_images), stage_dw for the weight gradients; the heads
// are dense_head.hip's k_fs_head_* kernels (the input-gradient one with the ReLU' epilogue chain_bwd gives a plain last block) or,
// where a tanh follows, the fused head kernel k_td3_head_act below.  Carve, forward, backward, stage-arena size, grids and key
// splitting: net_pass.h, shared with fastsac.hip, reppo.hip, mpo.hip and espo.hip.
//
// fp16 window: the split-operand engine holds |weight| < 1023, |activation| < 4094, per-sample gradient < 8190.
// ReLU activations are not bounded by a LayerNorm; a value outside the window turns the affected products into inf / NaN, the
// AdamW launch skips a step whose gradient norm is non-finite, and the metrics carry the NaN -- the plugin raises on it, as
// fastsac.hip does.  Nothing is silently wrong.
//
// Noise: the reference draws with torch's CUDA generator; the library uses its counter RNG (threefry, the key split per call
// like rlx_fastsac_*), and rlx_dbg_set_sac_noise(eps_next, .) injects the given N(0, 1) draws of the exploration noise
// (rlx_fasttd3_act_f32, [N, A]) and of the smoothing noise (rlx_fasttd3_critic_update_f32, [B, A]) for parity tests.
// CPU twin: tests/fasttd3_twin.py, pinned by outputs of the reference's own modules and closures (tests/golden/fasttd3_reference.npz).
#include "dpg.h"

namespace rlx {

static int td3_check(const rlx_mlp_desc& d) {
  RLX_REQUIRE(d.n_hidden >= 1 && d.n_hidden <= 3 && d.in_dim > 0 && d.out_dim > 0, RLX_EINVAL,
              "fasttd3: network descriptor needs 1..3 hidden layers and positive widths");
  RLX_REQUIRE(d.act == RLX_ACT_RELU && !d.ln_first && !d.has_logstd, RLX_EINVAL,
              "fasttd3: network descriptor must be act = RLX_ACT_RELU, ln_first = 0, has_logstd = 0");
  for (int l = 0; l < d.n_hidden; ++l)
    RLX_REQUIRE(d.hidden[l] > 0 && d.hidden[l] % 64 == 0 && d.hidden[l] <= 1024, RLX_EUNSUP,
                "fasttd3: hidden widths must be multiples of 64, at most 1024");
  return RLX_OK;
}

static Chain td3_layout(const rlx_mlp_desc& d) {   // the flat layout of rlx_mlp_desc without LayerNorm and log-std
  return make_chain(d.in_dim, d.hidden, d.n_hidden, d.out_dim, NORM_NONE, RLX_ACT_RELU);
}

// ---------------------------------------------------------------------------------------------------------------- kernels
enum TdNoise { TD_NOISE_NONE = 0, TD_NOISE_EXPLORE = 1, TD_NOISE_SMOOTH = 2 };

// The policy's head fused with what follows it: one thread per (row, action) computes head = H[i, :] . W[:, j] + b[j] (one
// ascending fmaf chain; K <= 1024 and A <= 64, small next to the trunk) and a = tanh(head), then
//   EXPLORE (policy.get_action, policy.py:57-66): a += eps * noise_scale[i]; act[i, j] = a (what the ring stores);
//            proc[i, j] = clip_rescale ? low + 0.5 (clamp(a, -1, 1) + 1)(high - low) : a (what the env gets)
//   SMOOTH   (critic_loss_fn, fasttd3.py:143-144): a = clamp(a + clamp(eps * smoothing_eps, +-clip), -1, 1), written straight into
//            the action columns [c0, c0 + A) of the target critics' input rows (row stride ld): no concat pass
//   NONE     a itself (the policy step's action columns; evaluation)
// eps: eps_inject[i, j] (test hook) or normal(bits(key, (i + row_off) * A + j of M_global * A)).
__global__ __launch_bounds__(256) void k_td3_head_act(const float* __restrict__ H, const float* __restrict__ W, const float* __restrict__ b,
                                                      int64_t M, int K, int A, int mode, const float* __restrict__ noise_scale, float smooth_eps,
                                                      float smooth_clip, uint32_t k0, uint32_t k1, int scheme,
                                                      const float* __restrict__ eps_inject, int64_t row_off, int64_t M_global,
                                                      float* __restrict__ act, int ld, int c0, float* __restrict__ proc, int clip_rescale,
                                                      const float* __restrict__ low, const float* __restrict__ high) {
  const int64_t n = M * A;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / A;
    const int j = (int)(e - i * A);
    const float* hr = H + i * K;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(hr[k], W[(int64_t)k * A + j], acc);
    float a = tanhf(acc + b[j]);
    if (mode != TD_NOISE_NONE) {
      const float eps = eps_inject ? eps_inject[i * A + j]
                                   : normal_from_bits(random_bits_at(k0, k1, (uint64_t)(i + row_off) * A + j, (uint64_t)M_global * A, scheme));
      if (mode == TD_NOISE_EXPLORE) {
        a = a + eps * noise_scale[i];
      } else {
        const float nz = fminf(fmaxf(eps * smooth_eps, -smooth_clip), smooth_clip);
        a = fminf(fmaxf(a + nz, -1.0f), 1.0f);
      }
    }
    act[i * ld + c0 + j] = a;
    if (proc) proc[i * A + j] = clip_rescale ? low[j] + 0.5f * (fminf(fmaxf(a, -1.0f), 1.0f) + 1.0f) * (high[j] - low[j]) : a;
  }
}

// noise_scales[i] = U[0, 1) (noise_std_max - noise_std_min) + noise_std_min for every env (dones == NULL: fasttd3.py:241) or for
// the envs whose done is set (fasttd3.py:274-278); u = bits(key, i of N) -> [0, 1) as jax.random.uniform
__global__ __launch_bounds__(256) void k_td3_noise_scales(float* __restrict__ scales, const float* __restrict__ dones, int N, uint32_t k0,
                                                          uint32_t k1, int scheme, float lo, float hi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N || (dones && !(dones[i] > 0.f))) return;
  scales[i] = bits_to_unit(random_bits_at(k0, k1, (uint64_t)i, (uint64_t)N, scheme)) * (hi - lo) + lo;
}

// policy loss seeds (fasttd3.py:105-120): q_k = sum_j softmax(l_k)_j z_j, q = min(q1, q2) (clipped) or (q1 + q2) / 2,
// loss = -mean(q); d loss / d l_kj = -(w_k / B) p_kj (z_j - q_k) with torch.minimum's weights: all to the smaller one, 1/2 each on
// a tie.  One wave per row; partial[block] = sum of -q_b over its four rows.
__global__ __launch_bounds__(256) void k_td3_policy_seed(const float* __restrict__ l1, const float* __restrict__ l2, float* __restrict__ d1,
                                                         float* __restrict__ d2, float* __restrict__ partial, int64_t M, int NA, float v_min,
                                                         float v_max, int clipped, float inv_b) {
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
      w1 = q[0] < q[1] ? 1.f : (q[0] > q[1] ? 0.f : 0.5f);
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
    loss = -qv;
  }
  if (lane == 0) s_loss[w] = loss;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
}

__global__ __launch_bounds__(256) void k_td3_policy_loss(const float* __restrict__ partial, int n, float inv_b, float* __restrict__ metrics) {
  __shared__ float s_buf[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_buf[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) metrics[0] = ((s_buf[0] + s_buf[1]) + (s_buf[2] + s_buf[3])) * inv_b;
}

static int td3_head_act(const Chain& L, const float* p, const float* H, int64_t M, int mode, const float* noise_scale, float smooth_eps,
                        float smooth_clip, const uint32_t ks[2], int scheme, const float* inject, int64_t row_off, int64_t M_global, float* act,
                        int ld, int c0, float* proc, int clip_rescale, const float* low, const float* high, hipStream_t st) {
  const int A = L.head.out;
  hipLaunchKernelGGL(k_td3_head_act, dim3(elem_grid(M * A)), dim3(256), 0, st, H, p + L.head.W, p + L.head.b, M, L.head.in, A, mode, noise_scale,
                     smooth_eps, smooth_clip, ks[0], ks[1], scheme, inject, row_off, M_global, act, ld, c0, proc, clip_rescale, low, high);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

static int td3_check_pair(const rlx_mlp_desc& pd, const rlx_mlp_desc& qd, const rlx_fasttd3_hparams& hp, int* A_out, int* Oc_out) {
  int rc = td3_check(pd);
  if (rc) return rc;
  rc = td3_check(qd);
  if (rc) return rc;
  const int A = pd.out_dim;
  RLX_REQUIRE(A <= 64, RLX_EUNSUP, "fasttd3: act_dim (policy out_dim) at most 64");
  RLX_REQUIRE(qd.in_dim > A && qd.out_dim == hp.nr_atoms && hp.nr_atoms >= 2 && hp.nr_atoms <= 128, RLX_EINVAL,
              "fasttd3: critic in_dim = critic obs + act, out_dim = nr_atoms (2..128)");
  RLX_REQUIRE(hp.v_max > hp.v_min, RLX_EINVAL, "fasttd3: v_max > v_min");
  *A_out = A;
  *Oc_out = qd.in_dim - A;
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int rlx_fasttd3_noise_scales_f32(rlx_ctx* ctx, uint32_t key_io[2], int scheme, float* noise_scales, const float* dones, int N,
                                 float noise_std_min, float noise_std_max, void* stream) {
  RLX_REQUIRE(ctx && key_io && noise_scales && N > 0, RLX_EINVAL, "rlx_fasttd3_noise_scales_f32: bad args");
  uint32_t ks[2];
  next_key(key_io, ks, 1, scheme);      // key, subkey = split(key)
  hipLaunchKernelGGL(k_td3_noise_scales, dim3(div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, noise_scales, dones, N, ks[0], ks[1], scheme,
                     noise_std_min, noise_std_max);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int rlx_fasttd3_act_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, const float* pparams, const float* obs, const float* noise_scales,
                        uint32_t key_io[2], int scheme, float* action, float* processed_action, int N, int deterministic,
                        int clip_and_rescale, const float* low, const float* high, int row_offset, int N_global, void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && obs && key_io && action && processed_action && N > 0 && N_global >= N &&
                  (deterministic || noise_scales) && (!clip_and_rescale || (low && high)),
              RLX_EINVAL, "rlx_fasttd3_act_f32: bad args");
  int rc = td3_check(*pdesc);
  if (rc) return rc;
  RLX_REQUIRE(pdesc->out_dim <= 64, RLX_EUNSUP, "rlx_fasttd3_act_f32: act_dim at most 64");
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain L = td3_layout(*pdesc);
  const int ldp = (pdesc->in_dim + 3) & ~3;
  ChainBufs b;
  float* xs;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(L, N, a, &b);
    xs = a.take((size_t)N * ldp);
  });
  if (rc) return rc;
  rc = fs_concat(obs, pdesc->in_dim, nullptr, 0, xs, ldp, N, st);
  if (!rc) rc = chain_fwd(ctx, L, pparams, xs, ldp, b, nullptr, N, st);
  if (rc) return rc;
  uint32_t ks[2] = {0, 0};
  if (!deterministic) next_key(key_io, ks, 1, scheme);
  return td3_head_act(L, pparams, b.H[L.n_hidden - 1], N, deterministic ? TD_NOISE_NONE : TD_NOISE_EXPLORE, noise_scales, 0.f, 0.f, ks,
                      scheme, ctx->dbg_sac_eps[0], row_offset, N_global, action, pdesc->out_dim, 0, processed_action, clip_and_rescale, low,
                      high, st);
}

int rlx_fasttd3_critic_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, const float* pparams, const rlx_mlp_desc* qdesc, float* qparams,
                                  float* qm, float* qv, float* qtarget, const float* states, const float* next_states,
                                  const float* critic_states, const float* critic_next_states, const float* actions, const float* rewards,
                                  const float* dones, const float* truncations, const float* effective_n_steps, int64_t B,
                                  uint32_t key_io[2], int scheme, int64_t* opt_count_io, const rlx_fasttd3_hparams* hp, float* metrics_out,
                                  void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && qdesc && qparams && qm && qv && qtarget && states && next_states && actions && rewards && dones &&
                  truncations && effective_n_steps && key_io && opt_count_io && hp && metrics_out && B > 0,
              RLX_EINVAL, "rlx_fasttd3_critic_update_f32: bad args");
  int A, Oc;
  int rc = td3_check_pair(*pdesc, *qdesc, *hp, &A, &Oc);
  if (rc) return rc;
  RLX_REQUIRE((critic_states != nullptr) == (critic_next_states != nullptr) && (critic_states || Oc == pdesc->in_dim), RLX_EINVAL,
              "rlx_fasttd3_critic_update_f32: critic obs width != policy obs width needs critic_states AND critic_next_states");
  const float* cs = critic_states ? critic_states : states;
  const float* cn = critic_next_states ? critic_next_states : next_states;
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain LP = td3_layout(*pdesc), LQ = td3_layout(*qdesc);
  const int64_t nq = LQ.n_params;
  const int NA = hp->nr_atoms, ldc = (Oc + A + 3) & ~3, ldp = (pdesc->in_dim + 3) & ~3;
  // ---- arena: policy trunk, one set for the two target passes (inference, one after the other), two sets for the online critics
  ChainBufs bp, bt, b1, b2;
  float *xc, *xn, *lt1, *lt2, *l1, *l2, *d1, *d2, *zeros, *gq, *xs, *ninf;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(LP, B, a, &bp);
    chain_carve(LQ, B, a, &bt);
    chain_carve(LQ, B, a, &b1);
    chain_carve(LQ, B, a, &b2);
    xc = a.take((size_t)B * ldc);
    xn = a.take((size_t)B * ldc);
    for (float** l : {&lt1, &lt2, &l1, &l2, &d1, &d2}) *l = a.take((size_t)B * NA);
    zeros = a.take(B);                                          // next_log_probs of the C51 target: 0 (no entropy term)
    gq = a.take(2 * nq);
    xs = a.take((size_t)B * ldp);                               // policy observations of s' at a 16-byte row pitch
    ninf = a.take(1);                                           // log_alpha of the C51 target: -inf (alpha = 0)
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc || !sq) return RLX_ENOMEM;
  uint32_t ks[2];
  next_key(key_io, ks, 1, scheme);
  BxReleaseAll bx_all{ctx};
  {
    const NetRef nets[5] = {{pparams, &LP, false}, {qtarget, &LQ, false}, {qtarget + nq, &LQ, false}, {qparams, &LQ, true}, {qparams + nq, &LQ, true}};
    rc = trunk_images(ctx, nets, 5, B, st);
    if (rc) return rc;
  }
  // Two streams: the online critics on (s, a) on the side stream; the policy on s', the smoothed next action and both target
  // critics on (s', a') on the caller's stream.  After the C51 loss one critic's backward on each.
  FsFork fk(ctx, st);
  rc = fk.begin();
  if (!rc) rc = fs_concat(cs, Oc, actions, A, xc, ldc, B, st);
  if (!rc) rc = fk.fork();
  if (!rc) rc = chain_fwd(ctx, LQ, qparams, xc, ldc, b1, l1, B, fk.side());
  if (!rc) rc = chain_fwd(ctx, LQ, qparams + nq, xc, ldc, b2, l2, B, fk.side());
  if (!rc) rc = fs_concat(cn, Oc, nullptr, A, xn, ldc, B, fk.main());
  if (!rc) rc = fs_concat(next_states, pdesc->in_dim, nullptr, 0, xs, ldp, B, st);
  if (!rc) rc = chain_fwd(ctx, LP, pparams, xs, ldp, bp, nullptr, B, st);
  if (!rc) rc = td3_head_act(LP, pparams, bp.H[LP.n_hidden - 1], B, TD_NOISE_SMOOTH, nullptr, hp->smoothing_epsilon, hp->smoothing_clip_value,
                             ks, scheme, ctx->dbg_sac_eps[0], 0, B, xn, ldc, Oc, nullptr, 0, nullptr, nullptr, st);
  if (!rc) rc = chain_fwd(ctx, LQ, qtarget, xn, ldc, bt, lt1, B, st);
  if (!rc) rc = chain_fwd(ctx, LQ, qtarget + nq, xn, ldc, bt, lt2, B, st);
  if (rc) return rc;
  RLX_HIP_TRY(hipMemsetAsync(zeros, 0, (size_t)B * sizeof(float), st));
  RLX_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ninf, (int)0xff800000u, 1, st));
  rc = fk.join();
  // ---- C51 target with alpha = exp(-inf) = 0 and zero log-probs: r - discount * 0 * 0 == r exactly; out4 = metrics_out[0..3]
  if (!rc) rc = rlx_c51_critic_loss_f32(ctx, l1, l2, lt1, lt2, rewards, dones, truncations, effective_n_steps, zeros, ninf, B, NA, hp->gamma,
                                        hp->v_min, hp->v_max, hp->clipped_double_q, d1, d2, metrics_out, stream);
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
  // ---- one AdamW over both critics (fasttd3.py:89), clip_grad_norm_ semantics, then the Polyak step (:316-320) in the same launch
  rc = torch_clip_adam(qparams, gq, qm, qv, 2 * nq, sq, *opt_count_io + 1, hp->lr_critic, *hp, metrics_out + 3, st, qtarget, hp->tau,
                       hp->weight_decay);
  if (rc) return rc;
  *opt_count_io += 1;
  return RLX_OK;
}

int rlx_fasttd3_policy_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, const rlx_mlp_desc* qdesc,
                                  const float* qparams, const float* states, const float* critic_states, int64_t B, int64_t* opt_count_io,
                                  const rlx_fasttd3_hparams* hp, float* metrics_out, void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && pm && pv && qdesc && qparams && states && opt_count_io && hp && metrics_out && B > 0, RLX_EINVAL,
              "rlx_fasttd3_policy_update_f32: bad args");
  int A, Oc;
  int rc = td3_check_pair(*pdesc, *qdesc, *hp, &A, &Oc);
  if (rc) return rc;
  RLX_REQUIRE(critic_states || Oc == pdesc->in_dim, RLX_EINVAL,
              "rlx_fasttd3_policy_update_f32: critic obs width != policy obs width needs critic_states");
  const float* cs = critic_states ? critic_states : states;
  hipStream_t st = (hipStream_t)stream;
  bx_release_all(ctx);
  const Chain LP = td3_layout(*pdesc), LQ = td3_layout(*qdesc);
  const int64_t np_ = LP.n_params, nq = LQ.n_params;
  const int NA = hp->nr_atoms, ldc = (Oc + A + 3) & ~3, ldp = (pdesc->in_dim + 3) & ~3;
  const int nblk = div_up(B, 4);
  ChainBufs bp, b1, b2;
  float *xp, *dx1, *dx2, *dhead, *l1, *l2, *d1, *d2, *part, *gp, *xs;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    chain_carve(LP, B, a, &bp);
    chain_carve(LQ, B, a, &b1);
    chain_carve(LQ, B, a, &b2);
    for (float** x : {&xp, &dx1, &dx2}) *x = a.take((size_t)B * ldc);
    dhead = a.take((size_t)B * A);
    for (float** l : {&l1, &l2, &d1, &d2}) *l = a.take((size_t)B * NA);
    part = a.take(nblk);
    gp = a.take(np_);
    xs = a.take((size_t)B * ldp);                               // policy observations at a 16-byte row pitch
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc || !sq) return RLX_ENOMEM;
  const float inv_b = 1.0f / (float)B;
  const uint32_t no_key[2] = {0, 0};
  BxReleaseAll bx_all{ctx};
  {
    const NetRef nets[3] = {{pparams, &LP, true}, {qparams, &LQ, true}, {qparams + nq, &LQ, true}};
    rc = trunk_images(ctx, nets, 3, B, st);
    if (rc) return rc;
  }
  // policy on s, its action straight into the critics' input rows, both critics (one per stream), seeds
  rc = fs_concat(cs, Oc, nullptr, A, xp, ldc, B, st);
  if (!rc) rc = fs_concat(states, pdesc->in_dim, nullptr, 0, xs, ldp, B, st);
  if (!rc) rc = chain_fwd(ctx, LP, pparams, xs, ldp, bp, nullptr, B, st);
  if (!rc) rc = td3_head_act(LP, pparams, bp.H[LP.n_hidden - 1], B, TD_NOISE_NONE, nullptr, 0.f, 0.f, no_key, 0, nullptr, 0, B, xp, ldc, Oc,
                             nullptr, 0, nullptr, nullptr, st);
  FsFork fk(ctx, st);
  if (!rc) rc = fk.begin();
  if (!rc) rc = fk.fork();
  if (!rc) rc = chain_fwd(ctx, LQ, qparams + nq, xp, ldc, b2, l2, B, fk.side());
  if (!rc) rc = chain_fwd(ctx, LQ, qparams, xp, ldc, b1, l1, B, fk.main());
  if (!rc) rc = fk.join();
  if (rc) return rc;
  hipLaunchKernelGGL(k_td3_policy_seed, dim3(nblk), dim3(256), 0, st, (const float*)l1, (const float*)l2, d1, d2, part, B, NA, hp->v_min,
                     hp->v_max, hp->clipped_double_q, inv_b);
  RLX_LAUNCH_CHECK();
  {
    BwdPass bwd(ctx, B);
    rc = bwd.begin(2 * chain_stage_floats(ctx, LQ, B, false) + chain_stage_floats(ctx, LP, B, true));
    if (rc) return rc;
    // the critics' input gradients on the action columns (no parameter gradients; one critic per stream), then the policy's backward
    rc = fk.fork();
    if (!rc) rc = chain_bwd(ctx, LQ, qparams + nq, xp, ldc, b2, d2, nullptr, dx2, ldc, B, fk.side(), Oc, A);
    if (!rc) rc = chain_bwd(ctx, LQ, qparams, xp, ldc, b1, d1, nullptr, dx1, ldc, B, fk.main(), Oc, A);
    if (!rc) rc = fk.join();
    if (rc) return rc;
    rc = dpg_tanh_bwd(xp, dx1, dx2, ldc, Oc, dhead, B, A, st);   // (dpg.h: shared with td3.hip)
    if (!rc) rc = chain_bwd(ctx, LP, pparams, xs, ldp, bp, dhead, gp, nullptr, 0, B, st);
    if (!rc) rc = bwd.finish(st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_td3_policy_loss, dim3(1), dim3(256), 0, st, (const float*)part, nblk, inv_b, metrics_out);
  RLX_LAUNCH_CHECK();
  rc = torch_clip_adam(pparams, gp, pm, pv, np_, sq, *opt_count_io + 1, hp->lr_policy, *hp, metrics_out + 1, st, nullptr, 0.f, hp->weight_decay);
  if (rc) return rc;
  *opt_count_io += 1;
  return RLX_OK;
}

}  // extern "C"
