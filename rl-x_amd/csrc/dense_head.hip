// dense_head.hip -- the kernels every network pass of fastsac.hip, fasttd3.hip, reppo.hip, mpo.hip and espo.hip shares (net_pass.h
// declares their launchers): the dense heads (forward, input gradient, weight / bias gradient partials), the [obs | action] row concat,
// the N(0, 1) noise block, and the row norm + activation kernels of a Block with their one launcher (norm_act), among them the
// fused Dropout -> LayerNorm -> ReLU block of droq.hip's critics (k_drop_ln_relu).
#include "ln_kernels.h"
#include "net_pass.h"
#include "sac_sample.h"

namespace rlx {

// Dense heads (nr_atoms = 101 or 2 * act_dim outputs: widths the float4-tiled GEMM stages do not take -- their contraction and
// leading dimensions have to be multiples of four).  Any K (the callers' widths end at 1024) and N; small next to the trunk, so
// plain kernels.
// out[M, N] = H[M, K] @ W[K, N] + b: a workgroup of 128 threads per 8 rows x 128 columns, thread <-> output column.  The H values
// of a row are the same for every lane: their addresses are wave-uniform, so they arrive through the scalar cache as SGPR operands
// of the FMAs -- no LDS, no barrier, eight W loads in flight per thread.  (With H in LDS the kernel was LDS-issue bound: eight
// broadcast reads per k and wave; 22 -> 34 us when the W tiles went through LDS as well.)  One ascending fmaf chain per output.
__global__ __launch_bounds__(128) void k_fs_head_fwd(const float* __restrict__ H, const float* __restrict__ W, const float* __restrict__ b,
                                                     float* __restrict__ out, int64_t M, int K, int N) {
  const int64_t r0 = (int64_t)blockIdx.x * 8;
  const int n = blockIdx.y * 128 + threadIdx.x;
  const int nc = n < N ? n : N - 1;                      // (idle lanes compute a copy of the last column)
  const float* hr[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) hr[r] = H + (r0 + r < M ? r0 + r : M - 1) * K;
  float acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) acc[r] = 0.f;
  int k = 0;
  for (; k + 8 <= K; k += 8) {
    float w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) w[u] = W[(int64_t)(k + u) * N + nc];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[r] = fmaf(hr[r][k + u], w[u], acc[r]);
    }
  }
  for (; k < K; ++k) {
    const float w = W[(int64_t)k * N + nc];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = fmaf(hr[r][k], w, acc[r]);
  }
  if (n < N) {
    const float bv = b[n];
#pragma unroll
    for (int r = 0; r < 8; ++r)
      if (r0 + r < M) out[(r0 + r) * N + n] = acc[r] + bv;
  }
}
// dH[M, K] = d[M, N] @ W[K, N]^T: a workgroup per 8 rows, d rows in LDS, thread <-> input column k.  ACT != NONE: dH holds the
// output H of a plain ACT block on entry and that block's dZ = dH act'(H) on exit (each entry is read by the thread that overwrites
// it).  ReLU is a select, not a product: dH * 0 would be -0 / NaN where dH is negative / non-finite.
template <int ACT>
__global__ __launch_bounds__(256) void k_fs_head_dx(const float* __restrict__ d, const float* __restrict__ W, float* __restrict__ dH,
                                                    int64_t M, int K, int N) {
  extern __shared__ float s_d[];   // [8][N]
  const int64_t r0 = (int64_t)blockIdx.x * 8;
  {
    const int64_t left = (M - r0) * N;
    lds_stage<256, float>(s_d, d + r0 * N, 8 * N, left < 8 * N ? (int)left : 8 * N, 0.f);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += 256) {
    float acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0.f;
    const float* wr = W + (int64_t)k * N;
    for (int n = 0; n < N; ++n) {
      const float w = wr[n];
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] = fmaf(s_d[r * N + n], w, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
      if (r0 + r < M) {
        if (ACT == RLX_ACT_RELU) acc[r] = dH[(r0 + r) * K + k] > 0.f ? acc[r] : 0.f;
        else if (ACT != RLX_ACT_NONE) acc[r] = acc[r] * act_grad_from_out(dH[(r0 + r) * K + k], ACT);
        dH[(r0 + r) * K + k] = acc[r];
      }
  }
}
// partial[s][K * N + N]: dW = H^T d and db = column sums of d over the rows [s * rows, (s + 1) * rows) -- summed in row order;
// the slabs are added in slab order by the reduction kernel.  blockIdx.y = slab, thread <-> (k, n) pairs.
__global__ __launch_bounds__(256) void k_fs_head_dw(const float* __restrict__ H, const float* __restrict__ d, float* __restrict__ partial,
                                                    int64_t M, int K, int N, int rows, int64_t PS, int boff) {
  const int64_t r0 = (int64_t)blockIdx.y * rows;
  const int64_t r1 = r0 + rows < M ? r0 + rows : M;
  float* out = partial + (int64_t)blockIdx.y * PS;
  const int total = K * N + N;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    float acc = 0.f;
    if (e < K * N) {
      const int k = e / N, n = e - k * N;
      for (int64_t r = r0; r < r1; ++r) acc = fmaf(H[r * K + k], d[r * N + n], acc);
    } else {
      const int n = e - K * N;
      for (int64_t r = r0; r < r1; ++r) acc += d[r * N + n];
    }
    out[e < K * N ? e : boff + (e - K * N)] = acc;
  }
}

// The same partials from a register tile: workgroup = slab, thread = 8 k x NJ n outputs (k = 8 tk .. 8 tk + 7, n = tn + TN j),
// 16-row chunks of H and d staged in LDS; every output is one ascending fmaf chain over the slab's rows like above.  (The
// per-output loop above re-reads H and d from L2 for every output: 134 us at [8192, 192] x [8192, 101]; this one 10.)
// Slab layout: [K * N] dW, then db at float `boff` (both 16-byte aligned when the caller pads: vector path of the reduction).
template <int NJ>
__global__ __launch_bounds__(256) void k_fs_head_dw_tiled(const float* __restrict__ H, const float* __restrict__ d,
                                                          float* __restrict__ partial, int64_t M, int K, int N, int rows, int TK, int TN,
                                                          int64_t PS, int boff) {
  extern __shared__ __attribute__((aligned(16))) float s_hd[];
  constexpr int RC = 16;
  float* Hs = s_hd;              // [RC][K]
  float* Ds = s_hd + RC * K;     // [RC][N]
  const int tk = threadIdx.x / TN, tn = threadIdx.x - tk * TN;
  const bool on = tk < TK;
  float acc[8][NJ], bsum[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    bsum[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i][j] = 0.f;
  }
  const int64_t r0 = (int64_t)blockIdx.x * rows;
  const int64_t r1 = r0 + rows < M ? r0 + rows : M;
  for (int64_t c0 = r0; c0 < r1; c0 += RC) {
    const int nr = (int)(r1 - c0 < RC ? r1 - c0 : RC);
    __syncthreads();
    lds_stage<256, float>(Hs, H + c0 * K, RC * K, nr * K, 0.f);
    lds_stage<256, float>(Ds, d + c0 * N, RC * N, nr * N, 0.f);
    __syncthreads();
    if (on) {
#pragma unroll 2
      for (int r = 0; r < RC; ++r) {
        const float4 h0 = *reinterpret_cast<const float4*>(Hs + r * K + 8 * tk);
        const float4 h1 = *reinterpret_cast<const float4*>(Hs + r * K + 8 * tk + 4);
        const float hv[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int n = tn + TN * j;
          const float dv = n < N ? Ds[r * N + n] : 0.f;
          bsum[j] += dv;
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i][j] = fmaf(hv[i], dv, acc[i][j]);
        }
      }
    }
  }
  if (!on) return;
  float* out = partial + (int64_t)blockIdx.x * PS;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = tn + TN * j;
    if (n >= N) continue;
#pragma unroll
    for (int i = 0; i < 8; ++i) out[(int64_t)(8 * tk + i) * N + n] = acc[i][j];
    if (tk == 0) out[boff + n] = bsum[j];
  }
}

// [obs | action] rows of a critic input (row stride ld; the action columns may be filled later by k_fs_sample)
__global__ __launch_bounds__(256) void k_fs_concat(const float* __restrict__ obs, int Oc, const float* __restrict__ act, int A,
                                                   float* __restrict__ out, int ld, int64_t M) {
  const int64_t n = M * ld;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / ld;
    const int c = (int)(i - r * ld);
    out[i] = c < Oc ? obs[r * Oc + c] : (act && c < Oc + A ? act[r * A + (c - Oc)] : 0.f);
  }
}

// N(0, 1) draws of an [n] block: normal(bits(key, i of n))
__global__ __launch_bounds__(256) void k_normal_noise(float* __restrict__ out, int64_t n, uint32_t k0, uint32_t k1, int scheme) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = normal_from_bits(random_bits_at(k0, k1, (uint64_t)i, (uint64_t)n, scheme));
}

// torch.nn.RMSNorm(D) (weight only) + activation over [M, D], D % 64 == 0, D <= 768: one wave per row.
//   fwd: Y = act((Z * rsqrt(mean(Z^2) + eps)) * g)          (Z kept for the backward)
//   bwd: dY (in place) -> dZ = r (dxh - xh mean(dxh xh)),  dxh = dY act'(y) g;  per-block partial dg -> partials[grid][D]
// SiLU' comes from the recomputed pre-activation (ln_kernels.h does the same for the LayerNorm blocks).
template <bool BWD, int ACT>
__global__ __launch_bounds__(256) void k_rms_act(const float* __restrict__ Z, float* __restrict__ Y, const float* __restrict__ g,
                                                 float* __restrict__ partials, int64_t M, int D, float eps) {
  constexpr int NJMAX = 12;
  extern __shared__ __attribute__((aligned(16))) float smem[];   // bwd: [4][D]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int NJ = D >> 6;
  float gam[NJMAX], dg[NJMAX];
#pragma unroll
  for (int j = 0; j < NJMAX; ++j) {
    gam[j] = j < NJ ? g[lane + 64 * j] : 0.f;
    dg[j] = 0.f;
  }
  const float invD = 1.0f / (float)D;
  for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < M; row += (int64_t)gridDim.x * 4) {
    float z[NJMAX], dy[NJMAX];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NJMAX; ++j) {
      z[j] = j < NJ ? Z[row * D + lane + 64 * j] : 0.f;
      if (BWD) dy[j] = j < NJ ? Y[row * D + lane + 64 * j] : 0.f;
      ss += z[j] * z[j];
    }
    ss = wave_sum(ss);
    const float r = rsqrtf(ss * invD + eps);
    if (!BWD) {
#pragma unroll
      for (int j = 0; j < NJMAX; ++j)
        if (j < NJ) {
          const float y = (z[j] * r) * gam[j];
          Y[row * D + lane + 64 * j] = ACT == RLX_ACT_SILU ? silu_fwd(y) : y;
        }
    } else {
      float m2 = 0.f, xh[NJMAX], dxh[NJMAX];
#pragma unroll
      for (int j = 0; j < NJMAX; ++j) {
        xh[j] = z[j] * r;
        const float y = xh[j] * gam[j];
        const float d = (j < NJ) ? dy[j] * (ACT == RLX_ACT_SILU ? silu_grad(y) : 1.f) : 0.f;
        dg[j] += d * xh[j];
        dxh[j] = d * gam[j];
        m2 += dxh[j] * xh[j];
      }
      m2 = wave_sum(m2) * invD;
#pragma unroll
      for (int j = 0; j < NJMAX; ++j)
        if (j < NJ) Y[row * D + lane + 64 * j] = r * (dxh[j] - xh[j] * m2);
    }
  }
  if (BWD) {
#pragma unroll
    for (int j = 0; j < NJMAX; ++j)
      if (j < NJ) smem[w * D + lane + 64 * j] = dg[j];
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += 256)
      partials[(int64_t)blockIdx.x * D + i] = (smem[i] + smem[D + i]) + (smem[2 * D + i] + smem[3 * D + i]);
  }
}

// LayerNorm + tanh, forward / backward (ln_kernels.h with the activation as a compile-time constant); eps is the block's: MPO's
// torch.nn.LayerNorm 1e-5, FastMPO's `mpo` network kind flax's 1e-6
template <bool BWD>
__global__ __launch_bounds__(256) void k_mpo_ln_tanh(const float* __restrict__ Z, float* __restrict__ Y, const float* __restrict__ g,
                                                     const float* __restrict__ be, float* __restrict__ partials, int64_t M, int D,
                                                     float eps) {
  ln_act_body<BWD, 8, RLX_ACT_TANH>(Z, Y, g, be, partials, M, D, RLX_ACT_TANH, eps);
}

// Dropout -> LayerNorm (flax: eps 1e-6, "fast variance") -> ReLU, forward / backward, over [M, D] (droq/flax/critic.py:27-30 and
// :31-34 in one launch; ln_act_body's layout: one wave per row, four rows per workgroup, D % 64 == 0, D <= 64 NJMAX).
//   fwd: z' = kept ? z / keep : 0; Y = relu(LN(z') g + be).  Z stays pre-dropout and nothing else is written.
//   bwd: dY (in Y) -> dZ = (kept / keep) LNbwd(dY relu'); the statistics are recomputed from Z and the regenerated mask;
//        per-workgroup partials [grid][2 D] of [dg | db], as ln_act_body leaves them.
// The mask is no buffer: the row's layer key (three dependent threefry blocks, wave-uniform, droq_layer_key) is taken once per row
// and every lane draws its own units' bits, one threefry block per element; a lane's flags are the bits of one register.
// DROP = false makes no draws: a plain LayerNorm + ReLU block with ln_act_body's arithmetic.
struct DropArgs { uint32_t k0, k1; int scheme; uint32_t base, stride, count, j, E, l, L; float keep; };
template <bool BWD, int NJMAX, bool DROP>
__global__ __launch_bounds__(256) void k_drop_ln_relu(const float* __restrict__ Z, float* __restrict__ Y, const float* __restrict__ g,
                                                      const float* __restrict__ be, float* __restrict__ partials, int64_t M, int D,
                                                      DropArgs da) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // bwd: [4][2*D]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int NJ = D >> 6;
  float gam[NJMAX], bet[NJMAX], dg[NJMAX], db[NJMAX];
#pragma unroll
  for (int j = 0; j < NJMAX; ++j) {
    gam[j] = j < NJ ? g[lane + 64 * j] : 0.f;
    bet[j] = j < NJ ? be[lane + 64 * j] : 0.f;
    dg[j] = db[j] = 0.f;
  }
  const float invD = 1.0f / (float)D;
  for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < M; row += (int64_t)gridDim.x * 4) {
    uint32_t kept = 0xffffffffu;   // bit j: unit lane + 64 j is kept
    if (DROP) {
      uint32_t lk0, lk1;
      droq_layer_key(da.k0, da.k1, da.scheme, da.base + da.stride * (uint32_t)row, da.count, da.j, da.E, da.l, da.L, lk0, lk1);
      kept = 0u;
#pragma unroll
      for (int j = 0; j < NJMAX; ++j)
        if (j < NJ && droq_unit_kept(lk0, lk1, da.scheme, (uint32_t)(lane + 64 * j), (uint32_t)D, da.keep)) kept |= 1u << j;
    }
    float z[NJMAX], dy[NJMAX];
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int j = 0; j < NJMAX; ++j) {
      z[j] = j < NJ ? Z[row * D + lane + 64 * j] : 0.f;
      if (DROP) z[j] = (kept >> j) & 1u ? z[j] / da.keep : 0.f;
      if (BWD) dy[j] = j < NJ ? Y[row * D + lane + 64 * j] : 0.f;
      s += z[j];
      ss += z[j] * z[j];
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    const float mean = s * invD;
    const float rstd = rsqrtf(fmaxf(0.f, ss * invD - mean * mean) + 1e-6f);
    if (!BWD) {
#pragma unroll
      for (int j = 0; j < NJMAX; ++j)
        if (j < NJ) Y[row * D + lane + 64 * j] = fmaxf((z[j] - mean) * rstd * gam[j] + bet[j], 0.f);
    } else {
      float m1 = 0.f, m2 = 0.f, xh[NJMAX], dxh[NJMAX];
#pragma unroll
      for (int j = 0; j < NJMAX; ++j) {
        xh[j] = (z[j] - mean) * rstd;
        const float yv = xh[j] * gam[j] + bet[j];
        const float d = (j < NJ && yv > 0.f) ? dy[j] : 0.f;
        dg[j] += d * xh[j];
        db[j] += d;
        dxh[j] = d * gam[j];
        m1 += dxh[j];
        m2 += dxh[j] * xh[j];
      }
      m1 = wave_sum(m1) * invD;
      m2 = wave_sum(m2) * invD;
#pragma unroll
      for (int j = 0; j < NJMAX; ++j)
        if (j < NJ) {
          const float dz = rstd * (dxh[j] - m1 - xh[j] * m2);
          Y[row * D + lane + 64 * j] = DROP ? ((kept >> j) & 1u ? dz / da.keep : 0.f) : dz;
        }
    }
  }
  if (BWD) {
#pragma unroll
    for (int j = 0; j < NJMAX; ++j)
      if (j < NJ) {
        smem[w * 2 * D + lane + 64 * j] = dg[j];
        smem[w * 2 * D + D + lane + 64 * j] = db[j];
      }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * D; i += 256)
      partials[(int64_t)blockIdx.x * 2 * D + i] = (smem[i] + smem[2 * D + i]) + (smem[4 * D + i] + smem[6 * D + i]);
  }
}
// the lean form holds D <= 256 (the reference's default width, droq/flax/default_config.py), the wide one D <= 768
template <bool BWD>
static int launch_drop_ln_relu(const Block& o, const float* p, const float* Z, float* Y, float* part, int grid, int64_t M, size_t lds,
                               hipStream_t st, const DropKeys* dk) {
  RLX_REQUIRE(o.drop >= 0.f && o.drop < 1.f, RLX_EINVAL, "norm_act: a block's dropout rate must be in [0, 1)");
  RLX_REQUIRE(o.drop == 0.f || dk, RLX_EINVAL, "norm_act: a block with dropout needs the pass's dropout keys");
  const int D = o.out;
  DropArgs da{};
  if (o.drop > 0.f)
    da = DropArgs{dk->k0, dk->k1, dk->scheme, dk->base, dk->stride, dk->count, (uint32_t)dk->j, (uint32_t)dk->E, (uint32_t)dk->l,
                  (uint32_t)dk->L, 1.0f - o.drop};
#define RLX_DROP_LN(NJMAX, DROP) \
  hipLaunchKernelGGL((k_drop_ln_relu<BWD, NJMAX, DROP>), dim3(grid), dim3(256), lds, st, Z, Y, p + o.g, p + o.be, part, M, D, da)
  if (D <= 256) {
    if (o.drop > 0.f) RLX_DROP_LN(4, true);
    else RLX_DROP_LN(4, false);
  } else {
    if (o.drop > 0.f) RLX_DROP_LN(12, true);
    else RLX_DROP_LN(12, false);
  }
#undef RLX_DROP_LN
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int fs_head_fwd(const float* H, const float* W, const float* b, float* out, int64_t M, int K, int N, hipStream_t st) {
  hipLaunchKernelGGL(k_fs_head_fwd, dim3(div_up(M, 8), div_up(N, 128)), dim3(128), 0, st, H, W, b, out, M, K, N);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int fs_head_bwd(rlx_ctx* ctx, float* H_dH, const float* W, const float* d, float* gW, float* gb, int64_t M, int K, int N, hipStream_t st,
                int act) {
  RLX_REQUIRE(act == RLX_ACT_NONE || act == RLX_ACT_RELU || act == RLX_ACT_TANH || act == RLX_ACT_ELU, RLX_EUNSUP,
              "fs_head_bwd: the input-gradient epilogue takes no activation, ReLU, tanh or ELU");
  if (gW) {
    const int boff = (K * N + 3) & ~3;
    const int64_t PS = boff + ((N + 3) & ~3);
    const int TK = K / 8, TN = TK > 0 && TK <= 256 ? 256 / TK : 0;
    const int nj = TN ? div_up(N, TN) : 99;
    const bool tiled = K % 8 == 0 && nj <= 12 && (size_t)16 * (K + N) * sizeof(float) <= 48 * 1024;
    const int rows = tiled ? (M >= 8192 ? 32 : 64) : 128, S = div_up(M, rows);   // (>= 256 slabs: one per CU)
    float* part = stage_alloc(ctx, (size_t)S * PS);
    if (!part) return RLX_ENOMEM;
    if (tiled) {
      const size_t lds = (size_t)16 * (K + N) * sizeof(float);
#define FS_DW_TILED(NJ) hipLaunchKernelGGL(k_fs_head_dw_tiled<NJ>, dim3(S), dim3(256), lds, st, (const float*)H_dH, d, part, M, K, N, rows, TK, TN, PS, boff)
      if (nj <= 2) FS_DW_TILED(2);
      else if (nj <= 4) FS_DW_TILED(4);
      else if (nj <= 8) FS_DW_TILED(8);
      else FS_DW_TILED(12);
#undef FS_DW_TILED
    } else {
      int gx = div_up(K * N + N, 256);
      if (gx > 64) gx = 64;
      hipLaunchKernelGGL(k_fs_head_dw, dim3(gx, S), dim3(256), 0, st, (const float*)H_dH, d, part, M, K, N, rows, PS, boff);
    }
    RLX_LAUNCH_CHECK();
    ReduceTable tab;
    tab.n = 0;
    tab.seg[tab.n++] = ReduceSeg{part, gW, (int64_t)K * N, PS, S, 0, 1.f, 0.f, 1};
    tab.seg[tab.n++] = ReduceSeg{part + boff, gb, (int64_t)N, PS, S, 0, 1.f, 0.f, 1};
    const int rc = stage_reduce(ctx, tab, nullptr, nullptr, st);
    if (rc) return rc;
  }
#define FS_HEAD_DX(ACT) hipLaunchKernelGGL(k_fs_head_dx<ACT>, dim3(div_up(M, 8)), dim3(256), (size_t)8 * N * sizeof(float), st, d, W, H_dH, M, K, N)
  if (act == RLX_ACT_RELU) FS_HEAD_DX(RLX_ACT_RELU);
  else if (act == RLX_ACT_TANH) FS_HEAD_DX(RLX_ACT_TANH);
  else if (act == RLX_ACT_ELU) FS_HEAD_DX(RLX_ACT_ELU);
  else FS_HEAD_DX(RLX_ACT_NONE);
#undef FS_HEAD_DX
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int fs_concat(const float* obs, int Oc, const float* act, int A, float* out, int ld, int64_t M, hipStream_t st) {
  int grid = div_up(M * ld, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(k_fs_concat, dim3(grid), dim3(256), 0, st, obs, Oc, act, A, out, ld, M);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int launch_normal_noise(float* out, int64_t n, uint32_t k0, uint32_t k1, int scheme, hipStream_t st) {
  hipLaunchKernelGGL(k_normal_noise, dim3(elem_grid(n)), dim3(256), 0, st, out, n, k0, k1, scheme);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

template <bool BWD>
static int norm_act_t(const Block& o, const float* p, const float* Z, float* Y, float* part, int grid, int64_t M, hipStream_t st,
                      const DropKeys* dk) {
  const int D = o.out;
  const size_t row = BWD ? (size_t)D * sizeof(float) : 0;   // LDS: four waves of [dg | db] (LayerNorm) or [dg] (RMSNorm)
  const bool ln = o.norm == NORM_LAYER, th = o.act == RLX_ACT_TANH;
  RLX_REQUIRE(D % 64 == 0 && D <= (th ? 512 : 768), RLX_EUNSUP, "norm_act: the row-norm kernels hold a row in one wave");
  if (ln && o.act == RLX_ACT_RELU && o.eps == 1e-6f) return launch_drop_ln_relu<BWD>(o, p, Z, Y, part, grid, M, 8 * row, st, dk);
  RLX_REQUIRE(o.drop == 0.f, RLX_EUNSUP, "norm_act: dropout has a kernel in front of (LayerNorm eps 1e-6, ReLU) only");
  if (ln && o.act == RLX_ACT_SILU)      // (the activation as a run-time argument: k_ln_act_wide takes the switch once per launch)
    hipLaunchKernelGGL(k_ln_act_wide<BWD>, dim3(grid), dim3(256), 8 * row, st, Z, Y, p + o.g, p + o.be, part, M, D, o.act, o.eps);
  else if (ln && th)
    hipLaunchKernelGGL(k_mpo_ln_tanh<BWD>, dim3(grid), dim3(256), 8 * row, st, Z, Y, p + o.g, p + o.be, part, M, D, o.eps);
  else if (o.norm == NORM_RMS && o.act == RLX_ACT_SILU)
    hipLaunchKernelGGL((k_rms_act<BWD, RLX_ACT_SILU>), dim3(grid), dim3(256), 4 * row, st, Z, Y, p + o.g, part, M, D, o.eps);
  else RLX_REQUIRE(false, RLX_EUNSUP, "norm_act: no kernel for this (norm, activation, eps)");
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
int norm_act(const Block& o, const float* p, const float* Z, float* Y, float* part, int grid, int64_t M, hipStream_t st,
             const DropKeys* dk) {
  return part ? norm_act_t<true>(o, p, Z, Y, part, grid, M, st, dk) : norm_act_t<false>(o, p, Z, Y, part, grid, M, st, dk);
}

}  // namespace rlx
