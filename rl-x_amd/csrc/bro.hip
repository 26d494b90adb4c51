// bro.hip -- the kernels of the reference's BRO family (rl_x/algorithms/bro/flax): BroNet's post-norm residual LayerNorm rows
// (layers.py:10-29), forward and backward, a normalise-on-load Dense layer for forward passes of few rows, and the pairwise
// quantile-Huber critic loss (bro.py:29-32, :179-189); and the entry points rlx_bro_net_f32 (the network, bro_net.h) and
// rlx_bro_quantile_loss_f32.  float32 throughout, every sum in a fixed order, no atomics: identical calls give identical bits.
//
// Row kernels (k_bro_ln, k_bro_ln_bwd): hyper.hip's shape.  One wave per row, four rows per workgroup, rows grid-strided; lane l
// holds the 16-byte chunks l, l + 64, ... of a row of H <= 1024 floats (NQ = ceil(H / 256) <= 4) from its one load to its one store.
// Statistics as ln_kernels.h: mean and E[z^2] by wave butterflies, variance E[z^2] - mean^2 clamped at 0, rsqrtf.  The forward keeps
// (mean, rstd) per row; the backward rebuilds x^ = (z - mean) rstd from them and the kept z, writes d z, stores the sum of the two
// arriving gradients where the residual branch carries it on, and keeps d g / d b of its columns in registers over the rows it walks.
// After the walk the four waves fold through LDS in wave order into one partial row [d g | d b] per workgroup; stage_reduce finishes.
//
// k_bro_layer: zout = f(in) W + bias for one Dense layer, f the LayerNorm (+ ReLU, or + residual) of the layer in front.
// A workgroup owns 32 rows x 64 output columns; the grid is ceil(M / 32) x ceil(N / 64), so 128 rows of a 512-wide layer are 32
// workgroups where a 128 x 128 GEMM tile gives 8.  Prologue: wave w takes the tile's rows w, w + 4, ...: the raw row comes from
// memory into registers as chunks (the row kernels' layout), the statistics are two butterflies, and the normalised row -- the
// layer's true input -- goes to LDS once, [32][K + 1] floats (the odd stride keeps the 32 rows of an A fragment on 32 banks).  Every
// column strip repeats this cheap prologue on the same rows in the same order, so all strips hold identical inputs, and each stores
// only its own 64 columns of the new block input x: disjoint slices, no race, no grid barrier.  Main loop: wave w owns the column
// tile w & 1 and the K half w >> 1; A fragments come from LDS, B fragments straight from W in memory (32 consecutive floats of two
// rows per load, each element read once per row tile), on v_mfma_f32_32x32x2_f32, the exact-fp32 instruction of gemm.h.  The two K
// halves meet in LDS, lower half first; the bias is added and the raw z stored.  Ragged shapes are guards: rows >= M and first-layer
// columns >= K are zeros in LDS, weight columns >= N are never loaded and never stored.
//
// k_bro_qloss: one wave per batch row.  The row's target quantiles y and both critics' predictions sit in the wave's LDS rows; lane
// i (and i + 64) owns predicted quantile i, walks the targets j in order and keeps its gradient as a private sum; the row's loss is
// a wave butterfly.  A workgroup adds its waves' losses in wave order into one partial; k_bro_qloss_fold adds the partials in order.
#include "bro_net.h"

namespace rlx {

__device__ __forceinline__ float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ __forceinline__ float4 operator+(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 operator-(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 operator*(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 operator*(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float sum4(float4 a) { return (a.x + a.y) + (a.z + a.w); }
__device__ __forceinline__ float4 relu4(float4 a) { return make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f)); }
// g where y > 0, else 0
__device__ __forceinline__ float4 mask4(float4 g, float4 y) {
  return make_float4(y.x > 0.f ? g.x : 0.f, y.y > 0.f ? g.y : 0.f, y.z > 0.f ? g.z : 0.f, y.w > 0.f ? g.w : 0.f);
}
// chunk j of a row of nch chunks (zeros beyond the row: they add nothing to a sum)
__device__ __forceinline__ float4 ld_chunk(const float* row, int j, int nch) {
  return j < nch ? reinterpret_cast<const float4*>(row)[j] : f4(0.f);
}
__device__ __forceinline__ void st_chunk(float* row, int j, int nch, float4 v) {
  if (j < nch) reinterpret_cast<float4*>(row)[j] = v;
}
// (mean, rstd) of a row held as chunks: flax's fast variance
template <int NQ>
__device__ __forceinline__ float2 row_stats(const float4 (&z)[NQ], float invH, float eps) {
  float s = 0.f, ss = 0.f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    s += sum4(z[q]);
    ss += sum4(z[q] * z[q]);
  }
  const float mean = wave_sum(s) * invH;
  return make_float2(mean, rsqrtf(fmaxf(0.f, wave_sum(ss) * invH - mean * mean) + eps));
}

// ------------------------------------------------------------------------------------------------------------ row kernels
struct LnArgs {
  const float *z, *g, *be, *x;      // x: the residual (RES)
  float *out, *stats;               // forward
  const float *d, *d2;              // backward: the arriving gradient d (+ d2)
  float *dz, *dres, *part;          // backward: d z, d + d2 (RES with d2), [grid, 2 H] partial [d g | d b]
  float eps;
  int H;
  int64_t M;
};

// RES 0: y = relu(LN(z) g + b);  RES 1: x' = LN(z) g + b + x
template <int NQ, int RES>
__global__ __launch_bounds__(256) void k_bro_ln(const LnArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nch = a.H >> 2;
  const float invH = 1.0f / (float)a.H;
  float4 g[NQ], be[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    g[q] = ld_chunk(a.g, lane + 64 * q, nch);
    be[q] = ld_chunk(a.be, lane + 64 * q, nch);
  }
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < a.M; row += (int64_t)gridDim.x * 4) {
    float4 z[NQ], x[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      z[q] = ld_chunk(a.z + row * a.H, lane + 64 * q, nch);
      if (RES) x[q] = ld_chunk(a.x + row * a.H, lane + 64 * q, nch);
    }
    const float2 ms = row_stats<NQ>(z, invH, a.eps);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float4 y = ((z[q] - f4(ms.x)) * ms.y) * g[q] + be[q];
      st_chunk(a.out + row * a.H, lane + 64 * q, nch, RES ? y + x[q] : relu4(y));
    }
    if (a.stats && lane == 0) {
      a.stats[2 * row] = ms.x;
      a.stats[2 * row + 1] = ms.y;
    }
  }
}

// From d y = (d + d2) [* 1[y > 0], RES 0]:  d g = sum_rows d y x^,  d b = sum_rows d y,  d x^ = d y g,
//   d z = rstd (d x^ - mean(d x^) - x^ mean(d x^ x^))
template <int NQ, int RES>
__global__ __launch_bounds__(256) void k_bro_ln_bwd(const LnArgs a) {
  __shared__ float4 fold[3 * 2 * NQ * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nch = a.H >> 2;
  const float invH = 1.0f / (float)a.H;
  float4 g[NQ], be[NQ], dg[NQ], db[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    g[q] = ld_chunk(a.g, lane + 64 * q, nch);
    be[q] = RES ? f4(0.f) : ld_chunk(a.be, lane + 64 * q, nch);
    dg[q] = db[q] = f4(0.f);
  }
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < a.M; row += (int64_t)gridDim.x * 4) {
    float4 xh[NQ], dy[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      xh[q] = ld_chunk(a.z + row * a.H, lane + 64 * q, nch);
      dy[q] = ld_chunk(a.d + row * a.H, lane + 64 * q, nch);
      if (a.d2) dy[q] = dy[q] + ld_chunk(a.d2 + row * a.H, lane + 64 * q, nch);
    }
    const float mean = a.stats[2 * row], rstd = a.stats[2 * row + 1];
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (RES && a.d2) st_chunk(a.dres + row * a.H, lane + 64 * q, nch, dy[q]);
      // (beyond the row a chunk is zeros: x^ = -mean rstd there, but d y = 0 keeps it out of every sum)
      xh[q] = (xh[q] - f4(mean)) * rstd;
      if (!RES) dy[q] = mask4(dy[q], xh[q] * g[q] + be[q]);
      dg[q] = dg[q] + dy[q] * xh[q];
      db[q] = db[q] + dy[q];
      dy[q] = dy[q] * g[q];      // d x^
      m1 += sum4(dy[q]);
      m2 += sum4(dy[q] * xh[q]);
    }
    m1 = wave_sum(m1) * invH;
    m2 = wave_sum(m2) * invH;
#pragma unroll
    for (int q = 0; q < NQ; ++q) st_chunk(a.dz + row * a.H, lane + 64 * q, nch, (dy[q] - f4(m1) - xh[q] * m2) * rstd);
  }
  // waves 1..3 hand their column sums over, wave 0 adds them in wave order: one partial row [d g | d b] per workgroup
  if (wv) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      fold[((wv - 1) * 2 * NQ + q) * 64 + lane] = dg[q];
      fold[((wv - 1) * 2 * NQ + NQ + q) * 64 + lane] = db[q];
    }
  }
  __syncthreads();
  if (wv == 0) {
    float* pr = a.part + (int64_t)blockIdx.x * 2 * a.H;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float4 tg = dg[q], tb = db[q];
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        tg = tg + fold[(w * 2 * NQ + q) * 64 + lane];
        tb = tb + fold[(w * 2 * NQ + NQ + q) * 64 + lane];
      }
      st_chunk(pr, lane + 64 * q, nch, tg);
      st_chunk(pr + a.H, lane + 64 * q, nch, tb);
    }
  }
}

__global__ __launch_bounds__(256) void k_bro_unpad(const float* __restrict__ src, int ld, int64_t M, int n, float* __restrict__ dst) {
  const int64_t tot = M * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / n;
    dst[i] = src[r * ld + (i - r * n)];
  }
}

// ------------------------------------------------------------------------------------------------------------ the fused layer
constexpr int BRO_TM = 32, BRO_TN = 64;      // a workgroup's rows and output columns
constexpr int BRO_KG = 8;                    // k-pairs (MFMAs) per fragment group
static inline int bro_kpad(int K) { return (K + 31) & ~31; }      // columns of the tile in LDS: both K halves whole fragment groups
static inline size_t bro_layer_lds(int K) { return ((size_t)BRO_TM * (bro_kpad(K) + 1) + 2 * 16 * 64) * sizeof(float); }

template <int MODE, int NQ>
__global__ __launch_bounds__(256) void k_bro_layer(const BroLayer a) {
  extern __shared__ __attribute__((aligned(16))) float bro_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int Kp = (a.K + 31) & ~31, LD = Kp + 1;
  float* As = bro_lds;                      // [32][LD]: the layer's input rows
  float* fold = bro_lds + BRO_TM * LD;      // [2][16][64]: the upper K half's accumulators
  const int64_t row0 = (int64_t)blockIdx.x * BRO_TM;
  const int strip = blockIdx.y;

  // ---- prologue: the tile's rows, normalised on the way, into LDS
  if constexpr (MODE == BRO_IN_RAW) {
    for (int r = wv; r < BRO_TM; r += 4) {
      const int64_t m = row0 + r;
      for (int k = lane; k < Kp; k += 64) As[r * LD + k] = (m < a.M && k < a.K) ? a.in[m * a.K + k] : 0.f;
    }
  } else {
    const int nch = a.K >> 2;
    const float invK = 1.0f / (float)a.K;
    float4 g[NQ], be[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      g[q] = ld_chunk(a.g, lane + 64 * q, nch);
      be[q] = ld_chunk(a.be, lane + 64 * q, nch);
    }
    for (int r = wv; r < BRO_TM; r += 4) {
      const int64_t m = row0 + r;
      float4 v[NQ];
      if (m < a.M) {      // (wave-uniform)
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = ld_chunk(a.in + m * a.K, lane + 64 * q, nch);
        const float2 ms = row_stats<NQ>(v, invK, a.eps);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int j = lane + 64 * q;
          const float4 y = ((v[q] - f4(ms.x)) * ms.y) * g[q] + be[q];
          v[q] = MODE == BRO_IN_RES ? y + ld_chunk(a.xres + m * a.K, j, nch) : relu4(y);
          if (a.xnew && (j >> 4) == strip) st_chunk(a.xnew + m * a.K, j, nch, v[q]);      // chunks 16 s .. 16 s + 15: this strip's columns
        }
      } else {
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = f4(0.f);
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = lane + 64 * q;
        if (j < nch) {
          float* t = As + r * LD + 4 * j;
          t[0] = v[q].x; t[1] = v[q].y; t[2] = v[q].z; t[3] = v[q].w;
        }
      }
    }
  }
  __syncthreads();

  // ---- main loop: wave (ct, kh) = column tile ct of the strip over the K half kh
  const int ct = wv & 1, kh = wv >> 1, li = lane & 31, lh = lane >> 5;
  const int col = strip * BRO_TN + ct * 32 + li;
  const bool col_ok = col < a.N;
  const int kbeg = kh * (Kp >> 1), kend = kbeg + (Kp >> 1);
  const float* ap = As + li * LD + lh;                  // A[i = li][k = lh + .]
  const float* wp = a.W + (col_ok ? col : 0);           // B[k = lh + .][j = li]: W[k, col]
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float fb[BRO_KG], fbn[BRO_KG] = {}, fa[BRO_KG];
  auto load_b = [&](int k0, float (&f)[BRO_KG]) {
#pragma unroll
    for (int q = 0; q < BRO_KG; ++q) {
      const int k = k0 + 2 * q + lh;
      f[q] = (col_ok && k < a.K) ? wp[(int64_t)k * a.N] : 0.f;
    }
  };
  load_b(kbeg, fb);
  for (int k0 = kbeg; k0 < kend; k0 += 2 * BRO_KG) {
    if (k0 + 2 * BRO_KG < kend) load_b(k0 + 2 * BRO_KG, fbn);      // the next group's weights are in flight under this group's MFMAs
#pragma unroll
    for (int q = 0; q < BRO_KG; ++q) fa[q] = ap[k0 + 2 * q];
#pragma unroll
    for (int q = 0; q < BRO_KG; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q], fb[q], acc, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < BRO_KG; ++q) fb[q] = fbn[q];
  }

  // ---- the two K halves meet, lower half first; bias; store (C: col = li, row = (r & 3) + 8 (r >> 2) + 4 lh)
  if (kh) {
#pragma unroll
    for (int r = 0; r < 16; ++r) fold[(ct * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (!kh && col_ok) {
    const float bv = a.bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t m = row0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (m < a.M) a.zout[m * a.N + col] = (acc[r] + fold[(ct * 16 + r) * 64 + lane]) + bv;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ the critic loss
struct QlossArgs {
  const float *q1, *q2, *nq1, *nq2, *rew, *term, *nlogp, *log_alpha;
  float *dq1, *dq2, *part, *y_out;
  int64_t B;
  int N;
  float gamma, pess, kappa;
};
constexpr int QL_MAXN = 128, QL_GROUP = 16;

__global__ __launch_bounds__(256) void k_bro_qloss(const QlossArgs a) {
  __shared__ float sy[4][QL_MAXN], sq[4][2][QL_MAXN], wloss[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, N = a.N;
  const float alpha = (float)exp((double)a.log_alpha[0]);      // entropy_coefficient.py:12
  const float scale = (float)((double)a.B * N);
  float loss = 0.f;      // this wave's rows, in row order
  for (int64_t base = (int64_t)blockIdx.x * 4; base < a.B; base += (int64_t)gridDim.x * 4) {      // (uniform trip count: barriers inside)
    const int64_t b = base + wv;
    const bool on = b < a.B;
    if (on) {
      const float keep = a.gamma * (1.0f - a.term[b]), r = a.rew[b], ent = alpha * a.nlogp[b];
      for (int j = lane; j < N; j += 64) {
        const float n1 = a.nq1[b * N + j], n2 = a.nq2[b * N + j];
        const float nq = (n1 + n2) / 2.0f - a.pess * fabsf(n1 - n2) / 2.0f;
        const float y = r + keep * (nq - ent);
        sy[wv][j] = y;
        sq[wv][0][j] = a.q1[b * N + j];
        sq[wv][1][j] = a.q2[b * N + j];
        if (a.y_out) a.y_out[b * N + j] = y;
      }
    }
    __syncthreads();
    if (on) {
      float rl = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < N) {
          const float tau = ((float)i + 0.5f) / (float)N;
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const float q = sq[wv][c][i];
            float gsum = 0.f, lsum = 0.f;
            for (int j0 = 0; j0 < N; j0 += QL_GROUP) {      // sums of QL_GROUP targets, then the sum of those: shorter chains of roundings
              float gp = 0.f, lp = 0.f;
              const int j1 = j0 + QL_GROUP < N ? j0 + QL_GROUP : N;
              for (int j = j0; j < j1; ++j) {
                const float td = sy[wv][j] - q, ab = fabsf(td);
                const float w = fabsf(tau - (td < 0.f ? 1.0f : 0.0f));
                const bool quad = ab <= a.kappa;
                lp += w * (quad ? 0.5f * td * td : a.kappa * (ab - 0.5f * a.kappa)) / a.kappa;
                gp += w * (quad ? td : copysignf(a.kappa, td)) / a.kappa;
              }
              gsum += gp;
              lsum += lp;
            }
            rl += lsum;
            (c ? a.dq2 : a.dq1)[b * N + i] = -gsum / scale;
          }
        }
      }
      loss += wave_sum(rl);
    }
    __syncthreads();
  }
  if (lane == 0) wloss[wv] = loss;
  __syncthreads();
  if (threadIdx.x == 0) a.part[blockIdx.x] = ((wloss[0] + wloss[1]) + wloss[2]) + wloss[3];
}
// loss = (sum of the n partials, in order) / (B N): one wave
__global__ __launch_bounds__(64) void k_bro_qloss_fold(const float* __restrict__ part, int n, float scale, float* __restrict__ loss_out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) s += part[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) loss_out[0] = s / scale;
}

// ------------------------------------------------------------------------------------------------------------ launchers
#define BRO_ROW_LAUNCH(KERNEL, RES, H, GRID, ST, ARGS)                                     \
  switch (div_up((H) / 4, 64)) {                                                           \
    case 1: hipLaunchKernelGGL((KERNEL<1, RES>), GRID, dim3(256), 0, ST, ARGS); break;     \
    case 2: hipLaunchKernelGGL((KERNEL<2, RES>), GRID, dim3(256), 0, ST, ARGS); break;     \
    case 3: hipLaunchKernelGGL((KERNEL<3, RES>), GRID, dim3(256), 0, ST, ARGS); break;     \
    default: hipLaunchKernelGGL((KERNEL<4, RES>), GRID, dim3(256), 0, ST, ARGS); break;    \
  }                                                                                        \
  RLX_LAUNCH_CHECK()

int bro_ln(const rlx_ctx* ctx, const float* z, const float* g, const float* be, const float* x, float eps, int64_t M, int H, float* out,
           float* stats, hipStream_t st) {
  LnArgs a{};
  a.z = z; a.g = g; a.be = be; a.x = x; a.out = out; a.stats = stats; a.eps = eps; a.H = H; a.M = M;
  const dim3 grid(rows_grid(ctx, M));
  if (x) { BRO_ROW_LAUNCH(k_bro_ln, 1, H, grid, st, a); }
  else { BRO_ROW_LAUNCH(k_bro_ln, 0, H, grid, st, a); }
  return RLX_OK;
}

int bro_ln_bwd(rlx_ctx* ctx, const float* z, const float* stats, const float* g, const float* be, bool res, const float* d, const float* d2,
               int64_t M, int H, float* dz, float* dres, float* g_g, float* g_be, hipStream_t st) {
  const int grid = bwd_rows_grid(ctx, M);
  LnArgs a{};
  a.z = z; a.stats = const_cast<float*>(stats); a.g = g; a.be = be; a.d = d; a.d2 = d2; a.dz = dz; a.dres = dres; a.H = H; a.M = M;
  a.part = stage_alloc(ctx, (size_t)grid * 2 * H);
  if (!a.part) return RLX_ENOMEM;
  if (res) { BRO_ROW_LAUNCH(k_bro_ln_bwd, 1, H, dim3(grid), st, a); }
  else { BRO_ROW_LAUNCH(k_bro_ln_bwd, 0, H, dim3(grid), st, a); }
  return norm_bwd_reduce(ctx, a.part, grid, H, g_g, g_be, st);
}

int bro_unpad(const float* src, int ld, int64_t M, int n, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(k_bro_unpad, dim3(elem_grid(M * n)), dim3(256), 0, st, src, ld, M, n, dst);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

static size_t bro_lds_limit() {      // bytes of LDS one workgroup of the current device may take (0: unknown)
  int dev = 0, lim = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) return 0;
  return (size_t)lim;
}
bool bro_layer_fits(int K) { return bro_layer_lds(K) <= bro_lds_limit(); }

template <int MODE, int NQ>
static int bro_layer_launch(const BroLayer& a, hipStream_t st) {
  static AttrOnce once;
  const size_t lds = bro_layer_lds(a.K);
  if (!once.done()) {      // the widest tile of this instantiation that the device holds
    const size_t widest = bro_layer_lds(MODE == BRO_IN_RAW ? 1024 : 256 * NQ), lim = bro_lds_limit();
    RLX_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_bro_layer<MODE, NQ>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(widest < lim ? widest : lim)));
    once.mark();
  }
  hipLaunchKernelGGL((k_bro_layer<MODE, NQ>), dim3(div_up(a.M, BRO_TM), div_up(a.N, BRO_TN)), dim3(256), lds, st, a);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int bro_layer(const BroLayer& a, hipStream_t st) {
  RLX_REQUIRE(bro_layer_fits(a.K), RLX_EUNSUP, "bro_layer: the 32-row tile of the layer's input does not fit the device's LDS");
  RLX_REQUIRE(!a.xnew || a.N == a.K, RLX_EINVAL, "bro_layer: xnew needs one column strip per 64 input columns (N == K)");
  if (a.mode == BRO_IN_RAW) return bro_layer_launch<BRO_IN_RAW, 1>(a, st);
  const int nq = div_up(a.K / 4, 64);
#define BRO_LAYER_NQ(MODE)                                         \
  switch (nq) {                                                    \
    case 1: return bro_layer_launch<MODE, 1>(a, st);               \
    case 2: return bro_layer_launch<MODE, 2>(a, st);               \
    case 3: return bro_layer_launch<MODE, 3>(a, st);               \
    default: return bro_layer_launch<MODE, 4>(a, st);              \
  }
  if (a.mode == BRO_IN_RES) { BRO_LAYER_NQ(BRO_IN_RES) }
  BRO_LAYER_NQ(BRO_IN_RELU)
#undef BRO_LAYER_NQ
}

static bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t m = 0;
  for (const void* p : ps) m |= (uintptr_t)p;
  return (m & 15) == 0;
}

// the envelope of the descriptor (RLX_EUNSUP, naming the field)
static int bro_check(const rlx_bro_desc& t) {
  RLX_REQUIRE(t.hidden >= 64 && t.hidden % 64 == 0 && t.hidden <= 1024, RLX_EUNSUP,
              "rlx_bro_net_f32: hidden must be a multiple of 64 up to 1024 (the row kernels hold a row in one wave)");
  RLX_REQUIRE(t.n_blocks >= 1 && t.n_blocks <= BRO_MAX_BLOCKS, RLX_EUNSUP, "rlx_bro_net_f32: n_blocks must be 1..4");
  RLX_REQUIRE(t.in_dim >= 1 && t.in_dim <= 1024, RLX_EUNSUP, "rlx_bro_net_f32: in_dim must be 1..1024");
  RLX_REQUIRE(t.out_dim >= 0 && t.out_dim <= 128, RLX_EUNSUP, "rlx_bro_net_f32: out_dim must be 0..128");
  RLX_REQUIRE(t.ln_eps > 0.f && std::isfinite(t.ln_eps), RLX_EUNSUP, "rlx_bro_net_f32: ln_eps must be positive");
  RLX_REQUIRE(t.fwd_path >= 0 && t.fwd_path <= 2, RLX_EUNSUP, "rlx_bro_net_f32: fwd_path must be 0 (default rule), 1 (layered) or 2 (fused)");
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int64_t rlx_bro_param_count(const rlx_bro_desc* desc) {
  if (!desc || desc->in_dim < 1 || desc->hidden < 1 || desc->n_blocks < 1 || desc->n_blocks > BRO_MAX_BLOCKS || desc->out_dim < 0) return -1;
  return make_bro(*desc).n_params;
}

int rlx_bro_net_f32(rlx_ctx* ctx, const rlx_bro_desc* desc, const float* params, const float* x, int64_t M, float* out, const float* d_out,
                    float* grads, float* dx, void* stream) {
  RLX_REQUIRE(ctx && desc && params && x && out, RLX_EINVAL, "rlx_bro_net_f32: NULL pointer (ctx, desc, params, x, out)");
  RLX_REQUIRE(!d_out || grads, RLX_EINVAL, "rlx_bro_net_f32: a backward (d_out) needs grads");
  const int rc = bro_check(*desc);
  if (rc) return rc;
  RLX_REQUIRE(M >= 1 && M <= (1 << 20), RLX_EUNSUP, "rlx_bro_net_f32: M must be 1..2^20 rows");
  RLX_REQUIRE(!(desc->fwd_path == 2 && d_out), RLX_EINVAL, "rlx_bro_net_f32: fwd_path 2 (fused) is forward only; a call with d_out takes the layered route");
  RLX_REQUIRE(aligned16({params, out, d_out, grads}), RLX_EINVAL, "rlx_bro_net_f32: params, out, d_out and grads must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const Bro E = make_bro(*desc);
  const bool bwd = d_out != nullptr;
  const bool fits = bro_layer_fits(E.H > E.in ? E.H : E.in);
  RLX_REQUIRE(desc->fwd_path != 2 || fits, RLX_EUNSUP, "rlx_bro_net_f32: fwd_path 2: the fused layer's row tile does not fit the device's LDS");
  if (desc->fwd_path == 2 || (desc->fwd_path == 0 && !bwd && fits && M <= BRO_FUSED_MAX_M)) {
    BroFusedBufs F;
    const int rcf = arena_carve(ctx, SL_BRO, [&](Arena& a) { bro_carve_fused(E, M, a, &F); });
    return rcf ? rcf : bro_fwd_fused(ctx, E, params, x, M, F, out, st);
  }
  BxReleaseAll release{ctx};
  int rcx = bro_images(ctx, E, params, bwd, M, st);
  if (rcx) return rcx;
  BroBufs B;
  rcx = arena_carve(ctx, SL_BRO, [&](Arena& a) { bro_carve(E, M, bwd, dx != nullptr, out, a, &B); });
  if (rcx) return rcx;
  rcx = bro_fwd(ctx, E, params, x, M, B, out, st);
  if (rcx || !bwd) return rcx;
  return bro_bwd(ctx, E, params, M, B, d_out, grads, dx, st);
}

int rlx_bro_quantile_loss_f32(rlx_ctx* ctx, const float* q1, const float* q2, const float* next_q1, const float* next_q2, const float* rewards,
                              const float* terminations, const float* next_logp, const float* log_alpha, int64_t B, int N, float gamma,
                              float pessimism, float kappa, float* dq1, float* dq2, float* loss_out, float* y_out, void* stream) {
  RLX_REQUIRE(ctx && q1 && q2 && next_q1 && next_q2 && rewards && terminations && next_logp && log_alpha && dq1 && dq2 && loss_out, RLX_EINVAL,
              "rlx_bro_quantile_loss_f32: NULL pointer (only y_out may be NULL)");
  RLX_REQUIRE(N >= 1 && N <= QL_MAXN, RLX_EUNSUP, "rlx_bro_quantile_loss_f32: N must be 1..128 quantiles");
  RLX_REQUIRE(kappa > 0.f && std::isfinite(kappa), RLX_EUNSUP, "rlx_bro_quantile_loss_f32: kappa must be positive");
  RLX_REQUIRE(B >= 1 && B <= (1 << 24), RLX_EUNSUP, "rlx_bro_quantile_loss_f32: B must be 1..2^24 rows");
  hipStream_t st = (hipStream_t)stream;
  int grid = div_up(B, 4);
  if (grid > 1024) grid = 1024;
  QlossArgs a{q1, q2, next_q1, next_q2, rewards, terminations, next_logp, log_alpha, dq1, dq2, nullptr, y_out, B, N, gamma, pessimism, kappa};
  a.part = (float*)scratch(ctx, SL_BRO, (size_t)grid * sizeof(float));
  if (!a.part) return RLX_ENOMEM;
  hipLaunchKernelGGL(k_bro_qloss, dim3(grid), dim3(256), 0, st, a);
  RLX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bro_qloss_fold, dim3(1), dim3(64), 0, st, (const float*)a.part, grid, (float)((double)B * N), loss_out);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

}  // extern "C"
