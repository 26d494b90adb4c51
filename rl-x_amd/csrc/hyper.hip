// hyper.hip -- the row and column operations of the reference's hyperspherical networks (rl_x/algorithms/simbav2/flax/layers.py:8-93,
// :131-143; simbav2.py:178, :233): l2-normalisation of activation rows behind a learned per-column Scaler, the LERP residual with its
// two normalisations, the scaled ReLU, each forward and backward, and the projection of weight matrices back to unit column norm; and
// the entry points rlx_hyper_net_f32 (the network, hyper_net.h), rlx_hyper_project_f32 and rlx_colnorm_f32.  float32 throughout, true
// sqrtf and division, every sum in a fixed order, no atomics: identical calls give identical bits.  No product lives here -- the three
// GEMMs of a layer are the existing launchers' -- so the kernels are about reading each element once.
//
// Row kernels: one wave per row, four rows per workgroup, rows grid-strided.  A row of H <= 1024 floats is H / 4 16-byte chunks; lane l
// holds the chunks l, l + 64, ... (NQ = ceil(H / 256) <= 4 of them) in registers from its one load to its one store, so a workgroup's
// loads are whole 1 KB runs.  A norm is a wave butterfly sum.  The forward kernels use no LDS and no barrier.  The lerp stores the two
// reciprocal clamped norms of a row; a reciprocal of exactly 1 / EPS marks a clamped norm, whose gradient is d / EPS (a constant norm).
// Backward: a wave recomputes its row from the kept pre-norm values, writes the input gradients over operands that are dead after it
// (d z over z, the residual branch's gradient over the arriving gradient), and keeps the Scaler / alpha gradient of its columns --
// a sum over the rows it walks -- in registers.  After the walk the waves of a workgroup fold through LDS in wave order, one partial
// row per workgroup goes to [grid, width], and the fixed-order slab reduction (stage_reduce) finishes the column sums.
// The scaled ReLU's backward is the same kernel shape over an H-wide column slab of [M, X] (grid.y = X / H).
//
// Projection: a workgroup owns a strip of 256 adjacent columns of one matrix (64 lanes x one 16-byte chunk: a row of the strip is one
// coalesced 1 KB run), its 16 waves split the K rows (wave w: rows w, w + 16, ...).  A lane sums the squares of its own four columns
// in row order, the waves fold through LDS in wave order, every thread forms the clamped norms of its columns, and the strip is read a
// second time and written divided: two reads at most, one write.  Matrices whose N is no multiple of 4 (or that are not 16-byte
// aligned) take the same walk with one column per lane (64-column strips).  One launch covers every matrix of a small table.
#include "hyper_net.h"

namespace rlx {

constexpr float HYPER_RMAX = 1.0f / HYPER_EPS;      // the reciprocal of a clamped norm
constexpr int COLN_WAVES = 16;

__device__ __forceinline__ float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ __forceinline__ float4 operator+(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 operator-(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 operator*(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 operator*(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
// chunk j of a row of nch chunks (zeros beyond the row: they add nothing to a sum)
__device__ __forceinline__ float4 ld_chunk(const float* row, int j, int nch) {
  return j < nch ? reinterpret_cast<const float4*>(row)[j] : f4(0.f);
}
__device__ __forceinline__ void st_chunk(float* row, int j, int nch, float4 v) {
  if (j < nch) reinterpret_cast<float4*>(row)[j] = v;
}
__device__ __forceinline__ float rnorm(float ss) {      // 1 / max(sqrt(ss), EPS)
  const float n = sqrtf(ss);
  return n > HYPER_EPS ? 1.0f / n : HYPER_RMAX;
}

// the column sums a wave kept over its rows -> one partial row of the workgroup: waves 1..3 hand theirs over, wave 0 adds in wave order
template <int NQ>
__device__ __forceinline__ void fold_partials(const float4 (&acc)[NQ], float* part_row, int nch) {
  __shared__ float4 fold[3 * NQ * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (wv) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) fold[((wv - 1) * NQ + q) * 64 + lane] = acc[q];
  }
  __syncthreads();
  if (wv == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float4 t = acc[q];
#pragma unroll
      for (int w = 0; w < 3; ++w) t = t + fold[(w * NQ + q) * 64 + lane];
      st_chunk(part_row, lane + 64 * q, nch, t);
    }
  }
}

struct RowArgs {
  float* z;            // scale-norm: z, lerp: z2, relu: d h (backward: overwritten by the input gradient)
  const float* x;      // lerp: the block's input; relu: z1
  const float* s;      // the Scaler / alpha vector
  float* out;          // forward: the normalised rows
  float* rn;           // lerp: [M, 2] reciprocal clamped norms
  const float *d, *d2; // backward: the arriving gradient d (+ d2)
  float* dres;         // lerp backward: the residual branch's gradient
  float* part;         // backward: [grid, width] partial column sums
  float c;
  int H, ld;           // ld: row stride (relu: X)
  int64_t M;
};

// e = l2n(s * (c z));  backward: d z = (d - e (e . d)) / n * s c over z,  d s = c sum_rows (d - e (e . d)) / n * z  (c: the reduction's)
template <int NQ, bool BWD>
__global__ __launch_bounds__(256) void k_hyper_scale_norm(const RowArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nch = a.H >> 2;
  float4 sc[NQ], acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    sc[q] = ld_chunk(a.s, lane + 64 * q, nch);
    acc[q] = f4(0.f);
  }
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < a.M; row += (int64_t)gridDim.x * 4) {
    float* zr = a.z + row * a.H;
    float4 z[NQ], u[NQ], g[NQ];
    float ss = 0.f, dot = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      z[q] = ld_chunk(zr, lane + 64 * q, nch);
      if (BWD) {
        g[q] = ld_chunk(a.d + row * a.H, lane + 64 * q, nch);
        if (a.d2) g[q] = g[q] + ld_chunk(a.d2 + row * a.H, lane + 64 * q, nch);
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      u[q] = sc[q] * (z[q] * a.c);
      ss += dot4(u[q], u[q]);
      if (BWD) dot += dot4(u[q], g[q]);
    }
    const float r = rnorm(wave_sum(ss));
    if (!BWD) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) st_chunk(a.out + row * a.H, lane + 64 * q, nch, u[q] * r);
    } else {
      const float k = r < HYPER_RMAX ? wave_sum(dot) * r * r : 0.f;      // e (e . d) = u k
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float4 du = (g[q] - u[q] * k) * r;
        acc[q] = acc[q] + du * z[q];
        st_chunk(zr, lane + 64 * q, nch, (du * sc[q]) * a.c);
      }
    }
  }
  if constexpr (BWD) fold_partials<NQ>(acc, a.part + (int64_t)blockIdx.x * a.H, nch);
}

// y = l2n(z2), v = x + a * (ca (y - x)), x' = l2n(v).  Backward from d x' = d (+ d2):
//   d v = (d x' - x' (x' . d x')) / n_v,  d a = ca sum_rows d v * (y - x),  d y = a * (ca d v),  d z2 = (d y - y (y . d y)) / n_z over z2,
//   the residual branch receives d v - d y = d v * (1 - a ca)
template <int NQ, bool BWD>
__global__ __launch_bounds__(256) void k_hyper_lerp(const RowArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nch = a.H >> 2;
  float4 al[NQ], acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    al[q] = ld_chunk(a.s, lane + 64 * q, nch);
    acc[q] = f4(0.f);
  }
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < a.M; row += (int64_t)gridDim.x * 4) {
    float* zr = a.z + row * a.H;
    float4 y[NQ], x[NQ], g[NQ];
    float r1, r2;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      y[q] = ld_chunk(zr, lane + 64 * q, nch);
      x[q] = ld_chunk(a.x + row * a.H, lane + 64 * q, nch);
      if (BWD) {
        g[q] = ld_chunk(a.d + row * a.H, lane + 64 * q, nch);
        if (a.d2) g[q] = g[q] + ld_chunk(a.d2 + row * a.H, lane + 64 * q, nch);
      }
    }
    if (BWD) {
      r1 = a.rn[2 * row];
      r2 = a.rn[2 * row + 1];
    } else {
      float ss = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) ss += dot4(y[q], y[q]);
      r1 = rnorm(wave_sum(ss));
    }
    float4 df[NQ], v[NQ];
    float ss2 = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      y[q] = y[q] * r1;
      df[q] = y[q] - x[q];
      v[q] = x[q] + al[q] * (df[q] * a.c);
      ss2 += dot4(v[q], v[q]);
    }
    if (!BWD) {
      r2 = rnorm(wave_sum(ss2));
#pragma unroll
      for (int q = 0; q < NQ; ++q) st_chunk(a.out + row * a.H, lane + 64 * q, nch, v[q] * r2);
      if (lane == 0) {
        a.rn[2 * row] = r1;
        a.rn[2 * row + 1] = r2;
      }
    } else {
      float dot = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) dot += dot4(v[q], g[q]);
      const float k2 = r2 < HYPER_RMAX ? wave_sum(dot) * r2 * r2 : 0.f;      // x' (x' . d x') = v k2
      float4 dy[NQ];
      dot = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float4 dv = (g[q] - v[q] * k2) * r2;
        acc[q] = acc[q] + dv * df[q];
        dy[q] = al[q] * (dv * a.c);
        dot += dot4(y[q], dy[q]);
        st_chunk(a.dres + row * a.H, lane + 64 * q, nch, dv - dy[q]);
      }
      const float k1 = r1 < HYPER_RMAX ? wave_sum(dot) : 0.f;      // (y is normalised already)
#pragma unroll
      for (int q = 0; q < NQ; ++q) st_chunk(zr, lane + 64 * q, nch, (dy[q] - y[q] * k1) * r1);
    }
  }
  if constexpr (BWD) fold_partials<NQ>(acc, a.part + (int64_t)blockIdx.x * a.H, nch);
}

// h = relu(s1 * (c z1)) + EPS: a grid-stride float4 element kernel over [M, X]
__global__ __launch_bounds__(256) void k_hyper_relu(const float* __restrict__ z1, const float* __restrict__ s1, float c,
                                                    float* __restrict__ h, int64_t n4, int x4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 z = reinterpret_cast<const float4*>(z1)[i], s = reinterpret_cast<const float4*>(s1)[i % x4];
    const float4 u = s * (z * c);
    reinterpret_cast<float4*>(h)[i] =
        make_float4(fmaxf(u.x, 0.f) + HYPER_EPS, fmaxf(u.y, 0.f) + HYPER_EPS, fmaxf(u.z, 0.f) + HYPER_EPS, fmaxf(u.w, 0.f) + HYPER_EPS);
  }
}

// d z1 = d h * [s1 c z1 > 0] * s1 c over d h,  d s1 = c sum_rows d h * [. > 0] * z1; blockIdx.y: the H-wide column slab of [M, X]
template <int NQ>
__global__ __launch_bounds__(256) void k_hyper_relu_bwd(const RowArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nch = a.H >> 2, col0 = blockIdx.y * a.H;
  float4 sc[NQ], acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    sc[q] = ld_chunk(a.s + col0, lane + 64 * q, nch);
    acc[q] = f4(0.f);
  }
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < a.M; row += (int64_t)gridDim.x * 4) {
    float* hr = a.z + row * a.ld + col0;
    float4 z[NQ], g[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      z[q] = ld_chunk(a.x + row * a.ld + col0, lane + 64 * q, nch);
      g[q] = ld_chunk(hr, lane + 64 * q, nch);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float4 u = sc[q] * (z[q] * a.c);
      const float4 t = make_float4(u.x > 0.f ? g[q].x : 0.f, u.y > 0.f ? g[q].y : 0.f, u.z > 0.f ? g[q].z : 0.f, u.w > 0.f ? g[q].w : 0.f);
      acc[q] = acc[q] + t * z[q];
      st_chunk(hr, lane + 64 * q, nch, (t * sc[q]) * a.c);
    }
  }
  fold_partials<NQ>(acc, a.part + (int64_t)blockIdx.x * a.ld + col0, nch);
}

// xt = l2n([x, shift]) with zero padding up to ld (<= 1028: at most 17 elements per lane); x has row stride `in`, no alignment
constexpr int EMB_Q = 17;
__global__ __launch_bounds__(256) void k_hyper_embed_in(const float* __restrict__ x, int in, float shift, int64_t M,
                                                        float* __restrict__ xt, int ld, float* __restrict__ rn) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < M; row += (int64_t)gridDim.x * 4) {
    float v[EMB_Q];
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < EMB_Q; ++q) {
      const int j = lane + 64 * q;
      v[q] = j < in ? x[row * in + j] : (j == in ? shift : 0.f);
      ss += v[q] * v[q];
    }
    const float r = rnorm(wave_sum(ss));
#pragma unroll
    for (int q = 0; q < EMB_Q; ++q) {
      const int j = lane + 64 * q;
      if (j < ld) xt[row * ld + j] = v[q] * r;
    }
    if (lane == 0) rn[row] = r;
  }
}
// dx = (d xt - xt (xt . d xt)) / n over the first `in` columns; the columns of d xt beyond `in` were never written and are not read
__global__ __launch_bounds__(256) void k_hyper_embed_in_bwd(const float* __restrict__ dxt, const float* __restrict__ xt,
                                                            const float* __restrict__ rn, int in, int ld, int64_t M,
                                                            float* __restrict__ dx) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < M; row += (int64_t)gridDim.x * 4) {
    float e[EMB_Q], g[EMB_Q];
    float dot = 0.f;
#pragma unroll
    for (int q = 0; q < EMB_Q; ++q) {
      const int j = lane + 64 * q;
      e[q] = j <= in ? xt[row * ld + j] : 0.f;
      g[q] = j <= in ? dxt[row * ld + j] : 0.f;
      dot += e[q] * g[q];
    }
    const float r = rn[row];
    const float k = r < HYPER_RMAX ? wave_sum(dot) : 0.f;
#pragma unroll
    for (int q = 0; q < EMB_Q; ++q) {
      const int j = lane + 64 * q;
      if (j < in) dx[row * in + j] = (g[q] - e[q] * k) * r;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ projection
struct ColJob { float* W; int64_t stride; int K, N, blk0, strips, vec; };      // blk0: the job's first workgroup
struct ColTable { int n; ColJob job[HYPER_MAX_MATS]; };

template <typename T>
__device__ __forceinline__ void colnorm_strip(float* W, int K, int N, int c, bool on, T* fold) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T ss{};
  if (on) {
#pragma unroll 4
    for (int k = wv; k < K; k += COLN_WAVES) {
      const T w = *reinterpret_cast<const T*>(W + (int64_t)k * N + c);
      ss = ss + w * w;
    }
  }
  fold[wv * 64 + lane] = ss;
  __syncthreads();
  T tot = fold[lane];
#pragma unroll
  for (int w = 1; w < COLN_WAVES; ++w) tot = tot + fold[w * 64 + lane];
  if (!on) return;
  T nrm;
  if constexpr (sizeof(T) == 16) nrm = make_float4(fmaxf(sqrtf(tot.x), HYPER_EPS), fmaxf(sqrtf(tot.y), HYPER_EPS), fmaxf(sqrtf(tot.z), HYPER_EPS), fmaxf(sqrtf(tot.w), HYPER_EPS));
  else nrm = fmaxf(sqrtf(tot), HYPER_EPS);
#pragma unroll 4
  for (int k = wv; k < K; k += COLN_WAVES) {
    T* p = reinterpret_cast<T*>(W + (int64_t)k * N + c);
    const T w = *p;
    if constexpr (sizeof(T) == 16) *p = make_float4(w.x / nrm.x, w.y / nrm.y, w.z / nrm.z, w.w / nrm.w);
    else *p = w / nrm;
  }
}

__global__ __launch_bounds__(64 * COLN_WAVES) void k_hyper_colnorm(const ColTable t) {
  __shared__ float4 fold[COLN_WAVES * 64];
  int i = 0;
  while (i + 1 < t.n && (int)blockIdx.x >= t.job[i + 1].blk0) ++i;
  const ColJob j = t.job[i];
  const int lb = blockIdx.x - j.blk0, lane = threadIdx.x & 63;
  float* W = j.W + (int64_t)(lb / j.strips) * j.stride;
  const int s = lb % j.strips;
  if (j.vec) {
    const int c = s * 256 + lane * 4;      // N % 4 == 0: a chunk lies inside the row or beyond it
    colnorm_strip<float4>(W, j.K, j.N, c, c < j.N, fold);
  } else {
    const int c = s * 64 + lane;
    colnorm_strip<float>(W, j.K, j.N, c, c < j.N, reinterpret_cast<float*>(fold));
  }
}

// ------------------------------------------------------------------------------------------------------------ launchers
#define HYPER_ROW_LAUNCH(KERNEL, BWDARGS, H, GRID, ST, ARGS)                                   \
  switch (div_up((H) / 4, 64)) {                                                               \
    case 1: hipLaunchKernelGGL((KERNEL<1 BWDARGS>), GRID, dim3(256), 0, ST, ARGS); break;      \
    case 2: hipLaunchKernelGGL((KERNEL<2 BWDARGS>), GRID, dim3(256), 0, ST, ARGS); break;      \
    case 3: hipLaunchKernelGGL((KERNEL<3 BWDARGS>), GRID, dim3(256), 0, ST, ARGS); break;      \
    default: hipLaunchKernelGGL((KERNEL<4 BWDARGS>), GRID, dim3(256), 0, ST, ARGS); break;     \
  }                                                                                            \
  RLX_LAUNCH_CHECK()
#define HYPER_COMMA_FALSE , false
#define HYPER_COMMA_TRUE , true

// the partial rows of a backward row kernel -> dst [width], scaled
static int hyper_finish(rlx_ctx* ctx, const float* part, int grid, int width, float scale, float* dst, hipStream_t st) {
  ReduceTable tab;
  tab.n = 0;
  tab.seg[tab.n++] = ReduceSeg{part, dst, (int64_t)width, (int64_t)width, grid, 0, scale, 0.f, 1};
  return stage_reduce(ctx, tab, nullptr, nullptr, st);
}

int hyper_embed_in(const rlx_ctx* ctx, const float* x, int in, float shift, int64_t M, float* xt, int ld, float* rn, hipStream_t st) {
  hipLaunchKernelGGL(k_hyper_embed_in, dim3(rows_grid(ctx, M)), dim3(256), 0, st, x, in, shift, M, xt, ld, rn);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
int hyper_embed_in_bwd(const rlx_ctx* ctx, const float* dxt, const float* xt, const float* rn, int in, int ld, int64_t M, float* dx,
                       hipStream_t st) {
  hipLaunchKernelGGL(k_hyper_embed_in_bwd, dim3(rows_grid(ctx, M)), dim3(256), 0, st, dxt, xt, rn, in, ld, M, dx);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
int hyper_scale_norm(const rlx_ctx* ctx, const float* z, const float* s, float c, int64_t M, int H, float* e, hipStream_t st) {
  RowArgs a{};
  a.z = const_cast<float*>(z); a.s = s; a.out = e; a.c = c; a.H = H; a.ld = H; a.M = M;
  HYPER_ROW_LAUNCH(k_hyper_scale_norm, HYPER_COMMA_FALSE, H, dim3(rows_grid(ctx, M)), st, a);
  return RLX_OK;
}
int hyper_scale_norm_bwd(rlx_ctx* ctx, float* z_dz, const float* s, float c, const float* d, const float* d2, int64_t M, int H, float* g_s,
                         hipStream_t st) {
  const int grid = bwd_rows_grid(ctx, M);
  RowArgs a{};
  a.z = z_dz; a.s = s; a.d = d; a.d2 = d2; a.c = c; a.H = H; a.ld = H; a.M = M;
  a.part = stage_alloc(ctx, (size_t)grid * H);
  if (!a.part) return RLX_ENOMEM;
  HYPER_ROW_LAUNCH(k_hyper_scale_norm, HYPER_COMMA_TRUE, H, dim3(grid), st, a);
  return hyper_finish(ctx, a.part, grid, H, c, g_s, st);
}
int hyper_relu(const float* z1, const float* s1, float c, int64_t M, int X, float* h, hipStream_t st) {
  const int64_t n4 = M * (X / 4);
  hipLaunchKernelGGL(k_hyper_relu, dim3(elem_grid(n4)), dim3(256), 0, st, z1, s1, c, h, n4, X / 4);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
int hyper_relu_bwd(rlx_ctx* ctx, const float* z1, const float* s1, float c, float* dh_dz1, int64_t M, int H, int X, float* g_s1, hipStream_t st) {
  int grid = bwd_rows_grid(ctx, M);
  if (grid > 256) grid = 256;      // X / H slabs share the chip, and the reduction adds `grid` partial rows per column
  RowArgs a{};
  a.z = dh_dz1; a.x = z1; a.s = s1; a.c = c; a.H = H; a.ld = X; a.M = M;
  a.part = stage_alloc(ctx, (size_t)grid * X);
  if (!a.part) return RLX_ENOMEM;
  HYPER_ROW_LAUNCH(k_hyper_relu_bwd, , H, dim3(grid, X / H), st, a);
  return hyper_finish(ctx, a.part, grid, X, c, g_s1, st);
}
int hyper_lerp(const rlx_ctx* ctx, const float* z2, const float* x, const float* al, float ca, int64_t M, int H, float* out, float* rn,
               hipStream_t st) {
  RowArgs a{};
  a.z = const_cast<float*>(z2); a.x = x; a.s = al; a.out = out; a.rn = rn; a.c = ca; a.H = H; a.ld = H; a.M = M;
  HYPER_ROW_LAUNCH(k_hyper_lerp, HYPER_COMMA_FALSE, H, dim3(rows_grid(ctx, M)), st, a);
  return RLX_OK;
}
int hyper_lerp_bwd(rlx_ctx* ctx, float* z2_dz2, const float* x, const float* al, float ca, const float* rn, const float* d, const float* d2,
                   int64_t M, int H, float* dres, float* g_a, hipStream_t st) {
  const int grid = bwd_rows_grid(ctx, M);
  RowArgs a{};
  a.z = z2_dz2; a.x = x; a.s = al; a.rn = const_cast<float*>(rn); a.d = d; a.d2 = d2; a.dres = dres; a.c = ca; a.H = H; a.ld = H; a.M = M;
  a.part = stage_alloc(ctx, (size_t)grid * H);
  if (!a.part) return RLX_ENOMEM;
  HYPER_ROW_LAUNCH(k_hyper_lerp, HYPER_COMMA_TRUE, H, dim3(grid), st, a);
  return hyper_finish(ctx, a.part, grid, H, ca, g_a, st);
}

int hyper_colnorm(const ColMat* mats, int n, hipStream_t st) {
  ColTable t;
  int64_t blocks = 0;
  RLX_REQUIRE(n >= 1 && n <= HYPER_MAX_MATS, RLX_EUNSUP, "hyper_colnorm: 1..9 matrices per launch");
  for (int i = 0; i < n; ++i) {
    const ColMat& m = mats[i];
    ColJob& j = t.job[i];
    j.W = m.W; j.stride = m.stride; j.K = m.K; j.N = m.N; j.blk0 = (int)blocks;
    j.vec = (m.N % 4 == 0 && m.stride % 4 == 0 && (reinterpret_cast<uintptr_t>(m.W) & 15) == 0) ? 1 : 0;
    j.strips = div_up(m.N, j.vec ? 256 : 64);
    blocks += (int64_t)m.E * j.strips;
    RLX_REQUIRE(blocks <= 0x7fffffffLL, RLX_EUNSUP, "hyper_colnorm: E * ceil(N / 64) must fit the grid");
  }
  t.n = n;
  hipLaunchKernelGGL(k_hyper_colnorm, dim3((unsigned)blocks), dim3(64 * COLN_WAVES), 0, st, t);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

static bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t m = 0;
  for (const void* p : ps) m |= (uintptr_t)p;
  return (m & 15) == 0;
}

// the envelope of the descriptor (RLX_EUNSUP, naming the field)
static int hyper_check(const char* who, const rlx_hyper_desc& t) {
  const std::string w(who);
  RLX_REQUIRE(t.hidden >= 64 && t.hidden % 64 == 0 && t.hidden <= 1024, RLX_EUNSUP,
              w + ": hidden must be a multiple of 64 up to 1024 (the row kernels hold a row in one wave)");
  RLX_REQUIRE(t.expansion >= 1 && (int64_t)t.expansion * t.hidden <= 4096, RLX_EUNSUP, w + ": expansion must be at least 1 with expansion * hidden <= 4096");
  RLX_REQUIRE(t.n_blocks >= 1 && t.n_blocks <= HYPER_MAX_BLOCKS, RLX_EUNSUP, w + ": n_blocks must be 1..4");
  RLX_REQUIRE(t.in_dim >= 1 && t.in_dim <= 1024, RLX_EUNSUP, w + ": in_dim must be 1..1024");
  RLX_REQUIRE(t.scaler_scale != 0.f && std::isfinite(t.scaler_init / t.scaler_scale), RLX_EUNSUP, w + ": scaler_scale must be non-zero");
  RLX_REQUIRE(t.alpha_scale != 0.f && std::isfinite(t.alpha_init / t.alpha_scale), RLX_EUNSUP, w + ": alpha_scale must be non-zero");
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int64_t rlx_hyper_param_count(const rlx_hyper_desc* desc) {
  if (!desc || desc->in_dim < 1 || desc->hidden < 1 || desc->expansion < 1 || desc->n_blocks < 1 || desc->n_blocks > HYPER_MAX_BLOCKS) return -1;
  return make_hyper(*desc).n_params;
}

int rlx_hyper_net_f32(rlx_ctx* ctx, const rlx_hyper_desc* desc, const float* params, const float* x, int64_t M, float* out,
                      const float* d_out, float* grads, float* dx, void* stream) {
  RLX_REQUIRE(ctx && desc && params && x && out, RLX_EINVAL, "rlx_hyper_net_f32: NULL pointer (ctx, desc, params, x, out)");
  RLX_REQUIRE(!d_out || grads, RLX_EINVAL, "rlx_hyper_net_f32: a backward (d_out) needs grads");
  const int rc = hyper_check("rlx_hyper_net_f32", *desc);
  if (rc) return rc;
  RLX_REQUIRE(M >= 1 && M <= (1 << 20), RLX_EUNSUP, "rlx_hyper_net_f32: M must be 1..2^20 rows");
  RLX_REQUIRE(aligned16({params, out, d_out, grads}), RLX_EINVAL, "rlx_hyper_net_f32: params, out, d_out and grads must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const Hyper E = make_hyper(*desc);
  const bool bwd = d_out != nullptr;
  BxReleaseAll release{ctx};
  int rcx = hyper_images(ctx, E, params, bwd, M, st);
  if (rcx) return rcx;
  HyperBufs B;
  rcx = arena_carve(ctx, SL_HYPER, [&](Arena& a) { hyper_carve(E, M, bwd, dx != nullptr, a, &B); });
  if (rcx) return rcx;
  rcx = hyper_fwd(ctx, E, params, x, M, B, out, st);
  if (rcx || !bwd) return rcx;
  return hyper_bwd(ctx, E, params, M, B, d_out, grads, dx, st);
}

int rlx_hyper_project_f32(rlx_ctx* ctx, const rlx_hyper_desc* desc, float* params, void* stream) {
  RLX_REQUIRE(ctx && desc && params, RLX_EINVAL, "rlx_hyper_project_f32: NULL pointer (ctx, desc, params)");
  const int rc = hyper_check("rlx_hyper_project_f32", *desc);
  if (rc) return rc;
  const Hyper E = make_hyper(*desc);
  ColMat mats[HYPER_MAX_MATS];
  int n = 0;
  mats[n++] = ColMat{params + E.We, 0, E.in + 1, E.H, 1};
  for (int b = 0; b < E.n_blocks; ++b) {
    mats[n++] = ColMat{params + E.blk[b].W1, 0, E.H, E.X, 1};
    mats[n++] = ColMat{params + E.blk[b].W2, 0, E.X, E.H, 1};
  }
  return hyper_colnorm(mats, n, (hipStream_t)stream);
}

int rlx_colnorm_f32(rlx_ctx* ctx, float* W, int64_t K, int64_t N, int E, int64_t stride, void* stream) {
  RLX_REQUIRE(ctx && W, RLX_EINVAL, "rlx_colnorm_f32: NULL pointer (ctx, W)");
  RLX_REQUIRE(K >= 1 && K <= (1 << 20), RLX_EUNSUP, "rlx_colnorm_f32: K must be 1..2^20");
  RLX_REQUIRE(N >= 1 && N <= (1 << 20), RLX_EUNSUP, "rlx_colnorm_f32: N must be 1..2^20");
  RLX_REQUIRE(E >= 1, RLX_EUNSUP, "rlx_colnorm_f32: E must be at least 1");
  RLX_REQUIRE(E == 1 || stride >= K * N, RLX_EUNSUP, "rlx_colnorm_f32: stride must be at least K * N");
  const ColMat m{W, stride, (int)K, (int)N, E};
  return hyper_colnorm(&m, 1, (hipStream_t)stream);
}

}  // extern "C"
