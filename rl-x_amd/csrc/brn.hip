// brn.hip -- batch renormalisation (rl_x/algorithms/crossq/flax/batch_renorm.py:77-130): the tree's one COLUMN-statistics layer.  Every
// other norm here is a row norm with a wave per row (k_rms_act, k_mpo_ln_tanh, k_drop_ln_relu); this one reduces over the M rows of
// x [M, D] (row stride ld, a multiple of four), so a lane owns a column and a wave reads 64 consecutive floats of a row.  net_pass.h
// declares the launchers.  Over scale g, bias b and the running ra_mean / ra_var (eps, r_max, d_max, momentum m: BrnCfg):
//   eval    y = (x - ra_mean) rsqrt(ra_var + eps) g + b                                                          (:87-93)
//   train   mu = mean_i x, v = max(0, mean_i x^2 - mu^2);  r = clip(sqrt(v + eps) / sqrt(ra_var + eps), 1 / r_max, r_max),
//           d = clip((mu - ra_mean) / sqrt(ra_var + eps), -d_max, d_max), both constants of the backward;  w = warmed;
//           cm = mu - w d sqrt(v) / r,  s = w / r^2 + (1 - w),  rho = rsqrt(v s + eps),  y = (x - cm) rho g + b;
//           then ra_mean <- m ra_mean + (1 - m) mu, ra_var <- m ra_var + (1 - m) v, in place                      (:95-128)
//   train backward, with sdy = sum_i dY_i and sdyx = sum_i dY_i x_i:  S1 = g sdy,  S2 = g (sdyx - cm sdy),  dcm = -rho S1,
//           dcv = -rho^3 S2 / 2,  dv = dcv s - dcm t with t = w (d / r) / (2 sqrt(v)),
//           dX_i = dY_i g rho + dcm / M + dv 2 (x_i - mu) / M,  dg = rho (sdyx - cm sdy),  db = sdy
//   eval backward: the per-column affine map, dX_i = dY_i g rho with rho = rsqrt(ra_var + eps), cm = ra_mean in dg.
// ZERO-VARIANCE RULE (a deviation): where v == 0 the reference's sqrt has an infinite derivative; here t = 0 where w = 0 or
// v = 0 -- the sqrt(v) term of cm then has no gradient -- and every result stays finite.
// Three launches per training pass and per backward, E networks (grid.z / grid.y) in each:
//   k_brn_colsum   lane <-> column, the four waves of a workgroup stride over the rows of a slab of BRN_SLAB_ROWS rows (more when
//                  M exceeds what 4 num_cus slabs hold); DOUBLE accumulators -- a column of mean 50 and std 0.5 loses its variance
//                  in float -- added across the waves through LDS in wave order, written as per-slab partials: no atomics
//   k_brn_finish_* one thread per (network, column): adds the slabs in slab order, does the column's arithmetic in double, writes
//                  the coefficients of the element-wise pass (rows padded to four columns, the padding zero) and, forward, what
//                  the backward needs -- save [7][Dp] = mu, cm (each as a float pair hi, lo: a column of mean 50 and std 0.5 keeps x - cm to
//                  float precision of the DIFFERENCE), rho, s, t -- and advances the running statistics
//   k_brn_apply_*  element-wise over float4 groups of a row, grid-stride; padding columns (c >= D) are written 0; the backward
//                  multiplies dX by 1[x > 0] when x is a ReLU's output, so the GEMM below needs no epilogue
// Fixed order everywhere: two identical calls give identical bits, and a launch over E networks equals E single launches.
#include "net_pass.h"

namespace rlx {

constexpr int BRN_SLAB_ROWS = 64;
constexpr int BRN_COEF_ROWS = 5;

// v as a float pair: hi + lo == v to 2^-48 relative
__device__ __forceinline__ void brn_split(double v, float& hi, float& lo) {
  hi = (float)v;
  lo = (float)(v - (double)hi);
}

static inline int brn_rows_per_slab(const rlx_ctx* ctx, int64_t M) {
  const int64_t cap = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 1) * 4;
  int64_t rows = BRN_SLAB_ROWS;
  if (div_up(M, rows) > cap) rows = (M + cap - 1) / cap;
  return (int)rows;
}
int brn_slabs(const rlx_ctx* ctx, int64_t M) { return div_up(M, brn_rows_per_slab(ctx, M)); }
// [E][S][2][D] doubles of slab partials, then [E][BRN_COEF_ROWS][Dp] floats of coefficients
size_t brn_work_floats(const rlx_ctx* ctx, int64_t M, int D, int E) {
  return a64(2 * (size_t)E * brn_slabs(ctx, M) * 2 * D) + a64((size_t)E * BRN_COEF_ROWS * brn_dp(D));
}

// part[((e S + slab) 2 + k) D + c]: k = 0 sum x (BWD: sum dY), k = 1 sum x^2 (BWD: sum dY x) over the slab's rows
template <bool BWD>
__global__ __launch_bounds__(256) void k_brn_colsum(const float* __restrict__ x, const float* __restrict__ dY, int ld, int64_t M, int D,
                                                    int rows_per_slab, int64_t e_x, int64_t e_y, double* __restrict__ part) {
  __shared__ double s_acc[4][2][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int slab = blockIdx.y, S = gridDim.y, e = blockIdx.z;
  const int64_t r0 = (int64_t)slab * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < M ? r0 + rows_per_slab : M;
  const float* xe = x + (int64_t)e * e_x;
  const float* de = BWD ? dY + (int64_t)e * e_y : nullptr;
  double a0 = 0.0, a1 = 0.0;
  if (c < D) {
    for (int64_t r = r0 + w; r < r1; r += 4) {
      const float xv = xe[r * ld + c];
      if (BWD) {
        const float gv = de[r * ld + c];
        a0 += (double)gv;
        a1 += (double)gv * (double)xv;
      } else {
        a0 += (double)xv;
        a1 += (double)xv * (double)xv;
      }
    }
  }
  s_acc[w][0][lane] = a0;
  s_acc[w][1][lane] = a1;
  __syncthreads();
  if (w == 0 && c < D) {
    double t0 = s_acc[0][0][lane], t1 = s_acc[0][1][lane];
    for (int k = 1; k < 4; ++k) {
      t0 += s_acc[k][0][lane];
      t1 += s_acc[k][1][lane];
    }
    double* out = part + ((int64_t)e * S + slab) * 2 * D;
    out[c] = t0;
    out[D + c] = t1;
  }
}

__device__ __forceinline__ void brn_slab_sums(const double* __restrict__ part, int e, int S, int D, int c, double& s0, double& s1) {
  s0 = 0.0;
  s1 = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* p = part + ((int64_t)e * S + s) * 2 * D;
    s0 += p[c];
    s1 += p[D + c];
  }
}

// coef [E][5][Dp] = cm hi, cm lo, rho g, b (the fifth row is the backward's); save [E][7][Dp] = mu hi, mu lo, cm hi, cm lo, rho, s, t;
// columns D .. Dp - 1 are 0
__global__ __launch_bounds__(256) void k_brn_finish_fwd(const double* __restrict__ part, int S, int64_t M, int D, int Dp,
                                                        const float* __restrict__ g, const float* __restrict__ b, int64_t e_p,
                                                        float* __restrict__ ra_mean, float* __restrict__ ra_var, int64_t e_s, BrnCfg cfg,
                                                        int warmed, float* __restrict__ coef, float* __restrict__ save) {
  const int c = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
  if (c >= Dp) return;
  float* co = coef + (int64_t)e * BRN_COEF_ROWS * Dp;
  float* sv = save + (int64_t)e * BRN_SAVE_ROWS * Dp;
  if (c >= D) {
    for (int k = 0; k < 4; ++k) co[k * Dp + c] = 0.f;
    for (int k = 0; k < BRN_SAVE_ROWS; ++k) sv[k * Dp + c] = 0.f;
    return;
  }
  double s0, s1;
  brn_slab_sums(part, e, S, D, c, s0, s1);
  const double mu = s0 / (double)M;
  double v = s1 / (double)M - mu * mu;
  v = v > 0.0 ? v : 0.0;
  const double eps = (double)cfg.eps, rmax = (double)cfg.r_max, dmax = (double)cfg.d_max, mom = (double)cfg.momentum;
  const double ram = (double)ra_mean[e * e_s + c], rav = (double)ra_var[e * e_s + c];
  const double sig = sqrt(rav + eps);
  double r = sqrt(v + eps) / sig;
  r = r < 1.0 / rmax ? 1.0 / rmax : (r > rmax ? rmax : r);
  double d = (mu - ram) / sig;
  d = d < -dmax ? -dmax : (d > dmax ? dmax : d);
  const double sq = sqrt(v);
  const double cm = warmed ? mu - d * sq / r : mu;
  const double s = warmed ? 1.0 / (r * r) : 1.0;
  const double rho = 1.0 / sqrt(v * s + eps);
  const double t = (warmed && v > 0.0) ? (d / r) / (2.0 * sq) : 0.0;
  float mu_hi, mu_lo, cm_hi, cm_lo;
  brn_split(mu, mu_hi, mu_lo);
  brn_split(cm, cm_hi, cm_lo);
  co[c] = cm_hi;
  co[Dp + c] = cm_lo;
  co[2 * Dp + c] = (float)(rho * (double)g[e * e_p + c]);
  co[3 * Dp + c] = b[e * e_p + c];
  sv[c] = mu_hi;
  sv[Dp + c] = mu_lo;
  sv[2 * Dp + c] = cm_hi;
  sv[3 * Dp + c] = cm_lo;
  sv[4 * Dp + c] = (float)rho;
  sv[5 * Dp + c] = (float)s;
  sv[6 * Dp + c] = (float)t;
  ra_mean[e * e_s + c] = (float)(mom * ram + (1.0 - mom) * mu);
  ra_var[e * e_s + c] = (float)(mom * rav + (1.0 - mom) * v);
}

// coef [E][5][Dp] = g rho, dcm / M, 2 dv / M, mu hi, mu lo; save == NULL: the backward of an eval pass from the running statistics
__global__ __launch_bounds__(256) void k_brn_finish_bwd(const double* __restrict__ part, int S, int64_t M, int D, int Dp,
                                                        const float* __restrict__ g, int64_t e_p, const float* __restrict__ save,
                                                        const float* __restrict__ ra_mean, const float* __restrict__ ra_var, int64_t e_s,
                                                        float eps, float* __restrict__ coef, float* __restrict__ dg, float* __restrict__ db) {
  const int c = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
  if (c >= Dp) return;
  float* co = coef + (int64_t)e * BRN_COEF_ROWS * Dp;
  if (c >= D) {
    for (int k = 0; k < BRN_COEF_ROWS; ++k) co[k * Dp + c] = 0.f;
    return;
  }
  double sdy, sdyx;
  brn_slab_sums(part, e, S, D, c, sdy, sdyx);
  const double gg = (double)g[e * e_p + c];
  double mu = 0.0, cm, rho, k0 = 0.0, k1 = 0.0;
  if (save) {
    const float* sv = save + (int64_t)e * BRN_SAVE_ROWS * Dp;
    mu = (double)sv[c] + (double)sv[Dp + c];
    cm = (double)sv[2 * Dp + c] + (double)sv[3 * Dp + c];
    rho = (double)sv[4 * Dp + c];
    const double s = (double)sv[5 * Dp + c], t = (double)sv[6 * Dp + c];
    const double S1 = gg * sdy, S2 = gg * (sdyx - cm * sdy);
    const double dcm = -rho * S1, dcv = -0.5 * rho * rho * rho * S2;
    const double dv = dcv * s - dcm * t;
    k0 = dcm / (double)M;
    k1 = 2.0 * dv / (double)M;
  } else {
    cm = (double)ra_mean[e * e_s + c];
    rho = 1.0 / sqrt((double)ra_var[e * e_s + c] + (double)eps);
  }
  co[c] = (float)(gg * rho);
  co[Dp + c] = (float)k0;
  co[2 * Dp + c] = (float)k1;
  brn_split(mu, co[3 * Dp + c], co[4 * Dp + c]);
  if (dg) dg[e * e_p + c] = (float)(rho * (sdyx - cm * sdy));
  if (db) db[e * e_p + c] = (float)sdy;
}

// a thread's walk over the float4 groups of [M, ld]: group index i = row ld4 + cg, advanced by the grid's stride without a division
struct BrnWalk {
  int64_t row;
  int cg, step_rows, step_cg;
  __device__ __forceinline__ BrnWalk(int ld4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    row = i / ld4;
    cg = (int)(i - row * ld4);
    step_rows = (int)(stride / ld4);
    step_cg = (int)(stride - (int64_t)step_rows * ld4);
  }
  __device__ __forceinline__ void next(int ld4) {
    row += step_rows;
    cg += step_cg;
    if (cg >= ld4) {
      cg -= ld4;
      ++row;
    }
  }
};
__device__ __forceinline__ float4 brn_coef4(const float* __restrict__ row, int c, int Dp) {   // a padded coefficient row: 16-byte aligned
  return c < Dp ? *reinterpret_cast<const float4*>(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float4 brn_cols4(const float* __restrict__ p, int c, int D) {      // four entries of an unpadded [D] vector
  return make_float4(c < D ? p[c] : 0.f, c + 1 < D ? p[c + 1] : 0.f, c + 2 < D ? p[c + 2] : 0.f, c + 3 < D ? p[c + 3] : 0.f);
}

// y = (x - cm hi - cm lo) a + b.  EVAL: cm, a, b from the running statistics and the parameters themselves; else from coef
template <bool EVAL>
__global__ __launch_bounds__(256) void k_brn_apply_fwd(const float* __restrict__ x, float* __restrict__ y, int ld, int64_t M, int D, int Dp,
                                                       int64_t e_x, int64_t e_y, const float* __restrict__ coef, const float* __restrict__ g,
                                                       const float* __restrict__ b, int64_t e_p, const float* __restrict__ ra_mean,
                                                       const float* __restrict__ ra_var, int64_t e_s, float eps) {
  const int e = blockIdx.y, ld4 = ld >> 2;
  const float* xe = x + (int64_t)e * e_x;
  float* ye = y + (int64_t)e * e_y;
  const float* co = EVAL ? nullptr : coef + (int64_t)e * BRN_COEF_ROWS * Dp;
  for (BrnWalk wk(ld4); wk.row < M; wk.next(ld4)) {
    const int c = wk.cg << 2;
    const int64_t at = wk.row * ld + c;
    const float4 xv = *reinterpret_cast<const float4*>(xe + at);
    float4 cm, a, bb, cl = make_float4(0.f, 0.f, 0.f, 0.f);
    if (EVAL) {
      cm = brn_cols4(ra_mean + e * e_s, c, D);
      const float4 var = brn_cols4(ra_var + e * e_s, c, D), gg = brn_cols4(g + e * e_p, c, D);
      a = make_float4(gg.x / sqrtf(var.x + eps), gg.y / sqrtf(var.y + eps), gg.z / sqrtf(var.z + eps), gg.w / sqrtf(var.w + eps));
      bb = brn_cols4(b + e * e_p, c, D);
    } else {
      cm = brn_coef4(co, c, Dp);
      cl = brn_coef4(co + Dp, c, Dp);
      a = brn_coef4(co + 2 * Dp, c, Dp);
      bb = brn_coef4(co + 3 * Dp, c, Dp);
    }
    float4 o;
    o.x = c < D ? fmaf((xv.x - cm.x) - cl.x, a.x, bb.x) : 0.f;
    o.y = c + 1 < D ? fmaf((xv.y - cm.y) - cl.y, a.y, bb.y) : 0.f;
    o.z = c + 2 < D ? fmaf((xv.z - cm.z) - cl.z, a.z, bb.z) : 0.f;
    o.w = c + 3 < D ? fmaf((xv.w - cm.w) - cl.w, a.w, bb.w) : 0.f;
    *reinterpret_cast<float4*>(ye + at) = o;
  }
}

// dX = (dY a + k0 + k1 (x - mu hi - mu lo)) [x > 0 when relu_mask], over dY in place
__global__ __launch_bounds__(256) void k_brn_apply_bwd(const float* __restrict__ x, float* __restrict__ d, int ld, int64_t M, int D, int Dp,
                                                       int64_t e_x, int64_t e_y, const float* __restrict__ coef, int relu_mask) {
  const int e = blockIdx.y, ld4 = ld >> 2;
  const float* xe = x + (int64_t)e * e_x;
  float* de = d + (int64_t)e * e_y;
  const float* co = coef + (int64_t)e * BRN_COEF_ROWS * Dp;
  for (BrnWalk wk(ld4); wk.row < M; wk.next(ld4)) {
    const int c = wk.cg << 2;
    const int64_t at = wk.row * ld + c;
    const float4 xv = *reinterpret_cast<const float4*>(xe + at);
    const float4 dv = *reinterpret_cast<const float4*>(de + at);
    const float4 a = brn_coef4(co, c, Dp), k0 = brn_coef4(co + Dp, c, Dp), k1 = brn_coef4(co + 2 * Dp, c, Dp), mu = brn_coef4(co + 3 * Dp, c, Dp),
                 ml = brn_coef4(co + 4 * Dp, c, Dp);
    float4 o;
    o.x = fmaf(dv.x, a.x, fmaf(k1.x, (xv.x - mu.x) - ml.x, k0.x));
    o.y = fmaf(dv.y, a.y, fmaf(k1.y, (xv.y - mu.y) - ml.y, k0.y));
    o.z = fmaf(dv.z, a.z, fmaf(k1.z, (xv.z - mu.z) - ml.z, k0.z));
    o.w = fmaf(dv.w, a.w, fmaf(k1.w, (xv.w - mu.w) - ml.w, k0.w));
    if (relu_mask) {
      o.x = xv.x > 0.f ? o.x : 0.f;
      o.y = xv.y > 0.f ? o.y : 0.f;
      o.z = xv.z > 0.f ? o.z : 0.f;
      o.w = xv.w > 0.f ? o.w : 0.f;
    }
    if (c >= D) o.x = 0.f;
    if (c + 1 >= D) o.y = 0.f;
    if (c + 2 >= D) o.z = 0.f;
    if (c + 3 >= D) o.w = 0.f;
    *reinterpret_cast<float4*>(de + at) = o;
  }
}

// the backward of an eval pass when no parameter gradient is wanted: dX = dY g rsqrt(ra_var + eps) [x > 0 when relu_mask] needs no
// column sums, so this one launch replaces the three
__global__ __launch_bounds__(256) void k_brn_apply_bwd_eval(const float* __restrict__ x, float* __restrict__ d, int ld, int64_t M, int D,
                                                            int64_t e_x, int64_t e_y, const float* __restrict__ g, int64_t e_p,
                                                            const float* __restrict__ ra_var, int64_t e_s, float eps, int relu_mask) {
  const int e = blockIdx.y, ld4 = ld >> 2;
  const float* xe = x + (int64_t)e * e_x;
  float* de = d + (int64_t)e * e_y;
  for (BrnWalk wk(ld4); wk.row < M; wk.next(ld4)) {
    const int c = wk.cg << 2;
    const int64_t at = wk.row * ld + c;
    const float4 dv = *reinterpret_cast<const float4*>(de + at);
    const float4 var = brn_cols4(ra_var + e * e_s, c, D), gg = brn_cols4(g + e * e_p, c, D);
    float4 o = make_float4(dv.x * (gg.x / sqrtf(var.x + eps)), dv.y * (gg.y / sqrtf(var.y + eps)), dv.z * (gg.z / sqrtf(var.z + eps)),
                           dv.w * (gg.w / sqrtf(var.w + eps)));
    if (relu_mask) {
      const float4 xv = *reinterpret_cast<const float4*>(xe + at);
      o.x = xv.x > 0.f ? o.x : 0.f;
      o.y = xv.y > 0.f ? o.y : 0.f;
      o.z = xv.z > 0.f ? o.z : 0.f;
      o.w = xv.w > 0.f ? o.w : 0.f;
    }
    if (c >= D) o.x = 0.f;
    if (c + 1 >= D) o.y = 0.f;
    if (c + 2 >= D) o.z = 0.f;
    if (c + 3 >= D) o.w = 0.f;
    *reinterpret_cast<float4*>(de + at) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
static inline float* brn_coef_of(const rlx_ctx* ctx, float* work, int64_t M, int D, int E) {
  return work + a64(2 * (size_t)E * brn_slabs(ctx, M) * 2 * D);
}

int brn_fwd_eval(const float* x, int ld, int64_t M, int D, const float* g, const float* b, const float* ra_mean, const float* ra_var,
                 float eps, float* y, const BrnEns& n, hipStream_t st) {
  hipLaunchKernelGGL(k_brn_apply_fwd<true>, dim3(elem_grid(M * (ld >> 2)), n.E), dim3(256), 0, st, x, y, ld, M, D, brn_dp(D), n.e_x, n.e_y,
                     (const float*)nullptr, g, b, n.e_p, ra_mean, ra_var, n.e_s, eps);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int brn_fwd_train(const rlx_ctx* ctx, const float* x, int ld, int64_t M, int D, const float* g, const float* b, float* ra_mean, float* ra_var,
                  const BrnCfg& cfg, bool warmed, float* y, float* save, float* work, const BrnEns& n, hipStream_t st) {
  const int S = brn_slabs(ctx, M), Dp = brn_dp(D);
  double* part = reinterpret_cast<double*>(work);
  float* coef = brn_coef_of(ctx, work, M, D, n.E);
  hipLaunchKernelGGL(k_brn_colsum<false>, dim3(div_up(D, 64), S, n.E), dim3(256), 0, st, x, (const float*)nullptr, ld, M, D,
                     brn_rows_per_slab(ctx, M), n.e_x, n.e_y, part);
  RLX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_brn_finish_fwd, dim3(div_up(Dp, 256), n.E), dim3(256), 0, st, (const double*)part, S, M, D, Dp, g, b, n.e_p, ra_mean,
                     ra_var, n.e_s, cfg, warmed ? 1 : 0, coef, save);
  RLX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_brn_apply_fwd<false>, dim3(elem_grid(M * (ld >> 2)), n.E), dim3(256), 0, st, x, y, ld, M, D, Dp, n.e_x, n.e_y,
                     (const float*)coef, g, b, n.e_p, (const float*)nullptr, (const float*)nullptr, n.e_s, cfg.eps);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int brn_bwd(const rlx_ctx* ctx, const float* x, int ld, int64_t M, int D, const float* g, const float* save, const float* ra_mean,
            const float* ra_var, float eps, float* dY_dX, bool relu_mask, float* dg, float* db, float* work, const BrnEns& n,
            hipStream_t st) {
  if (!save && !dg && !db) {   // an eval pass's input gradient alone: no column sums
    hipLaunchKernelGGL(k_brn_apply_bwd_eval, dim3(elem_grid(M * (ld >> 2)), n.E), dim3(256), 0, st, x, dY_dX, ld, M, D, n.e_x, n.e_y, g, n.e_p,
                       ra_var, n.e_s, eps, relu_mask ? 1 : 0);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
  }
  const int S = brn_slabs(ctx, M), Dp = brn_dp(D);
  double* part = reinterpret_cast<double*>(work);
  float* coef = brn_coef_of(ctx, work, M, D, n.E);
  hipLaunchKernelGGL(k_brn_colsum<true>, dim3(div_up(D, 64), S, n.E), dim3(256), 0, st, x, (const float*)dY_dX, ld, M, D,
                     brn_rows_per_slab(ctx, M), n.e_x, n.e_y, part);
  RLX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_brn_finish_bwd, dim3(div_up(Dp, 256), n.E), dim3(256), 0, st, (const double*)part, S, M, D, Dp, g, n.e_p, save, ra_mean,
                     ra_var, n.e_s, eps, coef, dg, db);
  RLX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_brn_apply_bwd, dim3(elem_grid(M * (ld >> 2)), n.E), dim3(256), 0, st, x, dY_dX, ld, M, D, Dp, n.e_x, n.e_y, (const float*)coef,
                     relu_mask ? 1 : 0);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int rlx_brn_f32(rlx_ctx* ctx, const float* x, int ld, int64_t M, int D, int E, const float* scale_bias, float* stats, const rlx_brn_config* cfg,
                int mode, float* y_io, float* save, int relu_mask, float* dgb_out, void* stream) {
  RLX_REQUIRE(ctx && x && scale_bias && stats && cfg && y_io, RLX_EINVAL, "rlx_brn_f32: NULL pointer (ctx, x, scale_bias, stats, cfg, y_io)");
  RLX_REQUIRE(mode >= RLX_BRN_EVAL_FWD && mode <= RLX_BRN_TRAIN_BWD, RLX_EINVAL, "rlx_brn_f32: mode must be one of RLX_BRN_*");
  RLX_REQUIRE(M >= 2, RLX_EINVAL, "rlx_brn_f32: M must be at least 2 (one row has no variance)");
  RLX_REQUIRE(M <= 0x7fffffffLL, RLX_EUNSUP, "rlx_brn_f32: M at most 2^31 - 1");
  RLX_REQUIRE(D >= 1, RLX_EINVAL, "rlx_brn_f32: D must be positive");
  RLX_REQUIRE(ld >= D && ld % 4 == 0, RLX_EINVAL, "rlx_brn_f32: ld must be a multiple of 4, at least D");
  RLX_REQUIRE(E >= 1, RLX_EINVAL, "rlx_brn_f32: E must be at least 1");
  RLX_REQUIRE(E <= 16, RLX_EUNSUP, "rlx_brn_f32: E at most 16");
  RLX_REQUIRE(cfg->momentum >= 0.f && cfg->momentum < 1.f, RLX_EINVAL, "rlx_brn_f32: cfg->momentum must be in [0, 1)");
  RLX_REQUIRE(cfg->eps > 0.f, RLX_EINVAL, "rlx_brn_f32: cfg->eps must be positive");
  RLX_REQUIRE(cfg->r_max >= 1.f && cfg->d_max >= 0.f, RLX_EINVAL, "rlx_brn_f32: cfg->r_max must be at least 1 and cfg->d_max at least 0");
  RLX_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y_io & 15) == 0, RLX_EINVAL, "rlx_brn_f32: x and y_io must be 16-byte aligned");
  const bool train = mode == RLX_BRN_TRAIN_FWD || mode == RLX_BRN_TRAIN_BWD;
  RLX_REQUIRE(!train || save, RLX_EINVAL, "rlx_brn_f32: a training pass and its backward need save");
  hipStream_t st = (hipStream_t)stream;
  const BrnEns n{E, M * ld, M * ld, 2 * (int64_t)D, 2 * (int64_t)D};
  const BrnCfg c{cfg->momentum, cfg->eps, cfg->r_max, cfg->d_max};
  float *mean = stats, *var = stats + D;
  if (mode == RLX_BRN_EVAL_FWD) return brn_fwd_eval(x, ld, M, D, scale_bias, scale_bias + D, mean, var, c.eps, y_io, n, st);
  float* work = (float*)scratch(ctx, SL_STAGE, brn_work_floats(ctx, M, D, E) * sizeof(float));
  if (!work) return RLX_ENOMEM;
  if (mode == RLX_BRN_TRAIN_FWD)
    return brn_fwd_train(ctx, x, ld, M, D, scale_bias, scale_bias + D, mean, var, c, cfg->warmed != 0, y_io, save, work, n, st);
  return brn_bwd(ctx, x, ld, M, D, scale_bias, mode == RLX_BRN_TRAIN_BWD ? save : nullptr, mean, var, c.eps, y_io, relu_mask != 0, dgb_out,
                 dgb_out ? dgb_out + D : nullptr, work, n, st);
}

}  // extern "C"
