// cnn.hip -- two-dimensional convolution for the image families of the reference (rl_x/algorithms/{dqn,ddqn,c51,dqn_hl_gauss,pqn}/
// flax/critic.py: Conv(32, 8x8, 4) -> Conv(64, 4x4, 2) -> Conv(64, 3x3, 1), VALID, ReLU, pqn with a channel LayerNorm after each),
// forward, input gradient and weight gradient, and the entry points rlx_conv2d_f32 (one layer) and rlx_cnn_net_f32 (the torso,
// cnn_net.h).  Every kernel is an implicit GEMM on v_mfma_f32_32x32x2_f32, gemm.h's exact-fp32 instruction: the im2col matrix
// exists only as LDS addresses.  float32 throughout, every sum in a fixed order, no atomics: identical calls give identical bits.
//
// k_conv_fwd: a workgroup owns a band of output rows of one image (or, where an image has few pixels, up to four whole images).
// The band's input rows are staged once into LDS as Xs[ih][iw % s][ci][iw / s]; the first layer reads the uint8 NCHW observation
// and divides by 255 on the way, later layers read NHWC floats.  In that layout the 32 output pixels of an A fragment -- neighbours
// along ow -- are neighbouring floats for every (kh, kw, ci): 32 lanes on 32 banks, where the NHWC map puts them s CI floats apart
// (16 or 64: one bank).  The input-row stride is padded so that the tile's next output row continues the bank sequence.  A wave
// owns 32 pixels x CO (one or two accumulator tiles fed by the same A fragment) and walks K = (kh, kw, ci pairs) through a step
// table in LDS (A offset, weight row), so no index is divided in the loop.  B fragments come straight from W [k k CI, CO] in
// memory, 32 consecutive floats per half wave, the next group of 8 steps in flight under this group's MFMAs.  Epilogue: bias, then
// ReLU, or flax's channel LayerNorm: a pixel's CO values sit in one half wave's registers (one per lane and column tile), so the
// statistics are five butterflies; z and (mean, rstd) are kept for the backward, y = relu(LN(z) g + be) goes on.
//
// k_conv_dgrad: gather form, a workgroup per image.  d z is staged as Ds[oh + HL][co][ow + HL] inside a zero halo of HL = ceil(k/s)
// pixels, so out-of-range taps read zeros and input rows / columns that VALID padding never reads come out as exact zeros.  The
// input pixels split into s^2 phases (ih % s, iw % s); a wave owns 32 pixels of one phase's sub-grid x CI and walks only that
// phase's taps (kh = ph + s j, kw = pw + s jw) x co pairs through the phase's step table.  B comes from the transposed kernel
// Wt [k k, CO, CI] (k_conv_wt).  The ReLU mask of the layer is applied while d y is staged.
//
// k_conv_wgrad: a workgroup owns (a slab of images, 128 rows of the k k CI axis); wave w owns 32 of those rows x CO.  Per band it
// stages the input rows as NHWC (a tile's 32 rows (kh, kw, ci) are consecutive floats for CI = 4, k = 8 and for CI >= 32) and the
// band's masked d z as Ds[pixel][co], then reduces over the pixels, two per MFMA.  The accumulators live across the whole slab;
// one partial [K CO | CO] per slab goes to the stage arena and the slabs are folded in order by the tree's segment reduction.
//
// k_conv_ln_bwd: CO / 4 lanes per pixel, a float4 of channels per lane; d z in place, [d g | d be] partial rows per workgroup.
#include "cnn_net.h"

namespace rlx {

constexpr int CV_KG = 8;      // K steps (MFMAs per column tile) per fragment group

__device__ __forceinline__ float half_sum(float v) {      // over the 32 lanes of a half wave, a fixed butterfly
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int acc_pix(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }      // C row of accumulator register r

// The K walk of k_conv_fwd and k_conv_dgrad.  Step t: A = ap[tab[t].x] (ap already holds the lane's pixel and its K half lh),
// B = wp[(row + lh) ldw + 32 ct] with row = tab[t].y >> 2; bit 1 / bit 0 of tab[t].y say whether the row of lh = 0 / 1 exists.
template <int NCT>
__device__ __forceinline__ void conv_mma(const float* __restrict__ ap, const int2* __restrict__ tab, int Tp, const float* __restrict__ wp,
                                         int ldw, int lh, f32x16 (&acc)[NCT]) {
  float fb[NCT][CV_KG], fbn[NCT][CV_KG] = {}, fa[CV_KG];
  int ao[CV_KG], aon[CV_KG] = {};
  auto load = [&](int t0, float (&f)[NCT][CV_KG], int (&o)[CV_KG]) {
#pragma unroll
    for (int q = 0; q < CV_KG; ++q) {
      const int2 e = tab[t0 + q];
      o[q] = e.x;
      const bool ok = (e.y >> (1 - lh)) & 1;
      const int64_t row = (e.y >> 2) + lh;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) f[ct][q] = ok ? wp[row * ldw + 32 * ct] : 0.f;
    }
  };
  load(0, fb, ao);
  for (int t0 = 0; t0 < Tp; t0 += CV_KG) {
    if (t0 + CV_KG < Tp) load(t0 + CV_KG, fbn, aon);      // the next group's weights are in flight under this group's MFMAs
#pragma unroll
    for (int q = 0; q < CV_KG; ++q) fa[q] = ap[ao[q]];
#pragma unroll
    for (int q = 0; q < CV_KG; ++q)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q], fb[ct][q], acc[ct], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < CV_KG; ++q) {
      ao[q] = aon[q];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) fb[ct][q] = fbn[ct][q];
    }
  }
}

template <int NCT>
__device__ __forceinline__ void zero_tiles(f32x16 (&acc)[NCT]) {
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
}

// ------------------------------------------------------------------------------------------------------------ forward
struct ConvFwdArgs {
  const uint8_t* xu;
  const float *xf, *W, *b, *g, *be;
  float *y, *z, *st;
  int64_t M;
  float eps;
  ConvGeo q;
};

template <int NCT, bool U8, bool NORM>
__global__ __launch_bounds__(256) void k_conv_fwd(const ConvFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float cv_lds[];
  const ConvGeo& q = a.q;
  constexpr int CO = 32 * NCT;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int Tp = (q.T + 7) & ~7, W4 = (q.W + 3) & ~3;
  int2* tab = reinterpret_cast<int2*>(cv_lds);              // [Tp] the step table
  int* iwq = reinterpret_cast<int*>(cv_lds + 2 * Tp);       // [W] where input column iw goes inside a (row, channel) plane set
  float* Xs = cv_lds + 2 * Tp + W4;                         // [G][band input rows][RS]
  const int oh0 = blockIdx.x * q.BR, nrows = min(q.BR, q.OH - oh0), nih = (nrows - 1) * q.s + q.k, ih0 = oh0 * q.s;
  const int mapsz = ((q.BR - 1) * q.s + q.k) * q.RS;

  const int spt = q.CIe >> 1;      // steps per tap
  for (int t = tid; t < Tp; t += 256) {
    int2 e = make_int2(0, 0);      // padding steps: a valid A address, no weight row
    if (t < q.T) {
      const int tap = t / spt, ci = 2 * (t - tap * spt), kh = tap / q.k, kw = tap - kh * q.k;
      e.x = kh * q.RS + ((kw % q.s) * q.CIe + ci) * q.QWp + kw / q.s;
      e.y = ((tap * q.CI + ci) << 2) | 2 | (ci + 1 < q.CI ? 1 : 0);
    }
    tab[t] = e;
  }
  for (int iw = tid; iw < q.W; iw += 256) iwq[iw] = (iw % q.s) * q.CIe * q.QWp + iw / q.s;
  __syncthreads();

  // ---- the band's input rows of every image of the workgroup, once
  for (int u = 0; u < q.G; ++u) {
    const int64_t n = (int64_t)blockIdx.y * q.G + u;
    if (n >= a.M) break;
    float* X = Xs + u * mapsz;
    if constexpr (U8) {      // [M, CI, H, W] bytes: a wave per (channel, row), a lane per column; odd CI: a plane of zeros
      for (int rid = wv; rid < q.CIe * nih; rid += 4) {
        const int ci = rid / nih, r = rid - ci * nih;
        const uint8_t* src = a.xu + ((n * q.CI + ci) * q.H + ih0 + r) * q.W;
        float* dst = X + r * q.RS + ci * q.QWp;
        for (int iw = lane; iw < q.W; iw += 64) dst[iwq[iw]] = ci < q.CI ? (float)src[iw] / 255.0f : 0.f;
      }
    } else {                 // [M, H, W, CI] floats, CI 32 or 64: consecutive lanes take consecutive channels (plane stride odd)
      const int lg = q.CI == 32 ? 5 : 6, row_n = q.W * q.CI;
      for (int r = 0; r < nih; ++r) {
        const float* src = a.xf + (n * q.H + ih0 + r) * row_n;
        for (int e = tid; e < row_n; e += 256) X[r * q.RS + (e & (q.CI - 1)) * q.QWp + iwq[e >> lg]] = src[e];
      }
    }
  }
  __syncthreads();

  // ---- a wave per 32-pixel tile
  const int np = nrows * q.OW, ptiles = (np + 31) >> 5;
  float bv[NCT], gv[NCT], bev[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    bv[ct] = a.b[32 * ct + li];
    gv[ct] = NORM ? a.g[32 * ct + li] : 0.f;
    bev[ct] = NORM ? a.be[32 * ct + li] : 0.f;
  }
  for (int task = wv; task < q.G * ptiles; task += 4) {
    const int u = task / ptiles, pt = task - u * ptiles;
    const int64_t n = (int64_t)blockIdx.y * q.G + u;
    if (n >= a.M) break;
    const int p = pt * 32 + li, pc = p < np ? p : 0, ohl = pc / q.OW, ow = pc - ohl * q.OW;      // pixels past the band repeat pixel 0
    f32x16 acc[NCT];
    zero_tiles<NCT>(acc);
    conv_mma<NCT>(Xs + u * mapsz + ohl * q.s * q.RS + ow + lh * q.QWp, tab, Tp, a.W + li, CO, lh, acc);
    const int64_t gp0 = (n * q.OH + oh0) * q.OW;      // the band's pixels are consecutive in [M, OH, OW]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int pr = pt * 32 + acc_pix(r, lh);
      float v[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) v[ct] = acc[ct][r] + bv[ct];
      if constexpr (NORM) {
        float s = 0.f, ss = 0.f;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          s += v[ct];
          ss += v[ct] * v[ct];
        }
        const float mean = half_sum(s) * (1.0f / CO);
        const float rstd = rsqrtf(fmaxf(0.f, half_sum(ss) * (1.0f / CO) - mean * mean) + a.eps);
        if (pr < np) {
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
            a.z[(gp0 + pr) * CO + 32 * ct + li] = v[ct];
            a.y[(gp0 + pr) * CO + 32 * ct + li] = fmaxf(((v[ct] - mean) * rstd) * gv[ct] + bev[ct], 0.f);
          }
          if (li == 0) {
            a.st[2 * (gp0 + pr)] = mean;
            a.st[2 * (gp0 + pr) + 1] = rstd;
          }
        }
      } else if (pr < np) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) a.y[(gp0 + pr) * CO + 32 * ct + li] = fmaxf(v[ct], 0.f);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ input gradient
__global__ __launch_bounds__(256) void k_conv_wt(const float* __restrict__ W, float* __restrict__ Wt, int taps, int CI, int CO) {
  const int n = taps * CI * CO;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int ci = i % CI, r = i / CI, co = r % CO, tap = r / CO;
    Wt[i] = W[(tap * CI + ci) * CO + co];
  }
}

struct ConvDgArgs {
  const float *d, *ymask, *Wt;
  float* dx;
  ConvGeo q;
};

template <int NCT>      // CI / 32
__global__ __launch_bounds__(256) void k_conv_dgrad(const ConvDgArgs a) {
  extern __shared__ __attribute__((aligned(16))) float cv_lds[];
  __shared__ int ptile[65], ptab[65], poff[4][32];      // per phase: first tile, first table entry; per wave: a tile's dx pixel offsets
  const ConvGeo& q = a.q;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int CO = q.CO, lg = CO == 32 ? 5 : 6, hco = CO >> 1, P = q.s * q.s, OHP = q.OH + 2 * q.HL;
  int2* tab = reinterpret_cast<int2*>(cv_lds);      // [n_tab]
  float* Ds = cv_lds + 2 * q.n_tab;                 // [OHP][RSd]
  const int64_t n = blockIdx.x;

  if (tid == 0) {
    int tt = 0, te = 0;
    for (int p = 0; p < P; ++p) {
      const int ph = p / q.s, pw = p - ph * q.s;
      const int HA = (q.H - ph + q.s - 1) / q.s, WB = (q.W - pw + q.s - 1) / q.s, J = (q.k - ph + q.s - 1) / q.s, JW = (q.k - pw + q.s - 1) / q.s;
      ptile[p] = tt;
      ptab[p] = te;
      tt += (HA * WB + 31) >> 5;
      te += (J * JW * hco + 7) & ~7;
    }
    ptile[P] = tt;
    ptab[P] = te;
  }
  for (int i = tid; i < q.n_tab; i += 256) tab[i] = make_int2(0, 0);
  for (int i = tid; i < OHP * q.RSd; i += 256) Ds[i] = 0.f;
  __syncthreads();
  for (int e = tid; e < q.k * q.k * hco; e += 256) {
    const int tap = e >> (lg - 1), co = 2 * (e & (hco - 1)), kh = tap / q.k, kw = tap - kh * q.k;
    const int ph = kh % q.s, j = kh / q.s, pw = kw % q.s, jw = kw / q.s, JW = (q.k - pw + q.s - 1) / q.s;
    tab[ptab[ph * q.s + pw] + (j * JW + jw) * hco + (co >> 1)] = make_int2(-(j * q.RSd) - jw + co * q.OWP, ((tap * CO + co) << 2) | 3);
  }
  for (int oh = 0; oh < q.OH; ++oh) {      // d z = d y 1[y > 0] where the layer has no norm
    const int64_t base = (n * q.OH + oh) * q.OW * CO;
    for (int e = tid; e < q.OW * CO; e += 256) {
      float v = a.d[base + e];
      if (a.ymask) v = a.ymask[base + e] > 0.f ? v : 0.f;
      Ds[(oh + q.HL) * q.RSd + (e & (CO - 1)) * q.OWP + (e >> lg) + q.HL] = v;
    }
  }
  __syncthreads();

  const int total = ptile[P];
  for (int task = wv; task < total; task += 4) {
    int p = 0;
    while (ptile[p + 1] <= task) ++p;
    const int tile = task - ptile[p], ph = p / q.s, pw = p - ph * q.s;
    const int HA = (q.H - ph + q.s - 1) / q.s, WB = (q.W - pw + q.s - 1) / q.s, nq = HA * WB;
    const int qi = tile * 32 + li, qc = qi < nq ? qi : 0, ia = qc / WB, ib = qc - ia * WB;      // input pixel (ph + s ia, pw + s ib)
    __builtin_amdgcn_wave_barrier();
    if (lh == 0) poff[wv][li] = qi < nq ? (ph + q.s * ia) * q.W + pw + q.s * ib : -1;
    __builtin_amdgcn_wave_barrier();
    f32x16 acc[NCT];
    zero_tiles<NCT>(acc);
    conv_mma<NCT>(Ds + (ia + q.HL) * q.RSd + ib + q.HL + lh * q.OWP, tab + ptab[p], ptab[p + 1] - ptab[p], a.Wt + li, q.CI, lh, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = poff[wv][acc_pix(r, lh)];
      if (o >= 0) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) a.dx[(n * q.H * q.W + o) * q.CI + 32 * ct + li] = acc[ct][r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ weight gradient
struct ConvWgArgs {
  const uint8_t* xu;
  const float *xf, *d, *ymask;
  float* part;
  int64_t M, PS;      // PS: floats of a slab's partial [K CO | CO], each part padded to four
  int boff, ips;      // where the bias part starts; images per slab
  ConvGeo q;
};

template <int NCT, bool U8>
__global__ __launch_bounds__(256) void k_conv_wgrad(const ConvWgArgs a) {
  extern __shared__ __attribute__((aligned(16))) float cv_lds[];
  const ConvGeo& q = a.q;
  constexpr int CO = 32 * NCT;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
  int* pixtab = reinterpret_cast<int*>(cv_lds);      // [NPw] a band pixel's offset in Xs
  float* Ds = cv_lds + q.NPw;                        // [NPw][CO]
  float* Xs = Ds + q.NPw * CO;                       // [band input rows][W][CI]
  const int K = q.k * q.k * q.CI, kt = blockIdx.x, row0 = (kt * 4 + wv) * 32;
  const bool wave_on = row0 < K;
  int rowoff = 0;      // the lane's row (kh, kw, ci) of the K axis as an offset in Xs
  if (row0 + li < K) {
    const int kr = row0 + li, tap = kr / q.CI, ci = kr - tap * q.CI, kh = tap / q.k, kw = tap - kh * q.k;
    rowoff = (kh * q.W + kw) * q.CI + ci;
  }
  for (int p = tid; p < q.NPw; p += 256) pixtab[p] = p < q.BRw * q.OW ? ((p / q.OW) * q.s * q.W + (p % q.OW) * q.s) * q.CI : 0;

  f32x16 acc[NCT];
  zero_tiles<NCT>(acc);
  float dbacc = 0.f;
  const int64_t n0 = (int64_t)blockIdx.y * a.ips, n1 = n0 + a.ips < a.M ? n0 + a.ips : a.M;
  for (int64_t n = n0; n < n1; ++n) {
    for (int band = 0; band < q.NBw; ++band) {
      const int oh0 = band * q.BRw, nrows = min(q.BRw, q.OH - oh0), nih = (nrows - 1) * q.s + q.k, ih0 = oh0 * q.s;
      const int np = nrows * q.OW, npP = (np + 15) & ~15;
      __syncthreads();      // the band before this one has been consumed (and pixtab written)
      if constexpr (U8) {
        for (int rid = wv; rid < q.CI * nih; rid += 4) {
          const int ci = rid / nih, r = rid - ci * nih;
          const uint8_t* src = a.xu + ((n * q.CI + ci) * q.H + ih0 + r) * q.W;
          for (int iw = lane; iw < q.W; iw += 64) Xs[(r * q.W + iw) * q.CI + ci] = (float)src[iw] / 255.0f;
        }
      } else {      // NHWC in memory and in LDS: a copy (CI 32 or 64: whole float4s)
        const float4* src = reinterpret_cast<const float4*>(a.xf + (n * q.H + ih0) * q.W * q.CI);
        for (int e = tid; e < nih * q.W * (q.CI >> 2); e += 256) reinterpret_cast<float4*>(Xs)[e] = src[e];
      }
      const int64_t base = (n * q.OH + oh0) * q.OW * CO;
      for (int e = tid; e < npP * CO; e += 256) {
        float v = 0.f;
        if (e < np * CO) {
          v = a.d[base + e];
          if (a.ymask) v = a.ymask[base + e] > 0.f ? v : 0.f;
        }
        Ds[e] = v;
      }
      __syncthreads();
      if (kt == 0 && tid < CO)
        for (int p = 0; p < np; ++p) dbacc += Ds[p * CO + tid];
      if (wave_on) {
        for (int p0 = 0; p0 < npP; p0 += 2 * CV_KG) {
          float fa[CV_KG], fb[NCT][CV_KG];
#pragma unroll
          for (int g = 0; g < CV_KG; ++g) {
            const int p = p0 + 2 * g + lh;      // pixels past the band: d z = 0 against the band's first pixel
            fa[g] = Xs[rowoff + (p < np ? pixtab[p] : 0)];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) fb[ct][g] = Ds[p * CO + 32 * ct + li];
          }
#pragma unroll
          for (int g = 0; g < CV_KG; ++g)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g], fb[ct][g], acc[ct], 0, 0, 0);
        }
      }
    }
  }
  float* part = a.part + (int64_t)blockIdx.y * a.PS;
  if (wave_on) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kr = row0 + acc_pix(r, lh);
      if (kr < K) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) part[(int64_t)kr * CO + 32 * ct + li] = acc[ct][r];
      }
    }
  }
  if (kt == 0 && tid < CO) part[a.boff + tid] = dbacc;
}

// ------------------------------------------------------------------------------------------------------------ channel LayerNorm backward
// From d y 1[y > 0] (the forward's stored y: the mask is the forward's by construction):  d g = sum d y x^,  d be = sum d y,  d x^ = d y g,  d z = rstd (d x^ - mean(d x^) - x^ mean(d x^ x^))
template <int CO>
__global__ __launch_bounds__(256) void k_conv_ln_bwd(const float* __restrict__ z, const float* __restrict__ st, const float* __restrict__ g,
                                                     const float* __restrict__ y, float* __restrict__ d, int64_t rows,
                                                     float* __restrict__ part) {
  constexpr int LPP = CO / 4, PPW = 64 / LPP;      // lanes per pixel, pixels per wave
  __shared__ float fold[4][2 * CO];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c4 = lane % LPP, sub = lane / LPP;
  const float4 g4 = reinterpret_cast<const float4*>(g)[c4];
  float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
  const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
  for (int64_t p0 = ((int64_t)blockIdx.x * 4 + wv) * PPW; p0 < rows; p0 += (int64_t)gridDim.x * 4 * PPW) {      // (wave-uniform trip count)
    const int64_t p = p0 + sub;
    const bool on = p < rows;
    float xh[4] = {0.f, 0.f, 0.f, 0.f}, dy[4] = {0.f, 0.f, 0.f, 0.f}, rstd = 0.f;
    if (on) {
      const float4 z4 = reinterpret_cast<const float4*>(z + p * CO)[c4], d4 = reinterpret_cast<const float4*>(d + p * CO)[c4];
      const float4 y4 = reinterpret_cast<const float4*>(y + p * CO)[c4];
      const float mean = st[2 * p];
      rstd = st[2 * p + 1];
      const float zz[4] = {z4.x, z4.y, z4.z, z4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w}, yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xh[i] = (zz[i] - mean) * rstd;
        dy[i] = yy[i] > 0.f ? dd[i] : 0.f;
      }
    }
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dg[i] += dy[i] * xh[i];
      db[i] += dy[i];
      dy[i] *= gg[i];      // d x^
      m1 += dy[i];
      m2 += dy[i] * xh[i];
    }
#pragma unroll
    for (int m = 1; m < LPP; m <<= 1) {
      m1 += __shfl_xor(m1, m, 64);
      m2 += __shfl_xor(m2, m, 64);
    }
    m1 *= 1.0f / CO;
    m2 *= 1.0f / CO;
    if (on) reinterpret_cast<float4*>(d + p * CO)[c4] = make_float4((dy[0] - m1 - xh[0] * m2) * rstd, (dy[1] - m1 - xh[1] * m2) * rstd,
                                                                     (dy[2] - m1 - xh[2] * m2) * rstd, (dy[3] - m1 - xh[3] * m2) * rstd);
  }
  // the wave's pixel sub-groups fold by butterflies, the four waves through LDS in wave order: one partial row per workgroup
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int m = LPP; m < 64; m <<= 1) {
      dg[i] += __shfl_xor(dg[i], m, 64);
      db[i] += __shfl_xor(db[i], m, 64);
    }
  if (lane < LPP) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      fold[wv][4 * c4 + i] = dg[i];
      fold[wv][CO + 4 * c4 + i] = db[i];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * CO) {
    const int i = threadIdx.x;
    part[(int64_t)blockIdx.x * 2 * CO + i] = ((fold[0][i] + fold[1][i]) + fold[2][i]) + fold[3][i];
  }
}

// ------------------------------------------------------------------------------------------------------------ geometry and launchers
int cnn_lds_limit(const rlx_ctx* ctx, size_t* out) {
  static size_t cache[64];      // per device, queried once (0: not yet)
  size_t& c = cache[ctx->device & 63];
  if (!c) {
    int lim = 0;
    RLX_HIP_TRY(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    RLX_REQUIRE(lim > 2048, RLX_EHIP, "cnn_lds_limit: the device reports no usable LDS per workgroup");
    c = (size_t)lim - 2048;      // (room for k_conv_dgrad's static tables)
  }
  *out = c;
  return RLX_OK;
}

// padding of a row stride `base` so that s rows later a tile's lanes continue on the banks after the OW pixels of this row
static int bank_pad(int base, int s, int OW) {
  for (int t = 0; t < 32; ++t)
    for (int pad = 0; pad < 32; ++pad)
      if ((s * (base + pad)) % 32 == (OW + t) % 32) return pad;
  return 0;
}

static size_t fwd_bytes(const ConvGeo& g, int rows, int G) {
  return ((size_t)2 * ((g.T + 7) & ~7) + ((g.W + 3) & ~3) + (size_t)G * ((rows - 1) * g.s + g.k) * g.RS) * sizeof(float);
}
static size_t wg_bytes(const ConvGeo& g, int rows) {
  const size_t npw = (size_t)((rows * g.OW + 15) & ~15);
  return (npw + npw * g.CO + (size_t)((rows - 1) * g.s + g.k) * g.W * g.CI) * sizeof(float);
}

int conv_geometry(const rlx_ctx* ctx, ConvGeo* gp, bool need_dgrad, const char* who) {
  ConvGeo& g = *gp;
  size_t lim = 0;
  const int rcl = cnn_lds_limit(ctx, &lim);
  if (rcl) return rcl;
  g.lds_lim = (int)lim;
  g.CIe = (g.CI + 1) & ~1;
  g.T = g.k * g.k * g.CIe / 2;
  g.QWp = ((g.W + g.s - 1) / g.s) | 1;
  g.RS = g.s * g.CIe * g.QWp;
  g.RS += bank_pad(g.RS, g.s, g.OW);
  RLX_REQUIRE(fwd_bytes(g, 1, 1) <= lim, RLX_EUNSUP,
              std::string(who) + ": kernel, in_w, channels: the `kernel` input rows of one output row do not fit the device's LDS (forward)");
  g.BR = 1;
  for (int r = g.OH; r > 1; --r)
    if (r * g.OW <= CNN_BAND_PIXELS && fwd_bytes(g, r, 1) <= CNN_LDS_SOFT) { g.BR = r; break; }
  g.NB = div_up(g.OH, g.BR);
  g.G = 1;
  if (g.NB == 1) {
    g.G = 4 / div_up(g.OH * g.OW, 32);
    if (g.G < 1) g.G = 1;
    while (g.G > 1 && fwd_bytes(g, g.BR, g.G) > CNN_LDS_SOFT) --g.G;
  }
  g.lds_fwd = fwd_bytes(g, g.BR, g.G);

  RLX_REQUIRE(wg_bytes(g, 1) <= lim, RLX_EUNSUP,
              std::string(who) + ": kernel, in_w, channels: the `kernel` input rows of one output row do not fit the device's LDS (weight gradient)");
  g.BRw = 1;
  for (int r = g.OH; r > 1; --r)
    if (wg_bytes(g, r) <= CNN_LDS_SOFT) { g.BRw = r; break; }
  g.NBw = div_up(g.OH, g.BRw);
  g.NPw = (g.BRw * g.OW + 15) & ~15;
  g.lds_wg = wg_bytes(g, g.BRw);

  g.HL = (g.k + g.s - 1) / g.s;
  g.OWP = (g.OW + 2 * g.HL) | 1;
  g.RSd = g.CO * g.OWP;
  g.RSd += bank_pad(g.RSd, 1, (g.W + g.s - 1) / g.s);
  g.n_tab = 0;
  for (int p = 0; p < g.s * g.s; ++p) {
    const int ph = p / g.s, pw = p % g.s;
    g.n_tab += (((g.k - ph + g.s - 1) / g.s) * ((g.k - pw + g.s - 1) / g.s) * (g.CO / 2) + 7) & ~7;
  }
  g.lds_dg = ((size_t)2 * g.n_tab + (size_t)(g.OH + 2 * g.HL) * g.RSd) * sizeof(float);
  RLX_REQUIRE(!need_dgrad || g.lds_dg <= lim, RLX_EUNSUP,
              std::string(who) + ": kernel, stride, channels: the layer's output map with its halo does not fit the device's LDS (input gradient)");
  return RLX_OK;
}

// dynamic LDS above the default: once per kernel and device
template <class Kern>
static int lds_attr(Kern kern, AttrOnce& once, int lds_lim) {
  if (once.done()) return RLX_OK;
  RLX_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_lim));
  once.mark();
  return RLX_OK;
}

template <int NCT, bool U8, bool NORM>
static int conv_fwd_launch(const ConvFwdArgs& a, hipStream_t stm) {
  static AttrOnce once;
  const int rc = lds_attr(k_conv_fwd<NCT, U8, NORM>, once, a.q.lds_lim);
  if (rc) return rc;
  hipLaunchKernelGGL((k_conv_fwd<NCT, U8, NORM>), dim3(a.q.NB, div_up(a.M, a.q.G)), dim3(256), a.q.lds_fwd, stm, a);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
int conv_fwd(const ConvGeo& q, const uint8_t* xu, const float* xf, const float* W, const float* b, const float* g, const float* be, float eps,
             int64_t M, float* y, float* z, float* st, hipStream_t stm) {
  const ConvFwdArgs a{xu, xf, W, b, g, be, y, z, st, M, eps, q};
#define CV_FWD(NCT)                                                                    \
  if (xu) return g ? conv_fwd_launch<NCT, true, true>(a, stm) : conv_fwd_launch<NCT, true, false>(a, stm); \
  return g ? conv_fwd_launch<NCT, false, true>(a, stm) : conv_fwd_launch<NCT, false, false>(a, stm);
  if (q.CO == 32) { CV_FWD(1) }
  CV_FWD(2)
#undef CV_FWD
}

int conv_ln_bwd(rlx_ctx* ctx, const ConvGeo& q, const float* z, const float* st, const float* g, const float* y, float* d, int64_t M,
                float* g_g, float* g_be, hipStream_t stm) {
  const int64_t rows = M * q.OH * q.OW;
  const int ppb = 4 * (q.CO == 32 ? 8 : 4);      // pixels of one pass of a workgroup
  int grid = div_up(rows, 4 * ppb);              // at least four passes each: fewer partial rows
  if (grid > ctx->num_cus * 4) grid = ctx->num_cus * 4;
  float* part = stage_alloc(ctx, (size_t)grid * 2 * q.CO);
  if (!part) return RLX_ENOMEM;
  if (q.CO == 32) hipLaunchKernelGGL(k_conv_ln_bwd<32>, dim3(grid), dim3(256), 0, stm, z, st, g, y, d, rows, part);
  else hipLaunchKernelGGL(k_conv_ln_bwd<64>, dim3(grid), dim3(256), 0, stm, z, st, g, y, d, rows, part);
  RLX_LAUNCH_CHECK();
  return norm_bwd_reduce(ctx, part, grid, q.CO, g_g, g_be, stm);
}

template <int NCT, bool U8>
static int conv_wgrad_launch(const ConvWgArgs& a, int ntk, int S, hipStream_t stm) {
  static AttrOnce once;
  const int rc = lds_attr(k_conv_wgrad<NCT, U8>, once, a.q.lds_lim);
  if (rc) return rc;
  hipLaunchKernelGGL((k_conv_wgrad<NCT, U8>), dim3(ntk, S), dim3(256), a.q.lds_wg, stm, a);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
// the slabs of the weight gradient: a function of M, the CU count and the layer's K tiles only
static int conv_wgrad_slabs(const rlx_ctx* ctx, const ConvGeo& q, int64_t M, int* ips_out) {
  const int ntk = div_up(q.k * q.k * q.CI, 128);
  int64_t S = ctx->num_cus / ntk;
  if (S < 1) S = 1;
  if (S > M) S = M;
  const int64_t ips = (M + S - 1) / S;
  *ips_out = (int)ips;
  return (int)((M + ips - 1) / ips);
}
int conv_wgrad(rlx_ctx* ctx, const ConvGeo& q, const uint8_t* xu, const float* xf, const float* d, const float* ymask, int64_t M, float* gW,
               float* gb, hipStream_t stm) {
  const int K = q.k * q.k * q.CI, ntk = div_up(K, 128);
  ConvWgArgs a{xu, xf, d, ymask, nullptr, M, 0, 0, 0, q};
  const int S = conv_wgrad_slabs(ctx, q, M, &a.ips);
  a.boff = (K * q.CO + 3) & ~3;
  a.PS = a.boff + q.CO;
  a.part = stage_alloc(ctx, (size_t)S * a.PS);
  if (!a.part) return RLX_ENOMEM;
  int rc;
  if (q.CO == 32) rc = xu ? conv_wgrad_launch<1, true>(a, ntk, S, stm) : conv_wgrad_launch<1, false>(a, ntk, S, stm);
  else rc = xu ? conv_wgrad_launch<2, true>(a, ntk, S, stm) : conv_wgrad_launch<2, false>(a, ntk, S, stm);
  if (rc) return rc;
  ReduceTable tab;
  tab.n = 0;
  tab.seg[tab.n++] = ReduceSeg{a.part, gW, (int64_t)K * q.CO, a.PS, S, 0, 1.f, 0.f, 1};
  tab.seg[tab.n++] = ReduceSeg{a.part + a.boff, gb, (int64_t)q.CO, a.PS, S, 0, 1.f, 0.f, 1};
  return stage_reduce(ctx, tab, nullptr, nullptr, stm);
}

int conv_wt(const ConvGeo& q, const float* W, float* Wt, hipStream_t stm) {
  const int taps = q.k * q.k;
  hipLaunchKernelGGL(k_conv_wt, dim3(elem_grid((int64_t)taps * q.CI * q.CO)), dim3(256), 0, stm, W, Wt, taps, q.CI, q.CO);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
template <int NCT>
static int conv_dgrad_launch(const ConvDgArgs& a, int64_t M, hipStream_t stm) {
  static AttrOnce once;
  const int rc = lds_attr(k_conv_dgrad<NCT>, once, a.q.lds_lim);
  if (rc) return rc;
  hipLaunchKernelGGL(k_conv_dgrad<NCT>, dim3((unsigned)M), dim3(256), a.q.lds_dg, stm, a);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
int conv_dgrad(const ConvGeo& q, const float* d, const float* ymask, const float* Wt, int64_t M, float* dx, hipStream_t stm) {
  const ConvDgArgs a{d, ymask, Wt, dx, q};
  return q.CI == 32 ? conv_dgrad_launch<1>(a, M, stm) : conv_dgrad_launch<2>(a, M, stm);
}

static bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t m = 0;
  for (const void* p : ps) m |= (uintptr_t)p;
  return (m & 15) == 0;
}

// one layer's problem fields (RLX_EUNSUP, naming the field as `who` spells it)
static int conv_check(const char* who, int l, int CI, int H, int W, int k, int s, int CO) {
  const std::string at = std::string(who) + (l >= 0 ? ": layer " + std::to_string(l) + ": " : ": ");
  RLX_REQUIRE(CO == 32 || CO == 64, RLX_EUNSUP, at + "ch (output channels) must be 32 or 64");
  RLX_REQUIRE(k >= 1 && k <= 8, RLX_EUNSUP, at + "kernel must be 1..8");
  RLX_REQUIRE(s >= 1 && s <= k, RLX_EUNSUP, at + "stride must be 1..kernel");
  RLX_REQUIRE(H >= k && W >= k, RLX_EUNSUP, at + "kernel is larger than the layer's input map");
  RLX_REQUIRE(CI >= 1 && H <= 128 && W <= 128, RLX_EUNSUP, at + "in_h, in_w must be at most 128");
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int64_t rlx_cnn_param_count(const rlx_cnn_desc* t) {
  if (!t || t->n_conv < 1 || t->n_conv > CNN_MAX_CONV || t->in_c < 1 || t->in_h < 1 || t->in_w < 1 || t->hidden < 1 || t->out_dim < 1) return -1;
  for (int l = 0; l < t->n_conv; ++l)
    if (t->ch[l] < 1) return -1;
  Cnn E;
  return make_cnn(*t, &E) ? E.n_params : -1;
}

int rlx_conv2d_f32(rlx_ctx* ctx, const uint8_t* x_u8, const float* x_f32, int64_t M, int H, int W, int CI, int kernel, int stride, int CO,
                   const float* Wt, const float* b, const float* g_be, float ln_eps, float* y, const float* d_y, float* dx, float* gW,
                   float* gb, float* g_gbe, void* stream) {
  RLX_REQUIRE(ctx && Wt && b && y, RLX_EINVAL, "rlx_conv2d_f32: NULL pointer (ctx, Wt, b, y)");
  RLX_REQUIRE((x_u8 != nullptr) != (x_f32 != nullptr), RLX_EINVAL, "rlx_conv2d_f32: exactly one of x_u8 and x_f32");
  RLX_REQUIRE(!d_y || (gW && gb && (!g_be || g_gbe)), RLX_EINVAL, "rlx_conv2d_f32: a backward (d_y) needs gW, gb and, with norm, g_gbe");
  RLX_REQUIRE(!dx || (d_y && x_f32), RLX_EINVAL, "rlx_conv2d_f32: dx needs d_y and a float32 input (the image gets no gradient)");
  int rc = conv_check("rlx_conv2d_f32", -1, CI, H, W, kernel, stride, CO);
  if (rc) return rc;
  RLX_REQUIRE(x_u8 ? CI <= 8 : (CI == 32 || CI == 64), RLX_EUNSUP, "rlx_conv2d_f32: CI must be 1..8 for a uint8 input, 32 or 64 for a float32 one");
  RLX_REQUIRE(!g_be || (ln_eps > 0.f && std::isfinite(ln_eps)), RLX_EUNSUP, "rlx_conv2d_f32: ln_eps must be positive");
  RLX_REQUIRE(M >= 1 && M <= (1 << 16), RLX_EUNSUP, "rlx_conv2d_f32: M must be 1..2^16 images");
  RLX_REQUIRE(aligned16({x_f32, Wt, b, g_be, y, d_y, dx, gW, gb, g_gbe}), RLX_EINVAL, "rlx_conv2d_f32: float pointers must be 16-byte aligned");
  ConvGeo q{};
  q.H = H; q.W = W; q.CI = CI; q.CO = CO; q.k = kernel; q.s = stride; q.OH = (H - kernel) / stride + 1; q.OW = (W - kernel) / stride + 1;
  q.u8 = x_u8 != nullptr;
  rc = conv_geometry(ctx, &q, dx != nullptr, "rlx_conv2d_f32");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)M * q.OH * q.OW;
  float *z = nullptr, *stats = nullptr, *dz = nullptr, *wt = nullptr;
  auto carve = [&](Arena& a) {
    if (g_be) { z = a.take(n * CO); stats = a.take(2 * n); }
    if (g_be && d_y) dz = a.take(n * CO);
    if (dx) wt = a.take((size_t)kernel * kernel * CI * CO);
  };
  if (arena_floats(carve)) rc = arena_carve(ctx, SL_CNN, carve);      // (a plain layer without dx keeps nothing)
  if (rc) return rc;
  rc = conv_fwd(q, x_u8, x_f32, Wt, b, g_be, g_be ? g_be + CO : nullptr, ln_eps, M, y, z, stats, st);
  if (rc || !d_y) return rc;
  const float *d = d_y, *mask = y;
  if (g_be) {      // d z from a copy of d y (the caller's stays as it is)
    RLX_HIP_TRY(hipMemcpyAsync(dz, d_y, n * CO * sizeof(float), hipMemcpyDeviceToDevice, st));
    rc = conv_ln_bwd(ctx, q, z, stats, g_be, y, dz, M, g_gbe, g_gbe + CO, st);
    if (rc) return rc;
    d = dz;
    mask = nullptr;
  }
  rc = conv_wgrad(ctx, q, x_u8, x_f32, d, mask, M, gW, gb, st);
  if (rc || !dx) return rc;
  rc = conv_wt(q, Wt, wt, st);
  return rc ? rc : conv_dgrad(q, d, mask, wt, M, dx, st);
}

int rlx_cnn_net_f32(rlx_ctx* ctx, const rlx_cnn_desc* desc, const float* params, const uint8_t* x, int64_t M, float* out, const float* d_out,
                    float* grads, void* stream) {
  RLX_REQUIRE(ctx && desc && params && x && out, RLX_EINVAL, "rlx_cnn_net_f32: NULL pointer (ctx, desc, params, x, out)");
  RLX_REQUIRE(!d_out || grads, RLX_EINVAL, "rlx_cnn_net_f32: a backward (d_out) needs grads");
  const rlx_cnn_desc& t = *desc;
  RLX_REQUIRE(t.n_conv >= 1 && t.n_conv <= CNN_MAX_CONV, RLX_EUNSUP, "rlx_cnn_net_f32: n_conv must be 1..3");
  RLX_REQUIRE(t.in_c >= 1 && t.in_c <= 8, RLX_EUNSUP, "rlx_cnn_net_f32: in_c must be 1..8");
  RLX_REQUIRE(t.in_h >= 1 && t.in_h <= 128 && t.in_w >= 1 && t.in_w <= 128, RLX_EUNSUP, "rlx_cnn_net_f32: in_h, in_w must be 1..128");
  RLX_REQUIRE(t.hidden >= 64 && t.hidden % 64 == 0 && t.hidden <= 1024, RLX_EUNSUP, "rlx_cnn_net_f32: hidden must be a multiple of 64 up to 1024");
  RLX_REQUIRE(t.out_dim >= 1 && t.out_dim <= 2048, RLX_EUNSUP, "rlx_cnn_net_f32: out_dim must be 1..2048");
  RLX_REQUIRE(t.ln_eps > 0.f && std::isfinite(t.ln_eps), RLX_EUNSUP, "rlx_cnn_net_f32: ln_eps must be positive");
  RLX_REQUIRE(M >= 1 && M <= (1 << 16), RLX_EUNSUP, "rlx_cnn_net_f32: M must be 1..2^16 images");
  int H = t.in_h, W = t.in_w, C = t.in_c;
  for (int l = 0; l < t.n_conv; ++l) {
    const int rc = conv_check("rlx_cnn_net_f32", l, C, H, W, t.kernel[l], t.stride[l], t.ch[l]);
    if (rc) return rc;
    H = (H - t.kernel[l]) / t.stride[l] + 1; W = (W - t.kernel[l]) / t.stride[l] + 1; C = t.ch[l];
  }
  RLX_REQUIRE(aligned16({params, out, d_out, grads}), RLX_EINVAL, "rlx_cnn_net_f32: params, out, d_out and grads must be 16-byte aligned");
  Cnn E;
  RLX_REQUIRE(make_cnn(t, &E), RLX_EUNSUP, "rlx_cnn_net_f32: kernel is larger than a layer's input map");
  const bool bwd = d_out != nullptr;
  for (int l = 0; l < E.n_conv; ++l) {
    const int rc = conv_geometry(ctx, &E.cv[l].q, bwd && l > 0, "rlx_cnn_net_f32");
    if (rc) return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  CnnBufs B;
  int rc = arena_carve(ctx, SL_CNN, [&](Arena& a) { cnn_carve(E, M, bwd, a, &B); });
  if (rc) return rc;
  rc = cnn_fwd(ctx, E, params, x, M, B, out, st);
  if (rc || !bwd) return rc;
  return cnn_bwd(ctx, E, params, x, M, B, d_out, grads, st);
}

}  // extern "C"
