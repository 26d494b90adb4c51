// gemm_sk.hip -- the split-K forward GEMM for few rows and a long K (gfx950):
//   C[M, N] = act(A[M, K] W[K, N] + bias[N]),   1 <= M <= 1024, N % 4 == 0, K % 4 == 0
// on v_mfma_f32_32x32x2_f32 (exact fp32 operands and accumulation, gemm.h).  k_gemm_fwd covers C with 128 x 128 tiles, each
// walking the whole K axis alone: at 32 x 512 outputs that is four workgroups on 256 CUs.  Here a workgroup owns 32 rows, 64
// columns and ONE SLICE of the K axis; the grid is ceil(M / 32) x ceil(N / 64) x S.
//
// k_gemm_sk<ACT>: four waves.  Wave w owns column tile w & 1 of the strip and K half w >> 1 of every stage of the slice.
//   A side: the slice's 32 x Ks part of A goes through LDS as [32][Lp + 1] floats (Lp: the stage's columns rounded up to 32, so
//     that both K halves are whole groups of 8 MFMA steps; the odd stride puts the 32 rows of a fragment on 32 banks), loaded with
//     16-byte loads along K where A's address allows it, rows >= M and columns >= the slice's end written as zeros.  A slice longer
//     than 512 columns is walked in stages of 512: 32 x 513 floats + the 8 KB fold buffer = 73 856 bytes, two workgroups per CU.
//   B side: fragments straight from W -- a half-wave load is 32 consecutive floats of one row, every weight element is read once
//     per row tile.  A wave keeps the 32 loads of its NEXT 64 k in flight under the 32 MFMAs of the current 64 k (one group of 16 k
//     is 512 matrix-pipe cycles, too short a cover for a trip to HBM), and the first 64 k of a stage are requested in front of the
//     stage's A loads.  Columns >= N are neither loaded nor stored; rows of W at or beyond the slice's end are never multiplied in
//     (the load is clamped to the slice's last row and the value replaced by zero).
//   The two K halves meet in LDS, lower half first.  ACT >= 0 (S == 1): bias, activation and store, a single launch.  ACT < 0
//   (S > 1): the raw partial tile goes to P[s][M][N].
// k_gemm_sk_finish<ACT>: C = act((((P[0] + P[1]) + P[2]) + ...) + bias), one float4 per thread (scalar where C or bias is not 16-byte
//   aligned).  No atomics, no scratch memory: identical calls give identical bits.
//
// The slices: K holds G = K / 16 whole groups and a tail of K % 16.  Slice s takes G / S groups, the first G % S slices one more,
// the last slice the tail: every slice but the last is a multiple of 16 k.  gemm_sk_slices() is the host rule.
#include "mlp.h"

namespace rlx {

constexpr int SK_TM = 32, SK_TN = 64;      // a workgroup's rows and output columns
constexpr int SK_STAGE = 512;              // columns of a slice in LDS at a time
constexpr int SK_KG = 8;                   // MFMA steps (k-pairs) per group
constexpr int SK_NG = 4;                   // groups per B request: 64 k, 32 loads per lane in flight
constexpr int SK_FOLD = 2 * 16 * 64;       // floats: the upper K half's accumulators of both column tiles
constexpr int SK_MIN_GROUPS = 2;           // the floor of a slice: 32 k, one whole group for each K half
constexpr int SK_MAX_SLICES = 64;
constexpr size_t SK_PARTIAL_CAP = size_t(64) << 20;      // bytes of P at most; S shrinks until S M N floats fit

struct SkArgs {
  const float *A, *W, *bias;
  float *C, *P;
  int64_t M;
  int N, K, lda, S, G, ldsw, vec_a;      // G: whole 16-k groups of K; ldsw: columns of As (the longest stage, rounded up to 32)
};

template <int ACT>
__global__ __launch_bounds__(256) void k_gemm_sk(const SkArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sk_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ct = wv & 1, kh = wv >> 1, li = lane & 31, lh = lane >> 5;
  const int LD = a.ldsw + 1;
  float* As = sk_lds;                       // [32][LD]
  float* fold = sk_lds + SK_TM * LD;        // [2][16][64]
  const int64_t row0 = (int64_t)blockIdx.x * SK_TM;
  const int s = blockIdx.z;
  const int base = a.G / a.S, rem = a.G % a.S;
  const int g0 = s * base + (s < rem ? s : rem);
  const int kbeg = 16 * g0;
  const int kend = s == a.S - 1 ? a.K : 16 * (g0 + base + (s < rem ? 1 : 0));
  const int col = blockIdx.y * SK_TN + ct * 32 + li;
  const bool col_ok = col < a.N;
  const float* wp = a.W + (col_ok ? col : 0);      // B[k = lh + .][j = li]: W[k, col]
  const float* ap = As + li * LD + lh;             // A[i = li][k = lh + .]

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float fb[SK_NG * SK_KG], fbn[SK_NG * SK_KG] = {};
  // the 64 k from row k0 of W on: plain loads where they all lie inside the slice (uniform), else clamped and masked
  auto load_b = [&](int k0, float (&f)[SK_NG * SK_KG]) {
    if (k0 + 2 * SK_NG * SK_KG <= kend) {
      const float* w0 = wp + (int64_t)(k0 + lh) * a.N;
#pragma unroll
      for (int q = 0; q < SK_NG * SK_KG; ++q) f[q] = w0[(int64_t)(2 * q) * a.N];
    } else {
#pragma unroll
      for (int q = 0; q < SK_NG * SK_KG; ++q) {
        const int k = k0 + 2 * q + lh;
        const float v = wp[(int64_t)(k < kend ? k : kend - 1) * a.N];
        f[q] = k < kend ? v : 0.f;
      }
    }
  };

  for (int kst = kbeg; kst < kend; kst += SK_STAGE) {
    const int len = kend - kst < SK_STAGE ? kend - kst : SK_STAGE;
    const int Lp = (len + 31) & ~31;
    const int hbeg = kh * (Lp >> 1), hend = hbeg + (Lp >> 1);      // this wave's columns of the stage
    load_b(kst + hbeg, fb);
    if (kst != kbeg) __syncthreads();      // every wave has read the stage before
    // ---- the stage of A: wave wv stores rows wv, wv + 4, ..., eight loads in flight per lane
    if (a.vec_a) {
      const int nch = Lp >> 2, vch = len >> 2;
      for (int j = lane; j < nch; j += 64) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t m = row0 + wv + 4 * u;
          v[u] = (m < a.M && j < vch) ? *reinterpret_cast<const float4*>(a.A + m * a.lda + kst + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          float* t = As + (wv + 4 * u) * LD + 4 * j;
          t[0] = v[u].x; t[1] = v[u].y; t[2] = v[u].z; t[3] = v[u].w;
        }
      }
    } else {
      for (int c = lane; c < Lp; c += 64) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t m = row0 + wv + 4 * u;
          v[u] = (m < a.M && c < len) ? a.A[m * a.lda + kst + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) As[(wv + 4 * u) * LD + c] = v[u];
      }
    }
    __syncthreads();
    // ---- this wave's K half of the stage, 64 k per trip
    for (int c = hbeg; c < hend; c += 2 * SK_NG * SK_KG) {
      if (c + 2 * SK_NG * SK_KG < hend) load_b(kst + c + 2 * SK_NG * SK_KG, fbn);
#pragma unroll
      for (int g = 0; g < SK_NG; ++g) {
        if (c + 2 * SK_KG * g < hend) {      // (uniform: a half is a whole number of groups)
          float fa[SK_KG];
#pragma unroll
          for (int q = 0; q < SK_KG; ++q) fa[q] = ap[c + 2 * SK_KG * g + 2 * q];
#pragma unroll
          for (int q = 0; q < SK_KG; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q], fb[SK_KG * g + q], acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int q = 0; q < SK_NG * SK_KG; ++q) fb[q] = fbn[q];
    }
  }

  // ---- the two K halves meet, lower half first (C: col = li, row = (r & 3) + 8 (r >> 2) + 4 lh)
  if (kh) {
#pragma unroll
    for (int r = 0; r < 16; ++r) fold[(ct * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (!kh && col_ok) {
    if constexpr (ACT >= 0) {
      const float bv = a.bias[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = row0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < a.M) a.C[m * a.N + col] = act_fwd_t<ACT>((acc[r] + fold[(ct * 16 + r) * 64 + lane]) + bv);
      }
    } else {
      float* pt = a.P + (int64_t)s * a.M * a.N;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = row0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < a.M) pt[m * a.N + col] = acc[r] + fold[(ct * 16 + r) * 64 + lane];
      }
    }
  }
}

// C[i] = act((((P[0][i] + P[1][i]) + ...) + P[S - 1][i]) + bias[i % N]); thread t owns the elements 4 t .. 4 t + 3 (N % 4 == 0: one row)
template <int ACT>
__global__ __launch_bounds__(64) void k_gemm_sk_finish(const float* __restrict__ P, const float* __restrict__ bias, float* __restrict__ C,
                                                      int64_t MN, int N, int S, int vec) {
  const int64_t i = ((int64_t)blockIdx.x * 64 + threadIdx.x) * 4;
  if (i >= MN) return;
  const int n = (int)(i % N);
  if (vec) {
    float4 v = *reinterpret_cast<const float4*>(P + i);
#pragma unroll 8
    for (int s = 1; s < S; ++s) {
      const float4 p = *reinterpret_cast<const float4*>(P + (int64_t)s * MN + i);
      v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    const float4 b = *reinterpret_cast<const float4*>(bias + n);
    *reinterpret_cast<float4*>(C + i) = make_float4(act_fwd_t<ACT>(v.x + b.x), act_fwd_t<ACT>(v.y + b.y), act_fwd_t<ACT>(v.z + b.z),
                                                    act_fwd_t<ACT>(v.w + b.w));
  } else {
    for (int e = 0; e < 4; ++e) {
      float v = P[i + e];
#pragma unroll 8
      for (int s = 1; s < S; ++s) v += P[(int64_t)s * MN + i + e];
      C[i + e] = act_fwd_t<ACT>(v + bias[n + e]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
// The slice count, a function of M, N, K and the CU count only (forced == 0), as choose_mc is: as many slices as bring the grid
// close to one workgroup per CU and no further, none shorter than SK_MIN_GROUPS groups, at most SK_MAX_SLICES, and S M N floats
// within SK_PARTIAL_CAP.  forced = 1 .. 64 replaces the first bound only.
int gemm_sk_slices(int64_t M, int N, int K, int num_cus, int forced) {
  const int64_t tiles = (int64_t)div_up(M, SK_TM) * div_up(N, SK_TN);
  int64_t S = forced > 0 ? forced : num_cus / tiles;
  const int G = K / 16;
  if (S > G / SK_MIN_GROUPS) S = G / SK_MIN_GROUPS;
  if (S > SK_MAX_SLICES) S = SK_MAX_SLICES;
  while (S > 1 && (size_t)S * M * N * sizeof(float) > SK_PARTIAL_CAP) --S;
  return S < 1 ? 1 : (int)S;
}

static size_t sk_lds_bytes(int ldsw) { return ((size_t)SK_TM * (ldsw + 1) + SK_FOLD) * sizeof(float); }

template <int ACT>
static int sk_launch(rlx_ctx* ctx, const SkArgs& a, double flops, double bytes, hipStream_t st) {
  static AttrOnce once;
  if (!once.done()) {
    RLX_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gemm_sk<ACT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)sk_lds_bytes(SK_STAGE)));
    once.mark();
  }
  ProfScope prof(ctx, PK_GEMM_SK, flops, st, bytes, a.M, a.N, a.K);
  RLX_PLAUNCH(k_gemm_sk<ACT>, dim3(div_up(a.M, SK_TM), div_up(a.N, SK_TN), a.S), dim3(256), sk_lds_bytes(a.ldsw), st, a);
  RLX_LAUNCH_CHECK();
  ++ctx->gemm_sk_launches;
  return RLX_OK;
}

#define RLX_SK_ACT_SWITCH(ACTV, CALL)                \
  switch (ACTV) {                                    \
    case RLX_ACT_TANH: return CALL(RLX_ACT_TANH);    \
    case RLX_ACT_ELU: return CALL(RLX_ACT_ELU);      \
    case RLX_ACT_RELU: return CALL(RLX_ACT_RELU);    \
    default: return CALL(RLX_ACT_NONE);              \
  }

template <int ACT>
static int sk_finish(const SkArgs& a, hipStream_t st) {
  const int64_t MN = a.M * a.N;
  const int vec = ((reinterpret_cast<uintptr_t>(a.C) | reinterpret_cast<uintptr_t>(a.bias)) & 15) == 0;
  hipLaunchKernelGGL(k_gemm_sk_finish<ACT>, dim3(div_up(MN / 4, 64)), dim3(64), 0, st, a.P, a.bias, a.C, MN, a.N, a.S, vec);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int launch_gemm_fwd_sk(rlx_ctx* ctx, const float* A, const float* W, const float* bias, float* C, int64_t M, int N, int K, int act,
                       hipStream_t st, int lda, int slices) {
  RLX_REQUIRE(M >= 1 && M <= GEMM_SK_MAX_M, RLX_EUNSUP, "launch_gemm_fwd_sk: M must be 1 .. 1024");
  RLX_REQUIRE(N >= 4 && N % 4 == 0, RLX_EUNSUP, "launch_gemm_fwd_sk: N must be a multiple of 4");
  RLX_REQUIRE(K >= 4 && K % 4 == 0, RLX_EUNSUP, "launch_gemm_fwd_sk: K must be a multiple of 4");
  RLX_REQUIRE(lda == 0 || (lda % 4 == 0 && lda >= K), RLX_EUNSUP, "launch_gemm_fwd_sk: lda must be 0 or a multiple of 4 that is >= K");
  RLX_REQUIRE(slices >= 0 && slices <= SK_MAX_SLICES, RLX_EINVAL, "launch_gemm_fwd_sk: slices must be 0 .. 64");
  SkArgs a{};
  a.A = A; a.W = W; a.bias = bias; a.C = C; a.M = M; a.N = N; a.K = K; a.lda = lda > 0 ? lda : K;
  a.G = K / 16;
  a.S = gemm_sk_slices(M, N, K, ctx->num_cus, slices);
  // the longest slice: one of the G % S longer ones, or the last with the tail
  const int base = a.G / a.S, longer = 16 * (base + (a.G % a.S ? 1 : 0)), last = 16 * base + (K - 16 * a.G);
  const int longest = longer > last ? longer : last;
  a.ldsw = longest >= SK_STAGE ? SK_STAGE : ((longest + 31) & ~31);
  a.vec_a = (reinterpret_cast<uintptr_t>(A) & 15) == 0;
  const double flops = 2.0 * (double)M * N * K, bytes = gemm_bytes(M, N, K);
  if (a.S == 1) {
#define RLX_SK_DIRECT(ACT) sk_launch<ACT>(ctx, a, flops, bytes, st)
    RLX_SK_ACT_SWITCH(act, RLX_SK_DIRECT)
#undef RLX_SK_DIRECT
  }
  a.P = (float*)scratch(ctx, SL_GEMM_SK, (size_t)a.S * M * N * sizeof(float));
  if (!a.P) return RLX_ENOMEM;
  const int rc = sk_launch<-1>(ctx, a, flops, bytes + 8.0 * a.S * (double)M * N, st);      // (P written, then read)
  if (rc) return rc;
#define RLX_SK_FINISH(ACT) sk_finish<ACT>(a, st)
  RLX_SK_ACT_SWITCH(act, RLX_SK_FINISH)
#undef RLX_SK_FINISH
}

}  // namespace rlx
