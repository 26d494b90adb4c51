// ssm.hip -- the memory of the reference's ppo_mamba2 policy (rl_x/algorithms/ppo_mamba2/flax_full_jit/policy.py:40-175): the depthwise
// causal convolution with its episode reset, the selective diagonal state-space scan with the z gate, forward and backward, and the
// entry points rlx_ssm_conv_f32, rlx_ssm_scan_f32 and rlx_mamba2_f32 (the block stack, mamba2_block.h).  float32 throughout, accurate
// expf / log1pf, every sum in a fixed order, no atomics: identical calls give identical bits.
//
// r_t = 0 iff t > 0 and done[s, t - 1]: the state (scan) and the window (conv) entering token t are zeroed.  Token 0 is never reset.
//
// Conv: a lane owns (sequence, channel, 32-token chunk) and walks its tokens with a K-deep register window; the chunk warms the window
// up over the K - 1 tokens in front of it (conv0 where those lie in front of the sequence), resets included.  64 consecutive channels
// of a token are one 256-byte row segment of proj (row stride 2 I).  The backward recomputes u1 on the same walk, keeps the K pending
// input gradients of the window's positions next to it (a reset retires them), runs K - 1 tokens past its chunk for the gradients
// that arrive from there, and leaves d conv_w / d conv_b as one partial row per (sequence, chunk).
//
// Scan: a workgroup owns (sequence, 64-channel slab), a lane one channel with its N states in registers, and the waves of the
// workgroup are consecutive time chunks (multiples of 16 tokens).  h_t = a_t r_t h_{t-1} + b_t is linear in h: each wave but the
// last scans its chunk from a zero state and keeps the product of a_t r_t (a reset makes it 0), the N end states and N products per
// lane go through LDS, after one barrier every wave folds the chunks in front of it in chunk order, then rescans its chunk from
// that state and emits g -- the emitted values follow the sequential order of operations.  The per-lane operands of 8 tokens
// (dt_raw, u, z) are requested together, one group ahead of the arithmetic; B_t | C_t and the done flags of the group are loaded
// once per wave (one element per lane) and reach the arithmetic through v_readlane.  The state entering every 16th token is stored.
// Backward: the same split.  The carry of d h is linear too (q_{t-1} = a_t r_t (C_t dy_t + q_t)): each wave but the first runs it
// over its chunk from zero (no states needed), the fold runs from the last chunk down.  Then per 16-token chunk, from the last: the
// states of 8 tokens are rebuilt from the checkpoint into registers (the later 8 first, after advancing over the earlier 8), and
// walked in reverse; h_{t-1} is never reconstructed by division.  dB_t / dC_t are sums over channels: a reduce-scatter over the wave
// (2 N values in 2 N shuffles), then a fixed-order sum over the slabs (k_ssm_bc_finish; at I == 64 straight into d xp).
// d A_log, d D, d dt_bias are accumulated per lane, summed over the workgroup's waves in wave order through LDS, and leave as one
// partial row per sequence for the slab reduction (stage_reduce).
#include "mamba2_block.h"

namespace rlx {

constexpr int SSM_G = 8;   // tokens per operand group of the scan kernels

__device__ __forceinline__ float ssm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float ssm_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // (d/dx: sigmoid(x), 1 in fp32 above 20)

// ------------------------------------------------------------------------------------------------------------------ conv
struct ConvArgs {
  const float* proj; const uint8_t* done; const float* conv0; const float* w; const float* b;
  float* u; float* convT;
  const float *du, *du2; float* dproj; float* part;   // backward
  int64_t c0_ss, cT_ss;
  int T, I, ldp, nch, nslab;
  int64_t waves;
};

template <int K, bool BWD>
__global__ __launch_bounds__(256) void k_ssm_conv(const ConvArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= a.waves) return;
  const int slab = (int)(gw % a.nslab), c = (int)((gw / a.nslab) % a.nch);
  const int64_t s = gw / ((int64_t)a.nslab * a.nch), row0 = s * a.T;
  const int i = slab * 64 + lane, T = a.T;
  const int t0 = c * SSM_CONV_TC, t1 = min(T, t0 + SSM_CONV_TC), tend = BWD ? min(T, t1 + K - 1) : t1;
  float wk[K], win[K], pend[K], live[K], dw[K];
  float db = 0.f;
  const float bias = a.b[i];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    wk[k] = a.w[k * a.I + i];
    win[k] = pend[k] = live[k] = dw[k] = 0.f;
  }
  const uint8_t* dn = a.done + row0;
#pragma unroll 4
  for (int tau = t0 - (K - 1); tau < tend; ++tau) {
    if (tau > 0 && dn[tau - 1]) {
#pragma unroll
      for (int k = 0; k < K; ++k) win[k] = live[k] = 0.f;
    }
    const float v = tau >= 0 ? a.proj[(row0 + tau) * a.ldp + i] : (a.conv0 ? a.conv0[s * a.c0_ss + (int64_t)(tau + K - 1) * a.I + i] : 0.f);
#pragma unroll
    for (int k = 0; k + 1 < K; ++k) {
      win[k] = win[k + 1];
      pend[k] = pend[k + 1];
      live[k] = live[k + 1];
    }
    win[K - 1] = v;
    pend[K - 1] = 0.f;
    live[K - 1] = 1.f;
    if (tau >= t0) {
      float u1 = bias;
#pragma unroll
      for (int k = 0; k < K; ++k) u1 += wk[k] * win[k];
      const float sg = ssm_sigmoid(u1);
      if (!BWD) a.u[(row0 + tau) * a.I + i] = u1 * sg;
      else {
        float g = a.du[(row0 + tau) * a.I + i];
        if (a.du2) g += a.du2[(row0 + tau) * a.I + i];
        const float du1 = g * (sg * (1.f + u1 * (1.f - sg)));
        if (tau < t1) {
          db += du1;
#pragma unroll
          for (int k = 0; k < K; ++k) dw[k] += du1 * win[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) pend[k] += live[k] * wk[k] * du1;
      }
    }
    if (BWD) {      // position tau - (K - 1) leaves the window with the next token: its gradient is complete
      const int pos = tau - (K - 1);
      if (pos >= t0 && pos < t1) a.dproj[(row0 + pos) * a.ldp + i] = pend[0];
    }
  }
  if (BWD) {
#pragma unroll
    for (int k = 1; k < K; ++k) {
      const int pos = tend - K + k;
      if (pos >= t0 && pos < t1) a.dproj[(row0 + pos) * a.ldp + i] = pend[k];
    }
    float* pr = a.part + (s * a.nch + c) * (int64_t)(K + 1) * a.I;
#pragma unroll
    for (int k = 0; k < K; ++k) pr[k * a.I + i] = dw[k];
    pr[K * a.I + i] = db;
  } else if (a.convT && t1 == T) {      // the window after token T - 1 (not reset by done[T - 1]: the caller's)
#pragma unroll
    for (int k = 1; k < K; ++k) a.convT[s * a.cT_ss + (int64_t)(k - 1) * a.I + i] = win[k];
  }
}

// ------------------------------------------------------------------------------------------------------------------ scan
struct ScanArgs {
  const float *u, *xp, *proj; const uint8_t* done; const float* h0; const float *dt_bias, *A_log, *D;
  float *g, *hT, *ckpt;
  const float* dg; float *du, *dxp, *dproj, *bc, *part;   // backward
  int64_t h0_ss, hT_ss, bc_ld, bc_slab;
  int T, I, nck, Lw, nslab;
};

// the operands of 8 tokens: per lane dt_raw, u (z, d g where wanted), and per wave B | C (element l of the group's 16 N floats in lane
// l of bc[l / 64]) and the done flag in front of token j in lane j.  Tokens past T - 1 repeat the last row: loaded, never used.
template <int N, bool Z, bool DG>
struct ScanGroup {
  static constexpr int NL = SSM_G * 2 * N / 64;
  float d[SSM_G], u[SSM_G], z[SSM_G], dg[SSM_G], bc[NL];
  int dn;
  __device__ __forceinline__ void load(const ScanArgs& a, int64_t row0, int tg, int i, int lane) {
    const int T = a.T, X = a.I + 2 * N;
#pragma unroll
    for (int j = 0; j < SSM_G; ++j) {
      const int64_t row = row0 + min(tg + j, T - 1);
      d[j] = a.xp[row * X + i];
      u[j] = a.u[row * a.I + i];
      if (Z) z[j] = a.proj[row * 2 * a.I + a.I + i];
      if (DG) dg[j] = a.dg[row * a.I + i];
    }
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int idx = q * 64 + lane;
      bc[q] = a.xp[(row0 + min(tg + idx / (2 * N), T - 1)) * X + a.I + idx % (2 * N)];
    }
    const int tp = tg + (lane & 7) - 1;
    dn = tp >= 0 && tp < T ? (int)a.done[row0 + tp] : 0;
  }
  __device__ __forceinline__ float B(int j, int n) const { return bcast(j * 2 * N + n); }
  __device__ __forceinline__ float C(int j, int n) const { return bcast(j * 2 * N + N + n); }
  __device__ __forceinline__ bool reset(int j) const { return __builtin_amdgcn_readlane(dn, j) != 0; }
  __device__ __forceinline__ float bcast(int e) const { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bc[e / 64]), e % 64)); }
};

template <int N>
__device__ __forceinline__ void ssm_load_state(const float* p, float (&h)[N]) {
#pragma unroll
  for (int n = 0; n < N; n += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + n);
    h[n] = v.x; h[n + 1] = v.y; h[n + 2] = v.z; h[n + 3] = v.w;
  }
}
template <int N>
__device__ __forceinline__ void ssm_store_state(float* p, const float (&h)[N]) {
#pragma unroll
  for (int n = 0; n < N; n += 4) *reinterpret_cast<float4*>(p + n) = make_float4(h[n], h[n + 1], h[n + 2], h[n + 3]);
}

// one token of the recurrence on a lane's N states; returns sum_n h_t[n] C_t[n]
template <int N, bool Z, bool DG>
__device__ __forceinline__ float ssm_step(const ScanGroup<N, Z, DG>& G, int j, const float (&A)[N], float dtb, float (&h)[N]) {
  const float delta = ssm_softplus(G.d[j] + dtb), du = delta * G.u[j];
  const bool rs = G.reset(j);
  float y = 0.f;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    h[n] = expf(delta * A[n]) * (rs ? 0.f : h[n]) + du * G.B(j, n);
    y += h[n] * G.C(j, n);
  }
  return y;
}

template <int N>
__global__ __launch_bounds__(512) void k_ssm_scan_fwd(const ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [waves - 1][E: N | P: N][64]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int slab = blockIdx.x % a.nslab, i = slab * 64 + lane, T = a.T;
  const int64_t s = blockIdx.x / a.nslab, row0 = s * T;
  const int ts = w * a.Lw, te = min(T, ts + a.Lw);
  float A[N], h[N];
  ssm_load_state<N>(a.A_log + (int64_t)i * N, A);
#pragma unroll
  for (int n = 0; n < N; ++n) A[n] = -expf(A[n]);
  const float dtb = a.dt_bias[i], Dp = a.D[i];
  if (nw > 1) {
    if (w < nw - 1) {      // the chunk from a zero state, and the product of a_t r_t over it
      float P[N];
#pragma unroll
      for (int n = 0; n < N; ++n) { h[n] = 0.f; P[n] = 1.f; }
      ScanGroup<N, false, false> G, Gn;
      if (ts < te) G.load(a, row0, ts, i, lane);
      for (int tg = ts; tg < te; tg += SSM_G) {
        if (tg + SSM_G < te) Gn.load(a, row0, tg + SSM_G, i, lane);
#pragma unroll
        for (int j = 0; j < SSM_G; ++j)
          if (tg + j < te) {
            const float delta = ssm_softplus(G.d[j] + dtb), du = delta * G.u[j];
            const bool rs = G.reset(j);
#pragma unroll
            for (int n = 0; n < N; ++n) {
              const float an = expf(delta * A[n]);
              h[n] = an * (rs ? 0.f : h[n]) + du * G.B(j, n);
              P[n] = rs ? 0.f : P[n] * an;
            }
          }
        G = Gn;
      }
#pragma unroll
      for (int n = 0; n < N; ++n) {
        lds[(w * 2 * N + n) * 64 + lane] = h[n];
        lds[(w * 2 * N + N + n) * 64 + lane] = P[n];
      }
    }
    __syncthreads();
  }
  if (ts >= te) return;
  if (a.h0) ssm_load_state<N>(a.h0 + s * a.h0_ss + (int64_t)i * N, h);
  else {
#pragma unroll
    for (int n = 0; n < N; ++n) h[n] = 0.f;
  }
  for (int c = 0; c < w; ++c) {      // the chunks in front of this one, in chunk order
#pragma unroll
    for (int n = 0; n < N; ++n) h[n] = lds[(c * 2 * N + N + n) * 64 + lane] * h[n] + lds[(c * 2 * N + n) * 64 + lane];
  }
  ScanGroup<N, true, false> G, Gn;
  G.load(a, row0, ts, i, lane);
  for (int tg = ts; tg < te; tg += SSM_G) {
    if (tg + SSM_G < te) Gn.load(a, row0, tg + SSM_G, i, lane);
    if (a.ckpt && tg % SSM_CK == 0) ssm_store_state<N>(a.ckpt + ((s * a.nck + tg / SSM_CK) * a.I + i) * N, h);
#pragma unroll
    for (int j = 0; j < SSM_G; ++j)
      if (tg + j < te) {
        const float y = ssm_step<N>(G, j, A, dtb, h) + Dp * G.u[j];
        a.g[(row0 + tg + j) * a.I + i] = y * (G.z[j] * ssm_sigmoid(G.z[j]));
      }
    G = Gn;
  }
  if (a.hT && te == T) ssm_store_state<N>(a.hT + s * a.hT_ss + (int64_t)i * N, h);
}

// v[0 .. CNT) of every lane -> the sum over the 64 lanes of v[e] in the lanes l with e(l) == e, in CNT + (6 - log2 CNT) shuffles: a
// step at distance off halves the values a lane still carries (the upper lanes keep the upper half).  e(l) is returned; every value
// sits in 64 / CNT lanes, those with (l & (64 / CNT - 1)) == 0 are its writers.  A fixed tree: the same bits every time.
template <int CNT>
__device__ __forceinline__ float ssm_reduce_scatter(float (&v)[CNT], int lane, int* e_out) {
  int e = 0, off = 32;
#pragma unroll
  for (int cnt = CNT; cnt > 1; cnt >>= 1, off >>= 1) {
    const int H = cnt >> 1;
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const float keep = up ? v[k + H] : v[k], send = up ? v[k] : v[k + H];
      v[k] = keep + __shfl_xor(send, off, 64);
    }
    e += up ? H : 0;
  }
#pragma unroll
  for (int o = 32 / CNT; o > 0; o >>= 1) v[0] += __shfl_xor(v[0], o, 64);
  *e_out = e;
  return v[0];
}

template <int N>
__global__ __launch_bounds__(256) void k_ssm_scan_bwd(const ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [waves - 1][E: N | P: N][64]; then [waves - 1][N + 2][64]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int slab = blockIdx.x % a.nslab, i = slab * 64 + lane, T = a.T, X = a.I + 2 * N;
  const int64_t s = blockIdx.x / a.nslab, row0 = s * T;
  const int ts = w * a.Lw, te = min(T, ts + a.Lw);
  float A[N], q[N], dA[N];
  ssm_load_state<N>(a.A_log + (int64_t)i * N, A);
#pragma unroll
  for (int n = 0; n < N; ++n) {
    A[n] = -expf(A[n]);
    q[n] = dA[n] = 0.f;
  }
  const float dtb = a.dt_bias[i], Dp = a.D[i];
  float dD = 0.f, ddtb = 0.f;
  if (nw > 1) {
    if (w > 0) {      // the carry of d h over the chunk from zero, and the product of a_t r_t
      float P[N];
#pragma unroll
      for (int n = 0; n < N; ++n) P[n] = 1.f;
      ScanGroup<N, true, true> G;
      for (int tg = ts + (te - 1 - ts) / SSM_G * SSM_G; tg >= ts && ts < te; tg -= SSM_G) {
        G.load(a, row0, tg, i, lane);
#pragma unroll
        for (int j = SSM_G - 1; j >= 0; --j)
          if (tg + j < te) {
            const float delta = ssm_softplus(G.d[j] + dtb), dy = G.dg[j] * (G.z[j] * ssm_sigmoid(G.z[j]));
            const bool rs = G.reset(j);
#pragma unroll
            for (int n = 0; n < N; ++n) {
              const float an = expf(delta * A[n]);
              q[n] = rs ? 0.f : an * (G.C(j, n) * dy + q[n]);
              P[n] = rs ? 0.f : P[n] * an;
            }
          }
      }
#pragma unroll
      for (int n = 0; n < N; ++n) {
        lds[((w - 1) * 2 * N + n) * 64 + lane] = q[n];
        lds[((w - 1) * 2 * N + N + n) * 64 + lane] = P[n];
        q[n] = 0.f;
      }
    }
    __syncthreads();
    for (int c = nw - 1; c > w; --c) {      // the chunks behind this one, from the last
#pragma unroll
      for (int n = 0; n < N; ++n) q[n] = lds[((c - 1) * 2 * N + N + n) * 64 + lane] * q[n] + lds[((c - 1) * 2 * N + n) * 64 + lane];
    }
  }
  float* bcp = a.bc + slab * a.bc_slab;
  for (int ck = (te - 1) / SSM_CK; ck * SSM_CK >= ts && ts < te; --ck) {
    float h0c[N], hs[SSM_G][N], hin[N];
    ssm_load_state<N>(a.ckpt + ((s * a.nck + ck) * a.I + i) * N, h0c);
#pragma unroll 1
    for (int sb = 1; sb >= 0; --sb) {      // the later 8 tokens first
      const int tb = ck * SSM_CK + sb * SSM_G;
      if (tb >= te) continue;
#pragma unroll
      for (int n = 0; n < N; ++n) hin[n] = h0c[n];
      if (sb) {      // advance over the earlier 8
        ScanGroup<N, false, false> Ga;
        Ga.load(a, row0, ck * SSM_CK, i, lane);
#pragma unroll
        for (int j = 0; j < SSM_G; ++j) {
          (void)ssm_step<N>(Ga, j, A, dtb, hin);
          __builtin_amdgcn_sched_barrier(0);      // (one token at a time: the scheduler otherwise interleaves all eight and spills)
        }
      }
      ScanGroup<N, true, true> G;
      G.load(a, row0, tb, i, lane);
#pragma unroll
      for (int j = 0; j < SSM_G; ++j) {      // (tokens past te - 1 repeat the last row: their states are not read)
#pragma unroll
        for (int n = 0; n < N; ++n) hs[j][n] = j ? hs[j - 1][n] : hin[n];
        (void)ssm_step<N>(G, j, A, dtb, hs[j]);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int j = SSM_G - 1; j >= 0; --j) {
        const int t = tb + j;
        if (t < te) {
        const float x = G.d[j] + dtb, delta = ssm_softplus(x), uu = G.u[j], z = G.z[j], sz = ssm_sigmoid(z);
        const bool rs = G.reset(j);
        float y = Dp * uu;
#pragma unroll
        for (int n = 0; n < N; ++n) y += hs[j][n] * G.C(j, n);
        const float dy = G.dg[j] * (z * sz);
        float du = dy * Dp, dde = 0.f, red[2 * N];
#pragma unroll
        for (int n = 0; n < N; ++n) {
          const float hp = rs ? 0.f : (j ? hs[j - 1][n] : hin[n]);
          const float Dn = G.C(j, n) * dy + q[n], an = expf(delta * A[n]), t1 = Dn * delta, Bn = G.B(j, n);
          red[n] = t1 * uu;              // d B_t[n], this channel's part
          red[N + n] = dy * hs[j][n];    // d C_t[n]
          du += t1 * Bn;
          dde += Dn * (an * A[n] * hp + Bn * uu);
          dA[n] += t1 * an * hp;
          q[n] = rs ? 0.f : an * Dn;
        }
        dD += dy * uu;
        const float ddt = dde * ssm_sigmoid(x);
        ddtb += ddt;
        const int64_t row = row0 + t;
        a.du[row * a.I + i] = du;
        a.dxp[row * X + i] = ddt;
        a.dproj[row * 2 * a.I + a.I + i] = G.dg[j] * y * (sz * (1.f + z * (1.f - sz)));
        int e;
        const float sum = ssm_reduce_scatter<2 * N>(red, lane, &e);
        if ((lane & (64 / (2 * N) - 1)) == 0) bcp[row * a.bc_ld + e] = sum;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // d dt_bias, d D, d A_log of the workgroup: waves 1 .. nw - 1 through LDS, summed by wave 0 in wave order
  if (nw > 1) {
    __syncthreads();
    if (w > 0) {
      float* o = lds + (w - 1) * (N + 2) * 64 + lane;
      o[0] = ddtb;
      o[64] = dD;
#pragma unroll
      for (int n = 0; n < N; ++n) o[(2 + n) * 64] = dA[n];
    }
    __syncthreads();
    if (w > 0) return;
    for (int c = 1; c < nw; ++c) {
      const float* o = lds + (c - 1) * (N + 2) * 64 + lane;
      ddtb += o[0];
      dD += o[64];
#pragma unroll
      for (int n = 0; n < N; ++n) dA[n] += o[(2 + n) * 64];
    }
  }
  float* pr = a.part + s * (int64_t)(N + 2) * a.I;
  pr[i] = ddtb;
  pr[a.I + i] = dD;
#pragma unroll
  for (int n = 0; n < N; ++n) dA[n] *= A[n];      // A = -exp(A_log): dA / dA_log = A
  ssm_store_state<N>(pr + 2 * a.I + (int64_t)i * N, dA);
}

// d xp[row, I + e] = sum over the slabs of bc[slab][row][e], in slab order
__global__ __launch_bounds__(256) void k_ssm_bc_finish(const float* __restrict__ bc, float* __restrict__ dxp, int64_t M, int n2, int nslab, int X) {
  const int64_t n = M * n2;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
    float v = bc[k];
    for (int sl = 1; sl < nslab; ++sl) v += bc[sl * n + k];
    dxp[(k / n2) * X + (X - n2) + k % n2] = v;
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
int ssm_check(const char* who, int64_t S, int64_t T, int I, int N, int K) {
  const std::string w(who);
  RLX_REQUIRE(I >= 64 && I % 64 == 0 && I <= 1024, RLX_EUNSUP, w + ": I (d_model * expand) must be a multiple of 64 up to 1024");
  RLX_REQUIRE(N == 4 || N == 8 || N == 16, RLX_EUNSUP, w + ": N (state_dim) must be 4, 8 or 16");
  RLX_REQUIRE(K >= 1 && K <= 4, RLX_EUNSUP, w + ": K (conv_kernel) must be 1..4");
  RLX_REQUIRE(T >= 1, RLX_EUNSUP, w + ": T must be at least 1");
  RLX_REQUIRE(S >= 1, RLX_EUNSUP, w + ": S must be at least 1");
  RLX_REQUIRE(T <= (1 << 20) && S * ((T + SSM_CONV_TC - 1) / SSM_CONV_TC) * (I / 64) <= 0x7fffffffLL, RLX_EUNSUP,
              w + ": S * ceil(T / 32) * I / 64 must fit the grid (and T <= 2^20)");
  return RLX_OK;
}

template <bool BWD>
static int conv_launch(const ConvArgs& a, int K, hipStream_t st) {
  const dim3 grid((unsigned)div_up(a.waves, 4)), block(256);
  if (K == 1) hipLaunchKernelGGL((k_ssm_conv<1, BWD>), grid, block, 0, st, a);
  else if (K == 2) hipLaunchKernelGGL((k_ssm_conv<2, BWD>), grid, block, 0, st, a);
  else if (K == 3) hipLaunchKernelGGL((k_ssm_conv<3, BWD>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_ssm_conv<4, BWD>), grid, block, 0, st, a);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
static ConvArgs conv_args(const float* proj, int ldp, const uint8_t* done, const float* conv0, int64_t c0_ss, const float* w, const float* b,
                          int64_t S, int T, int I) {
  ConvArgs a{};
  a.proj = proj; a.done = done; a.conv0 = conv0; a.w = w; a.b = b; a.c0_ss = c0_ss;
  a.T = T; a.I = I; a.ldp = ldp; a.nch = ssm_conv_chunks(T); a.nslab = I / 64;
  a.waves = S * a.nch * a.nslab;
  return a;
}
int ssm_conv_fwd(const float* proj, int ldp, const uint8_t* done, const float* conv0, int64_t c0_ss, const float* conv_w, const float* conv_b,
                 int64_t S, int T, int I, int K, float* u, float* convT, int64_t cT_ss, hipStream_t st) {
  ConvArgs a = conv_args(proj, ldp, done, conv0, c0_ss, conv_w, conv_b, S, T, I);
  a.u = u; a.convT = convT; a.cT_ss = cT_ss;
  return conv_launch<false>(a, K, st);
}
int ssm_conv_bwd(rlx_ctx* ctx, const float* proj, int ldp, const uint8_t* done, const float* conv0, int64_t c0_ss, const float* conv_w,
                 const float* conv_b, int64_t S, int T, int I, int K, const float* d_u, const float* d_u2, float* d_proj, float* g_w, float* g_b,
                 hipStream_t st) {
  ConvArgs a = conv_args(proj, ldp, done, conv0, c0_ss, conv_w, conv_b, S, T, I);
  const int rows = (int)(S * a.nch);
  const int64_t width = (int64_t)(K + 1) * I;
  a.du = d_u; a.du2 = d_u2; a.dproj = d_proj;
  a.part = stage_alloc(ctx, (size_t)rows * width);
  if (!a.part) return RLX_ENOMEM;
  const int rc = conv_launch<true>(a, K, st);
  if (rc) return rc;
  ReduceTable tab;
  tab.n = 0;
  tab.seg[tab.n++] = ReduceSeg{a.part, g_w, (int64_t)K * I, width, rows, 0, 1.f, 0.f, 1};
  tab.seg[tab.n++] = ReduceSeg{a.part + (int64_t)K * I, g_b, (int64_t)I, width, rows, 0, 1.f, 0.f, 1};
  return stage_reduce(ctx, tab, nullptr, nullptr, st);
}

// waves per workgroup and tokens per wave: chunks are whole 16-token blocks, and no wave is left without one
static int scan_split(int T, int n_chunks, int max_waves, int* Lw) {
  int nw = n_chunks > 0 ? n_chunks : SSM_DEFAULT_CHUNKS;
  nw = nw < max_waves ? nw : max_waves;
  const int nck = ssm_nck(T), per = div_up(nck, nw);
  *Lw = per * SSM_CK;
  return div_up(nck, per);
}
static ScanArgs scan_args(const float* u, const float* xp, const float* proj, const uint8_t* done, const float* h0, int64_t h0_ss,
                          const float* dt_bias, const float* A_log, const float* D, int T, int I) {
  ScanArgs a{};
  a.u = u; a.xp = xp; a.proj = proj; a.done = done; a.h0 = h0; a.h0_ss = h0_ss; a.dt_bias = dt_bias; a.A_log = A_log; a.D = D;
  a.T = T; a.I = I; a.nck = ssm_nck(T); a.nslab = I / 64;
  return a;
}
int ssm_scan_fwd(const float* u, const float* xp, const float* proj, const uint8_t* done, const float* h0, int64_t h0_ss, const float* dt_bias,
                 const float* A_log, const float* D, int64_t S, int T, int I, int N, float* g, float* hT, int64_t hT_ss, float* ckpt,
                 int n_chunks, hipStream_t st) {
  ScanArgs a = scan_args(u, xp, proj, done, h0, h0_ss, dt_bias, A_log, D, T, I);
  a.g = g; a.hT = hT; a.hT_ss = hT_ss; a.ckpt = ckpt;
  const int nw = scan_split(T, n_chunks, 8, &a.Lw);
  const dim3 grid((unsigned)(S * a.nslab)), block(64 * nw);
  const size_t lds = (size_t)(nw - 1) * 2 * N * 64 * sizeof(float);
  if (N == 4) hipLaunchKernelGGL(k_ssm_scan_fwd<4>, grid, block, lds, st, a);
  else if (N == 8) hipLaunchKernelGGL(k_ssm_scan_fwd<8>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(k_ssm_scan_fwd<16>, grid, block, lds, st, a);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}
int ssm_scan_bwd(rlx_ctx* ctx, const float* u, const float* xp, const float* proj, const uint8_t* done, const float* h0, int64_t h0_ss,
                 const float* dt_bias, const float* A_log, const float* D, int64_t S, int T, int I, int N, const float* ckpt, const float* d_g,
                 float* d_u, float* d_xp, float* d_proj, float* bc, float* g_dt_bias, float* g_A_log, float* g_D, int n_chunks, hipStream_t st) {
  ScanArgs a = scan_args(u, xp, proj, done, h0, h0_ss, dt_bias, A_log, D, T, I);
  const int64_t M = S * T, width = (int64_t)(N + 2) * I;
  a.ckpt = const_cast<float*>(ckpt); a.dg = d_g; a.du = d_u; a.dxp = d_xp; a.dproj = d_proj;
  if (a.nslab == 1) { a.bc = d_xp + I; a.bc_ld = I + 2 * N; a.bc_slab = 0; }      // one slab: the sums over channels are complete
  else { a.bc = bc; a.bc_ld = 2 * N; a.bc_slab = M * 2 * N; }
  a.part = stage_alloc(ctx, (size_t)S * width);
  if (!a.part) return RLX_ENOMEM;
  const int nw = scan_split(T, n_chunks, 4, &a.Lw);      // (at most 256 threads: a wave holds 8 x N states and needs more than 256 registers)
  const dim3 grid((unsigned)(S * a.nslab)), block(64 * nw);
  const size_t lds = (size_t)(nw - 1) * 2 * N * 64 * sizeof(float);
  if (N == 4) hipLaunchKernelGGL(k_ssm_scan_bwd<4>, grid, block, lds, st, a);
  else if (N == 8) hipLaunchKernelGGL(k_ssm_scan_bwd<8>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(k_ssm_scan_bwd<16>, grid, block, lds, st, a);
  RLX_LAUNCH_CHECK();
  if (a.nslab > 1) {
    hipLaunchKernelGGL(k_ssm_bc_finish, dim3(elem_grid(M * 2 * N)), dim3(256), 0, st, bc, d_xp, M, 2 * N, a.nslab, I + 2 * N);
    RLX_LAUNCH_CHECK();
  }
  ReduceTable tab;
  tab.n = 0;
  tab.seg[tab.n++] = ReduceSeg{a.part, g_dt_bias, (int64_t)I, width, (int)S, 0, 1.f, 0.f, 1};
  tab.seg[tab.n++] = ReduceSeg{a.part + I, g_D, (int64_t)I, width, (int)S, 0, 1.f, 0.f, 1};
  tab.seg[tab.n++] = ReduceSeg{a.part + 2 * I, g_A_log, (int64_t)I * N, width, (int)S, 0, 1.f, 0.f, 1};
  return stage_reduce(ctx, tab, nullptr, nullptr, st);
}

static bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t m = 0;
  for (const void* p : ps) m |= (uintptr_t)p;
  return (m & 15) == 0;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int rlx_ssm_conv_f32(rlx_ctx* ctx, const float* proj, const uint8_t* done, const float* conv0, const float* conv_w, const float* conv_b,
                     int64_t S, int64_t T, int I, int K, float* u, float* convT, const float* d_u, float* d_proj, float* d_conv_w,
                     float* d_conv_b, void* stream) {
  const int rc = ssm_check("rlx_ssm_conv_f32", S, T, I, 8, K);      // (first: an empty sequence has no rows to point at)
  if (rc) return rc;
  RLX_REQUIRE(ctx && proj && done && conv_w && conv_b && u, RLX_EINVAL, "rlx_ssm_conv_f32: NULL pointer (ctx, proj, done, conv_w, conv_b, u)");
  RLX_REQUIRE(!d_u || (d_proj && d_conv_w && d_conv_b), RLX_EINVAL, "rlx_ssm_conv_f32: a backward (d_u) needs d_proj, d_conv_w and d_conv_b");
  RLX_REQUIRE(aligned16({proj, conv0, u, convT, d_u, d_proj}), RLX_EINVAL,
              "rlx_ssm_conv_f32: proj, conv0, u, convT, d_u and d_proj must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t c_ss = (int64_t)(K - 1) * I;
  const int rf = ssm_conv_fwd(proj, 2 * I, done, K > 1 ? conv0 : nullptr, c_ss, conv_w, conv_b, S, (int)T, I, K, u, K > 1 ? convT : nullptr, c_ss, st);
  if (rf || !d_u) return rf;
  return ssm_conv_bwd(ctx, proj, 2 * I, done, K > 1 ? conv0 : nullptr, c_ss, conv_w, conv_b, S, (int)T, I, K, d_u, nullptr, d_proj, d_conv_w,
                      d_conv_b, st);
}

int rlx_ssm_scan_f32(rlx_ctx* ctx, const float* u, const float* xp, const float* proj, const uint8_t* done, const float* h0,
                     const float* dt_bias, const float* A_log, const float* D, int64_t S, int64_t T, int I, int N, float* g, float* hT,
                     const float* d_g, float* d_u, float* d_xp, float* d_proj, float* d_dt_bias, float* d_A_log, float* d_D, int n_chunks,
                     void* stream) {
  const int rc = ssm_check("rlx_ssm_scan_f32", S, T, I, N, 1);
  if (rc) return rc;
  RLX_REQUIRE(ctx && u && xp && proj && done && dt_bias && A_log && D && g, RLX_EINVAL,
              "rlx_ssm_scan_f32: NULL pointer (ctx, u, xp, proj, done, dt_bias, A_log, D, g)");
  RLX_REQUIRE(!d_g || (d_u && d_xp && d_proj && d_dt_bias && d_A_log && d_D), RLX_EINVAL,
              "rlx_ssm_scan_f32: a backward (d_g) needs d_u, d_xp, d_proj, d_dt_bias, d_A_log and d_D");
  RLX_REQUIRE(n_chunks == 0 || n_chunks == 1 || n_chunks == 2 || n_chunks == 4 || n_chunks == 8, RLX_EUNSUP,
              "rlx_ssm_scan_f32: n_chunks must be 0 (the default), 1, 2, 4 or 8");
  RLX_REQUIRE(aligned16({u, xp, proj, h0, A_log, g, hT, d_g, d_u, d_xp, d_proj, d_A_log}), RLX_EINVAL,
              "rlx_ssm_scan_f32: u, xp, proj, h0, A_log, g, hT, d_g, d_u, d_xp, d_proj and d_A_log must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const bool bwd = d_g != nullptr;
  const int64_t M = S * T, h_ss = (int64_t)I * N;
  float *ckpt = nullptr, *bc = nullptr;
  if (bwd) {
    const int rca = arena_carve(ctx, SL_SSM, [&](Arena& a) {
      ckpt = a.take((size_t)S * ssm_nck((int)T) * I * N);
      bc = I > 64 ? a.take((size_t)(I / 64) * M * 2 * N) : nullptr;
    });
    if (rca) return rca;
  }
  const int rf = ssm_scan_fwd(u, xp, proj, done, h0, h_ss, dt_bias, A_log, D, S, (int)T, I, N, g, hT, h_ss, ckpt, n_chunks, st);
  if (rf || !bwd) return rf;
  return ssm_scan_bwd(ctx, u, xp, proj, done, h0, h_ss, dt_bias, A_log, D, S, (int)T, I, N, ckpt, d_g, d_u, d_xp, d_proj, bc, d_dt_bias,
                      d_A_log, d_D, n_chunks, st);
}

int64_t rlx_mamba2_param_count(const rlx_mamba2_desc* desc) {
  if (!desc || desc->n_layers < 1 || desc->n_layers > M2_MAX_LAYERS || desc->d_model < 1 || desc->expand < 1 || desc->state_dim < 1 ||
      desc->conv_kernel < 1)
    return -1;
  return make_mamba2(*desc).n_params;
}

int rlx_mamba2_f32(rlx_ctx* ctx, const rlx_mamba2_desc* desc, const float* params, const float* x, const uint8_t* done, const float* h0,
                   const float* conv0, int64_t S, int64_t T, float* out, float* hT, float* convT, const float* d_out, float* grads, float* dx,
                   void* stream) {
  RLX_REQUIRE(ctx && desc && params && x && done && out, RLX_EINVAL, "rlx_mamba2_f32: NULL pointer (ctx, desc, params, x, done, out)");
  RLX_REQUIRE(!d_out || (grads && dx), RLX_EINVAL, "rlx_mamba2_f32: a backward (d_out) needs grads and dx");
  RLX_REQUIRE(desc->d_model >= 64 && desc->d_model % 64 == 0 && desc->d_model <= 512, RLX_EUNSUP,
              "rlx_mamba2_f32: d_model must be a multiple of 64 up to 512 (the row-norm kernels hold a row in one wave)");
  RLX_REQUIRE(desc->expand >= 1 && desc->expand <= 16, RLX_EUNSUP, "rlx_mamba2_f32: expand must be 1..16");
  RLX_REQUIRE(desc->n_layers >= 1 && desc->n_layers <= M2_MAX_LAYERS, RLX_EUNSUP, "rlx_mamba2_f32: n_layers must be 1..4");
  RLX_REQUIRE(desc->ln_eps > 0.f, RLX_EINVAL, "rlx_mamba2_f32: ln_eps must be positive");
  const Mamba2 E = make_mamba2(*desc);
  const int rc = ssm_check("rlx_mamba2_f32", S, T, E.I, E.N, E.K);
  if (rc) return rc;
  RLX_REQUIRE(S * T <= 0x7fffffffLL / 2048, RLX_EUNSUP, "rlx_mamba2_f32: S * T at most 2^20 rows");
  RLX_REQUIRE(aligned16({params, x, h0, conv0, out, hT, convT, d_out, grads, dx}), RLX_EINVAL,
              "rlx_mamba2_f32: params, x, h0, conv0, out, hT, convT, d_out, grads and dx must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t M = S * T;
  const bool bwd = d_out != nullptr;
  BxReleaseAll release{ctx};
  int rcx = mamba2_images(ctx, E, params, bwd, M, st);
  if (rcx) return rcx;
  M2Bufs B;
  rcx = arena_carve(ctx, SL_SSM, [&](Arena& a) { mamba2_carve(E, S, (int)T, bwd, a, &B); });
  if (rcx) return rcx;
  rcx = mamba2_fwd(ctx, E, params, x, done, h0, conv0, S, (int)T, B, out, hT, convT, st);
  if (rcx || !bwd) return rcx;
  return mamba2_bwd(ctx, E, params, x, done, h0, conv0, S, (int)T, B, d_out, grads, dx, st);
}

}  // extern "C"
