// mamba2_block.h -- the Mamba2 block stack on the host side (rl_x/algorithms/ppo_mamba2/flax_full_jit/policy.py:40-175: causal_conv_one_step,
// ssm_one_step, Mamba2Block.apply_one_step / forward_sequence), in tf_encoder.h's style: a descriptor of parameter offsets, the arena
// carve, and the forward and the backward as two functions (a policy puts its decode chain between them).  Per layer
//   ln -> in_proj GEMM [d, 2 I] (u0 | z) -> causal conv + SiLU (ssm.hip) -> x_proj GEMM [I, I + 2 N] (dt_raw | B | C) -> selective scan
//   with the z gate (ssm.hip) -> out_proj GEMM [I, d] -> + x
// FLAT PARAMETER LAYOUT (ABI), per layer, in this order:
//   ln scale [d], ln bias [d], W_in [d, 2 I], b_in [2 I], conv_w [K, I], conv_b [I], W_x [I, I + 2 N], b_x [I + 2 N], dt_bias [I],
//   A_log [I, N], D [I], W_out [I, d], b_out [d]
// GEMMs: launch_gemm_fwd / stage_dx / stage_dw as they are -- the exact engine below 4096 rows, the split-operand engine from 4096
// rows through net_images (mamba2_images).  The residual add rides on the next layer's LayerNorm (NormRes) and on tf_add at the end;
// backward, a LayerNorm's input gradient takes the gradient arriving over the residual branch as its last addend.
// u feeds both the scan and the x_proj GEMM: its two gradients are added by the conv's backward at the load, not by a kernel.
#pragma once
#include "tf_encoder.h"

namespace rlx {

constexpr int M2_MAX_LAYERS = 4;
constexpr int SSM_CK = 16;              // tokens between two checkpoints of the scan state
constexpr int SSM_CONV_TC = 32;         // tokens per time chunk of the conv kernels
constexpr int SSM_DEFAULT_CHUNKS = 1;   // time chunks (waves) per workgroup of the scan kernels: the fastest of 1 / 2 / 4 / 8 in tools/ssm_bench.py

// ---- ssm.hip.  Carries: conv0 / convT [S, K - 1, I] and h0 / hT [S, I, N] per sequence, `*_ss` floats from one sequence to the
// next (the block stack hands one layer of [S, L, ...] in); NULL carries in are zeros, NULL carries out are not written.
// RLX_EUNSUP, naming the field, outside I % 64 == 0 <= 1024, N in {4, 8, 16}, 1 <= K <= 4, T >= 1, S >= 1
int ssm_check(const char* who, int64_t S, int64_t T, int I, int N, int K);
static inline int ssm_nck(int T) { return (T + SSM_CK - 1) / SSM_CK; }
static inline int ssm_conv_chunks(int T) { return (T + SSM_CONV_TC - 1) / SSM_CONV_TC; }
// u = silu(conv(proj's u0 columns)) [S T, I]; proj at row stride ldp
int ssm_conv_fwd(const float* proj, int ldp, const uint8_t* done, const float* conv0, int64_t c0_ss, const float* conv_w, const float* conv_b,
                 int64_t S, int T, int I, int K, float* u, float* convT, int64_t cT_ss, hipStream_t st);
// d u (= d_u + d_u2 where d_u2 != NULL) -> d proj's u0 columns (row stride ldp), d conv_w [K, I], d conv_b [I]
int ssm_conv_bwd(rlx_ctx* ctx, const float* proj, int ldp, const uint8_t* done, const float* conv0, int64_t c0_ss, const float* conv_w,
                 const float* conv_b, int64_t S, int T, int I, int K, const float* d_u, const float* d_u2, float* d_proj, float* g_w, float* g_b,
                 hipStream_t st);
// g [S T, I] from u, xp [S T, I + 2 N], proj's z columns (row stride 2 I); ckpt (NULL: none) [S, ssm_nck(T), I, N] receives the state
// entering every 16th token; n_chunks: 0 the default, else 1 / 2 / 4 / 8
int ssm_scan_fwd(const float* u, const float* xp, const float* proj, const uint8_t* done, const float* h0, int64_t h0_ss, const float* dt_bias,
                 const float* A_log, const float* D, int64_t S, int T, int I, int N, float* g, float* hT, int64_t hT_ss, float* ckpt,
                 int n_chunks, hipStream_t st);
// d g -> d u, d xp, d proj's z columns, d dt_bias [I], d A_log [I, N], d D [I]; bc: [I / 64, S T, 2 N] floats of work space (unused
// at I == 64)
int ssm_scan_bwd(rlx_ctx* ctx, const float* u, const float* xp, const float* proj, const uint8_t* done, const float* h0, int64_t h0_ss,
                 const float* dt_bias, const float* A_log, const float* D, int64_t S, int T, int I, int N, const float* ckpt, const float* d_g,
                 float* d_u, float* d_xp, float* d_proj, float* bc, float* g_dt_bias, float* g_A_log, float* g_D, int n_chunks, hipStream_t st);

struct M2Layer { Block ln; int64_t W_in, b_in, conv_w, conv_b, W_x, b_x, dt_bias, A_log, D, W_out, b_out; };
struct Mamba2 { int d, I, N, K, n_layers; M2Layer layer[M2_MAX_LAYERS]; int64_t n_params; };

static inline Mamba2 make_mamba2(const rlx_mamba2_desc& t) {
  Mamba2 E{};
  E.d = t.d_model; E.I = t.d_model * t.expand; E.N = t.state_dim; E.K = t.conv_kernel; E.n_layers = t.n_layers;
  const int64_t d = E.d, I = E.I, N = E.N, K = E.K;
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += n; return o; };
  for (int l = 0; l < t.n_layers && l < M2_MAX_LAYERS; ++l) {
    M2Layer& L = E.layer[l];
    L.ln = Block{(int)d, (int)d, -1, -1, 0, 0, NORM_LAYER, RLX_ACT_NONE, t.ln_eps, 0.f};   // no Linear: norm_act reads out, g, be, norm, act, eps
    L.ln.g = take(d); L.ln.be = take(d);
    L.W_in = take(d * 2 * I); L.b_in = take(2 * I);
    L.conv_w = take(K * I); L.conv_b = take(I);
    L.W_x = take(I * (I + 2 * N)); L.b_x = take(I + 2 * N);
    L.dt_bias = take(I); L.A_log = take(I * N); L.D = take(I);
    L.W_out = take(I * d); L.b_out = take(d);
  }
  E.n_params = off;
  return E;
}

// Activations of one layer, kept for the backward.  A forward-only call gives every layer the first layer's set.
struct M2LayerBufs {
  float* xin;    // [M, d] the layer's input (layer 0: the caller's x, not carved)
  float* y;      // [M, d] ln(x); backward: d ln out, then d x
  float* proj;   // [M, 2 I] u0 | z
  float* u;      // [M, I]
  float* xp;     // [M, I + 2 N] dt_raw | B | C
  float* g;      // [M, I] gated scan output; backward: d g
  float* ckpt;   // [S, ceil(T / 16), I, N] (backward only)
};
struct M2Bufs {
  M2LayerBufs l[M2_MAX_LAYERS];
  float* branch;                         // [M, d] a block's output in front of its residual add
  float *dxp, *dproj, *du_s, *du_x, *bc; // backward: [M, I + 2 N], [M, 2 I], [M, I] (scan), [M, I] (x_proj), [I / 64, M, 2 N]
};
static inline void mamba2_carve(const Mamba2& E, int64_t S, int T, bool bwd, Arena& a, M2Bufs* B) {
  const size_t M = (size_t)S * T, d = E.d, I = E.I, X = E.I + 2 * E.N;
  for (int l = 0; l < E.n_layers; ++l) {
    M2LayerBufs& b = B->l[l];
    if (l > 0 && !bwd) {      // (xin: set below)
      b = B->l[0];
      continue;
    }
    b.xin = l ? a.take(M * d) : nullptr;
    b.y = a.take(M * d);
    b.proj = a.take(M * 2 * I);
    b.u = a.take(M * I);
    b.xp = a.take(M * X);
    b.g = a.take(M * I);
    b.ckpt = bwd ? a.take((size_t)S * ssm_nck(T) * I * E.N) : nullptr;
  }
  B->branch = a.take(M * d);
  B->dxp = bwd ? a.take(M * X) : nullptr;
  B->dproj = bwd ? a.take(M * 2 * I) : nullptr;
  B->du_s = bwd ? a.take(M * I) : nullptr;
  B->du_x = bwd ? a.take(M * I) : nullptr;
  B->bc = bwd && I > 64 ? a.take((I / 64) * M * 2 * E.N) : nullptr;
  if (!bwd) {   // forward only: a layer's input is dead once the next LayerNorm has formed its own, so one spare buffer serves l > 0
    float* spare = E.n_layers > 1 ? a.take(M * d) : nullptr;
    for (int l = 1; l < E.n_layers; ++l) B->l[l].xin = spare;
  }
}

// split-operand weight images of the three matrices of every layer (bwd: the transposed ones too); a no-op below 4096 rows
static inline int mamba2_images(rlx_ctx* ctx, const Mamba2& E, const float* p, bool bwd, int64_t M, hipStream_t st) {
  BxMat mats[3 * M2_MAX_LAYERS];
  int n = 0;
  for (int l = 0; l < E.n_layers; ++l) {
    const M2Layer& L = E.layer[l];
    mats[n++] = BxMat{p + L.W_in, E.d, 2 * E.I, true, bwd};
    mats[n++] = BxMat{p + L.W_x, E.I, E.I + 2 * E.N, true, bwd};
    mats[n++] = BxMat{p + L.W_out, E.I, E.d, true, bwd};
  }
  return net_images(ctx, mats, n, M, st);
}

// x [S T, d] -> out [S T, d], the carries h0 [S, L, I, N] / conv0 [S, L, K - 1, I] (NULL: zeros) -> hT / convT (NULL: not wanted);
// B keeps what mamba2_bwd reads
static inline int mamba2_fwd(rlx_ctx* ctx, const Mamba2& E, const float* p, const float* x, const uint8_t* done, const float* h0,
                             const float* conv0, int64_t S, int T, const M2Bufs& B, float* out, float* hT, float* convT, hipStream_t st) {
  const int64_t M = S * T;
  const int d = E.d, I = E.I, N = E.N, K = E.K, X = I + 2 * N, grid = rows_grid(ctx, M);
  const int64_t h_l = (int64_t)I * N, c_l = (int64_t)(K - 1) * I, h_ss = E.n_layers * h_l, c_ss = E.n_layers * c_l;
  int rc = RLX_OK;
  for (int l = 0; l < E.n_layers && !rc; ++l) {
    const M2Layer& L = E.layer[l];
    const M2LayerBufs& b = B.l[l];
    if (l == 0) rc = norm_act(L.ln, p, x, b.y, nullptr, grid, M, st);
    else {      // x_l = x_{l-1} + the previous block's branch, formed here
      const NormRes res{l > 1 ? B.l[l - 1].xin : x, b.xin};
      rc = norm_act(L.ln, p, B.branch, b.y, nullptr, grid, M, st, nullptr, &res);
    }
    if (!rc) rc = launch_gemm_fwd(ctx, b.y, p + L.W_in, p + L.b_in, b.proj, M, 2 * I, d, RLX_ACT_NONE, st, d);
    if (!rc) rc = ssm_conv_fwd(b.proj, 2 * I, done, conv0 && K > 1 ? conv0 + l * c_l : nullptr, c_ss, p + L.conv_w, p + L.conv_b, S, T, I, K, b.u,
                               convT && K > 1 ? convT + l * c_l : nullptr, c_ss, st);
    if (!rc) rc = launch_gemm_fwd(ctx, b.u, p + L.W_x, p + L.b_x, b.xp, M, X, I, RLX_ACT_NONE, st, I);
    if (!rc) rc = ssm_scan_fwd(b.u, b.xp, b.proj, done, h0 ? h0 + l * h_l : nullptr, h_ss, p + L.dt_bias, p + L.A_log, p + L.D, S, T, I, N, b.g,
                               hT ? hT + l * h_l : nullptr, h_ss, b.ckpt, 0, st);
    if (!rc) rc = launch_gemm_fwd(ctx, b.g, p + L.W_out, p + L.b_out, B.branch, M, d, I, RLX_ACT_NONE, st, I);
  }
  const int last = E.n_layers - 1;
  return rc ? rc : tf_add(last ? B.l[last].xin : x, B.branch, out, M * d, st);
}

// d_out [S T, d] -> grads (the flat layout, every entry written) and dx [S T, d]; consumes B
static inline int mamba2_bwd(rlx_ctx* ctx, const Mamba2& E, const float* p, const float* x, const uint8_t* done, const float* h0,
                             const float* conv0, int64_t S, int T, const M2Bufs& B, const float* d_out, float* grads, float* dx, hipStream_t st) {
  const int64_t M = S * T;
  const int d = E.d, I = E.I, N = E.N, K = E.K, X = I + 2 * N;
  const int64_t h_l = (int64_t)I * N, c_l = (int64_t)(K - 1) * I, h_ss = E.n_layers * h_l, c_ss = E.n_layers * c_l;
  int rc = RLX_OK;
  const float* dcur = d_out;      // d (layer output)
  for (int l = E.n_layers - 1; l >= 0 && !rc; --l) {
    const M2Layer& L = E.layer[l];
    const M2LayerBufs& b = B.l[l];
    rc = stage_dw(ctx, b.g, I, dcur, M, I, d, grads + L.W_out, grads + L.b_out, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, dcur, p + L.W_out, b.g, M, d, I, I, RLX_ACT_NONE, 0, st);                       // g <- d g
    if (!rc) rc = ssm_scan_bwd(ctx, b.u, b.xp, b.proj, done, h0 ? h0 + l * h_l : nullptr, h_ss, p + L.dt_bias, p + L.A_log, p + L.D, S, T, I, N,
                               b.ckpt, b.g, B.du_s, B.dxp, B.dproj, B.bc, grads + L.dt_bias, grads + L.A_log, grads + L.D, 0, st);
    if (!rc) rc = stage_dw(ctx, b.u, I, B.dxp, M, I, X, grads + L.W_x, grads + L.b_x, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, B.dxp, p + L.W_x, B.du_x, M, X, I, I, RLX_ACT_NONE, 0, st);
    if (!rc) rc = ssm_conv_bwd(ctx, b.proj, 2 * I, done, conv0 && K > 1 ? conv0 + l * c_l : nullptr, c_ss, p + L.conv_w, p + L.conv_b, S, T, I, K,
                               B.du_s, B.du_x, B.dproj, grads + L.conv_w, grads + L.conv_b, st);
    if (!rc) rc = stage_dw(ctx, b.y, d, B.dproj, M, d, 2 * I, grads + L.W_in, grads + L.b_in, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, B.dproj, p + L.W_in, b.y, M, 2 * I, d, d, RLX_ACT_NONE, 0, st);                 // y <- d ln out
    if (!rc) rc = tf_ln_bwd(ctx, L.ln, p, l ? b.xin : x, b.y, grads, NormRes{dcur, l ? nullptr : dx}, M, st);   // y (dx) <- d x_l
    dcur = b.y;
  }
  return rc;
}

}  // namespace rlx
