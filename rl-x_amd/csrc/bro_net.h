// bro_net.h -- BroNet of the reference's bro family on the host side (rl_x/algorithms/bro/flax/layers.py:10-29), in hyper_net.h's
// style: a descriptor of parameter offsets, the arena carves, the weight images, and the forward and the backward as functions.
//   first layer:  z0 = x W0 + b0;  x_0 = relu(LN(z0) g0 + be0)
//   block b:      za = x_b Wa + ba;  ya = relu(LN(za) ga + bea);  zb = ya Wb + bb;  x_{b+1} = LN(zb) gb + beb + x_b     (post-norm)
//   output:       out = x_n Wo + bo  (out_dim > 0), else out = x_n
// LN is flax.linen.LayerNorm at ln_eps with the "fast variance" of ln_kernels.h: mean, E[z^2] - mean^2 clamped at 0, rsqrt.
// FLAT PARAMETER LAYOUT (ABI): W0 [in, H], b0, g0, be0, then per block Wa [H, H], ba, ga, bea, Wb [H, H], bb, gb, beb, then
// Wo [H, out], bo where out_dim > 0.  Every offset is a multiple of 64 floats (H % 64 == 0).
// Two forward routes.  LAYERED: one GEMM launch and one row-kernel launch per Dense (launch_gemm_fwd / stage_dx / stage_dw as they
// are: the exact engine below 4096 rows, the split-operand engine from 4096 rows for the H x H matrices; the ragged first layer on
// the exact engine over rows zero padded to a multiple of four floats; the output layer, any width, on the dense head of
// dense_head.hip).  It keeps every pre-norm value and the row statistics, and is the only route of a call with a backward.
// FUSED (forward only, small M): one k_bro_layer launch per Dense, which normalises the previous layer's pre-norm rows while it
// loads them (bro.hip has the kernel); nothing but the raw z and the block inputs x_b goes through memory.
// Backward, in place where the stack allows: a norm's backward rebuilds x^ from the kept z and (mean, rstd); the block-end norm
// leaves d zb over zb (its arriving gradient lives on as the residual branch's), the inner norm and the first layer's leave d z over
// the dead arriving gradient.  A block's input gradient is R + T (R: what arrived over the residual branch, T: what stage_dx
// brings down through Wa); the sum is formed at the load of the norm backward that consumes it, which also stores it as the new R.
#pragma once
#include "net_pass.h"

namespace rlx {

constexpr int BRO_MAX_BLOCKS = 4;
constexpr int64_t BRO_FUSED_MAX_M = 1024;   // fwd_path 0: forward-only calls of at most this many rows take the fused route
enum BroIn { BRO_IN_RAW = 0, BRO_IN_RELU = 1, BRO_IN_RES = 2 };

// ---- bro.hip.  Rows are [M, H] at row stride H (H % 64 == 0 <= 1024: one wave holds a row), 16-byte aligned.
// x == NULL: out = relu(LN(z) g + be); else out = LN(z) g + be + x (out may be x or z).  stats (NULL: not kept): [M, 2] (mean, rstd)
int bro_ln(const rlx_ctx* ctx, const float* z, const float* g, const float* be, const float* x, float eps, int64_t M, int H, float* out,
           float* stats, hipStream_t st);
// the arriving gradient d (+ d2 where != NULL) -> dz (may be z, d or d2); res: the norm of a block's end (no ReLU), where d + d2 is
// also stored to dres when d2 != NULL (dres may be d).  g_g, g_be [H]: the scale / bias gradients, through stage_reduce
int bro_ln_bwd(rlx_ctx* ctx, const float* z, const float* stats, const float* g, const float* be, bool res, const float* d, const float* d2,
               int64_t M, int H, float* dz, float* dres, float* g_g, float* g_be, hipStream_t st);
// dst [M, n] = src [M, ld][:, :n]
int bro_unpad(const float* src, int ld, int64_t M, int n, float* dst, hipStream_t st);
// one Dense layer of the fused route: zout [M, N] = f(in) W + bias with f by `mode`:
//   BRO_IN_RAW  f = in [M, K] (any K <= 1024)
//   BRO_IN_RELU f = relu(LN(in) g + be),  BRO_IN_RES f = LN(in) g + be + xres      (in, xres [M, K], K = H)
// xnew (NULL: not wanted; needs N == K): receives f(in), each column strip of the launch storing its own 64 columns.
struct BroLayer {
  const float *in, *g, *be, *xres;
  float* xnew;
  const float *W, *bias;
  float* zout;
  int64_t M;
  int K, N, mode;
  float eps;
};
bool bro_layer_fits(int K);      // the row tile of K columns fits the device's LDS
int bro_layer(const BroLayer& a, hipStream_t st);

struct BroBlock { int64_t Wa, ba, ga, bea, Wb, bb, gb, beb; };
struct Bro {
  int in, H, n_blocks, out, ld;      // ld: row stride of the padded input
  float eps;
  int64_t W0, b0, g0, be0, Wo, bo;
  BroBlock blk[BRO_MAX_BLOCKS];
  int64_t n_params;
};

static inline Bro make_bro(const rlx_bro_desc& t) {
  Bro E{};
  E.in = t.in_dim; E.H = t.hidden; E.n_blocks = t.n_blocks; E.out = t.out_dim; E.ld = (t.in_dim + 3) & ~3; E.eps = t.ln_eps;
  const int64_t H = E.H;
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += n; return o; };
  E.W0 = take(E.in * H); E.b0 = take(H); E.g0 = take(H); E.be0 = take(H);
  for (int b = 0; b < t.n_blocks && b < BRO_MAX_BLOCKS; ++b) {
    BroBlock& L = E.blk[b];
    L.Wa = take(H * H); L.ba = take(H); L.ga = take(H); L.bea = take(H);
    L.Wb = take(H * H); L.bb = take(H); L.gb = take(H); L.beb = take(H);
  }
  if (E.out > 0) { E.Wo = take(H * E.out); E.bo = take(E.out); }
  E.n_params = off;
  return E;
}

// Buffers of the layered route.  A forward-only call keeps nothing: every block shares one set, the inner norm runs in place
// over za and the block-end norm writes x' over x (a wave holds its whole row before it stores).
struct BroBufs {
  float *xp, *z0, *st0;                   // [M, ld], [M, H], [M, 2]
  float* X[BRO_MAX_BLOCKS + 1];           // [M, H] block inputs; X[n_blocks]: the trunk's output (the caller's `out` when out_dim == 0)
  float *za[BRO_MAX_BLOCKS], *ya[BRO_MAX_BLOCKS], *zb[BRO_MAX_BLOCKS];      // [M, H]; backward: ya <- d ya, then d za; zb <- d zb
  float *sta[BRO_MAX_BLOCKS], *stb[BRO_MAX_BLOCKS];                         // [M, 2]
  float *R, *T, *dxp;                     // backward: [M, H] residual branch, [M, H] Dense branch, [M, ld] padded dx (dx wanted only)
};
static inline void bro_carve(const Bro& E, int64_t M, bool bwd, bool want_dx, float* out, Arena& a, BroBufs* B) {
  const size_t m = (size_t)M, H = E.H;
  const int n = E.n_blocks;
  B->xp = a.take(m * E.ld);
  B->z0 = a.take(m * H);
  B->st0 = bwd ? a.take(2 * m) : nullptr;
  B->X[0] = a.take(m * H);
  for (int b = 0; b < n; ++b) {
    if (!bwd) {
      B->za[b] = B->ya[b] = B->z0;
      B->zb[b] = b ? B->zb[0] : a.take(m * H);
      B->sta[b] = B->stb[b] = nullptr;
      B->X[b + 1] = B->X[0];
    } else {
      B->za[b] = a.take(m * H); B->ya[b] = a.take(m * H); B->zb[b] = a.take(m * H);
      B->sta[b] = a.take(2 * m); B->stb[b] = a.take(2 * m);
      B->X[b + 1] = (b + 1 < n || E.out > 0) ? a.take(m * H) : nullptr;
    }
  }
  if (E.out == 0) B->X[n] = out;
  B->R = bwd ? a.take(m * H) : nullptr;
  B->T = bwd ? a.take(m * H) : nullptr;
  B->dxp = bwd && want_dx ? a.take(m * E.ld) : nullptr;
}
// the fused route: two z buffers and two x buffers, each written by one launch while the other is read
struct BroFusedBufs { float *Z[2], *X[2]; };
static inline void bro_carve_fused(const Bro& E, int64_t M, Arena& a, BroFusedBufs* F) {
  for (int i = 0; i < 2; ++i) {
    F->Z[i] = a.take((size_t)M * E.H);
    F->X[i] = a.take((size_t)M * E.H);
  }
}

// split-operand weight images of the two matrices of every block (bwd: the transposed ones too); a no-op below 4096 rows
static inline int bro_images(rlx_ctx* ctx, const Bro& E, const float* p, bool bwd, int64_t M, hipStream_t st) {
  BxMat mats[2 * BRO_MAX_BLOCKS];
  int n = 0;
  for (int b = 0; b < E.n_blocks; ++b) {
    mats[n++] = BxMat{p + E.blk[b].Wa, E.H, E.H, true, bwd};
    mats[n++] = BxMat{p + E.blk[b].Wb, E.H, E.H, true, bwd};
  }
  return net_images(ctx, mats, n, M, st);
}

// x [M, in] -> out [M, out or H] on the layered route; B keeps what bro_bwd reads
static inline int bro_fwd(rlx_ctx* ctx, const Bro& E, const float* p, const float* x, int64_t M, const BroBufs& B, float* out,
                          hipStream_t st) {
  const int H = E.H;
  int rc = fs_concat(x, E.in, nullptr, 0, B.xp, E.ld, M, st);
  if (!rc) rc = gemm_fwd_auto(ctx, B.xp, p + E.W0, p + E.b0, B.z0, M, H, E.in, RLX_ACT_NONE, st, E.ld);
  if (!rc) rc = bro_ln(ctx, B.z0, p + E.g0, p + E.be0, nullptr, E.eps, M, H, B.X[0], B.st0, st);
  for (int b = 0; b < E.n_blocks && !rc; ++b) {
    const BroBlock& L = E.blk[b];
    rc = gemm_fwd_auto(ctx, B.X[b], p + L.Wa, p + L.ba, B.za[b], M, H, H, RLX_ACT_NONE, st, H);
    if (!rc) rc = bro_ln(ctx, B.za[b], p + L.ga, p + L.bea, nullptr, E.eps, M, H, B.ya[b], B.sta[b], st);
    if (!rc) rc = gemm_fwd_auto(ctx, B.ya[b], p + L.Wb, p + L.bb, B.zb[b], M, H, H, RLX_ACT_NONE, st, H);
    if (!rc) rc = bro_ln(ctx, B.zb[b], p + L.gb, p + L.beb, B.X[b], E.eps, M, H, B.X[b + 1], B.stb[b], st);
  }
  if (rc || E.out == 0) return rc;
  return fs_head_fwd(B.X[E.n_blocks], p + E.Wo, p + E.bo, out, M, H, E.out, st);
}

// the same function on the fused route: 2 + 2 n_blocks launches
static inline int bro_fwd_fused(const rlx_ctx* ctx, const Bro& E, const float* p, const float* x, int64_t M, const BroFusedBufs& F, float* out,
                                hipStream_t st) {
  const int H = E.H;
  BroLayer a{};
  a.M = M; a.eps = E.eps;
  a.in = x; a.mode = BRO_IN_RAW; a.K = E.in; a.N = H; a.W = p + E.W0; a.bias = p + E.b0; a.zout = F.Z[0];
  int rc = bro_layer(a, st);
  int zi = 0, xi = 0;      // the buffers that hold the newest z and x
  a.K = H;
  for (int b = 0; b < E.n_blocks && !rc; ++b) {
    const BroBlock& L = E.blk[b];
    // x_b = the norm of the layer before (the first layer's, or the previous block's end) -> X, za = x_b Wa + ba
    a.in = F.Z[zi]; a.mode = b ? BRO_IN_RES : BRO_IN_RELU;
    a.g = p + (b ? E.blk[b - 1].gb : E.g0); a.be = p + (b ? E.blk[b - 1].beb : E.be0);
    a.xres = b ? F.X[xi] : nullptr; a.xnew = F.X[b ? xi ^ 1 : xi];
    a.W = p + L.Wa; a.bias = p + L.ba; a.zout = F.Z[zi ^ 1];
    rc = bro_layer(a, st);
    if (rc) return rc;
    zi ^= 1;
    if (b) xi ^= 1;
    a.in = F.Z[zi]; a.mode = BRO_IN_RELU; a.g = p + L.ga; a.be = p + L.bea; a.xres = nullptr; a.xnew = nullptr;
    a.W = p + L.Wb; a.bias = p + L.bb; a.zout = F.Z[zi ^ 1];
    rc = bro_layer(a, st);
    zi ^= 1;
  }
  if (rc) return rc;
  const BroBlock& L = E.blk[E.n_blocks - 1];
  if (E.out == 0) return bro_ln(ctx, F.Z[zi], p + L.gb, p + L.beb, F.X[xi], E.eps, M, H, out, nullptr, st);
  a.in = F.Z[zi]; a.mode = BRO_IN_RES; a.g = p + L.gb; a.be = p + L.beb; a.xres = F.X[xi]; a.xnew = nullptr;
  a.N = E.out; a.W = p + E.Wo; a.bias = p + E.bo; a.zout = out;
  return bro_layer(a, st);
}

// d_out [M, out or H] -> grads (the flat layout, every entry written) and dx [M, in] (NULL: not wanted); consumes B
static inline int bro_bwd(rlx_ctx* ctx, const Bro& E, const float* p, int64_t M, const BroBufs& B, const float* d_out, float* grads, float* dx,
                          hipStream_t st) {
  const int H = E.H, n = E.n_blocks;
  int rc = RLX_OK;
  const float *d = d_out, *d2 = nullptr;      // the gradient of a block's output is d + d2
  if (E.out > 0) {
    rc = fs_head_bwd(ctx, B.X[n], p + E.Wo, d_out, grads + E.Wo, grads + E.bo, M, H, E.out, st, RLX_ACT_NONE);      // X[n] <- d x_n
    d = B.X[n];
  }
  for (int b = n - 1; b >= 0 && !rc; --b) {
    const BroBlock& L = E.blk[b];
    rc = bro_ln_bwd(ctx, B.zb[b], B.stb[b], p + L.gb, p + L.beb, true, d, d2, M, H, B.zb[b], B.R, grads + L.gb, grads + L.beb, st);   // zb <- d zb
    if (d2) d = B.R;                                                                                                      // R <- d + d2
    if (!rc) rc = stage_dw(ctx, B.ya[b], H, B.zb[b], M, H, H, grads + L.Wb, grads + L.bb, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, B.zb[b], p + L.Wb, B.ya[b], M, H, H, H, RLX_ACT_NONE, 0, st);                             // ya <- d ya
    if (!rc) rc = bro_ln_bwd(ctx, B.za[b], B.sta[b], p + L.ga, p + L.bea, false, B.ya[b], nullptr, M, H, B.ya[b], nullptr, grads + L.ga,
                             grads + L.bea, st);                                                                          // ya <- d za
    if (!rc) rc = stage_dw(ctx, B.X[b], H, B.ya[b], M, H, H, grads + L.Wa, grads + L.ba, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, B.ya[b], p + L.Wa, B.T, M, H, H, H, RLX_ACT_NONE, 0, st);                                 // T <- Dense branch
    d2 = B.T;
  }
  if (!rc) rc = bro_ln_bwd(ctx, B.z0, B.st0, p + E.g0, p + E.be0, false, d, d2, M, H, B.T, nullptr, grads + E.g0, grads + E.be0, st);   // T <- d z0
  if (!rc) {
    ExactDwScope exact(ctx);      // in_dim rows: the exact engine's guarded tiles
    rc = stage_dw(ctx, B.xp, E.ld, B.T, M, E.in, H, grads + E.W0, grads + E.b0, nullptr, nullptr, st);
  }
  if (rc || !dx) return rc;
  rc = stage_dx(ctx, B.T, p + E.W0, B.dxp, M, H, E.in, E.ld, RLX_ACT_NONE, 0, st);
  return rc ? rc : bro_unpad(B.dxp, E.ld, M, E.in, dx, st);
}

}  // namespace rlx
