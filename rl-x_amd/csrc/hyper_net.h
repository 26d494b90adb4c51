// hyper_net.h -- the hyperspherical network of the reference's simbav2 family on the host side (rl_x/algorithms/simbav2/flax/layers.py:8-93
// HyperDense / Scaler / HyperEmbedder / HyperMLP / HyperLERPBlock, :131-143 l2normalize_params), in mamba2_block.h's style: a descriptor
// of parameter offsets, the arena carve, and the forward and the backward as two functions (a plugin puts its head between them).
//   embedder:  xt = l2n([x, c_shift]);  z = xt W_e;  e = l2n(s_e * (c z))
//   block:     z1 = x W1;  h = relu(s1 * (c z1)) + EPS;  z2 = h W2;  y = l2n(z2);  v = x + a * (c_a (y - x));  x' = l2n(v)
// l2n(v) = v / max(|v|, EPS) along the row, EPS = 1e-8, c = scaler_init / scaler_scale, c_a = alpha_init / alpha_scale.
// FLAT PARAMETER LAYOUT (ABI): W_e [in + 1, H], s_e [H], then per block W1 [H, X], s1 [X], W2 [X, H], a [H]   (X = expansion H)
// GEMMs: launch_gemm_fwd / stage_dx / stage_dw as they are -- the exact engine below 4096 rows, the split-operand engine from 4096
// rows through net_images (hyper_images) for the blocks' matrices.  The embedder's matrix has in + 1 rows (ragged, tiny): its three
// products stay on the exact engine, over xt rows zero padded to a multiple of four floats.  HyperDense has no bias and the forward
// launchers read one: they get the context's zero vector (zeros_f32), no launcher is changed.
// Backward, in place where the stack allows: a lerp's backward leaves d z2 over z2 and the residual branch's gradient in R; the
// block's input gradient is R + T (T: what stage_dx brings down through W1), added at the load of the kernel that consumes it.
#pragma once
#include "net_pass.h"

namespace rlx {

constexpr int HYPER_MAX_BLOCKS = 4;
constexpr int HYPER_MAX_MATS = 1 + 2 * HYPER_MAX_BLOCKS;   // matrices of one network: one table of the projection kernel
constexpr float HYPER_EPS = 1e-8f;

// ---- hyper.hip.  Rows are [M, H] at row stride H (H % 64 == 0 <= 1024: one wave holds a row), 16-byte aligned.
// xt [M, ld] = l2n([x, shift]) zero padded to ld = (in + 1) rounded up to 4; rn [M] the reciprocal clamped norms
int hyper_embed_in(const rlx_ctx* ctx, const float* x, int in, float shift, int64_t M, float* xt, int ld, float* rn, hipStream_t st);
// d xt [M, ld] (columns <= in) -> dx [M, in]
int hyper_embed_in_bwd(const rlx_ctx* ctx, const float* dxt, const float* xt, const float* rn, int in, int ld, int64_t M, float* dx,
                       hipStream_t st);
// e = l2n(s * (c z))
int hyper_scale_norm(const rlx_ctx* ctx, const float* z, const float* s, float c, int64_t M, int H, float* e, hipStream_t st);
// d e = d (+ d2 where != NULL) -> d z over z, g_s [H]
int hyper_scale_norm_bwd(rlx_ctx* ctx, float* z_dz, const float* s, float c, const float* d, const float* d2, int64_t M, int H, float* g_s,
                         hipStream_t st);
// h = relu(s1 * (c z1)) + EPS over [M, X], X % 4 == 0
int hyper_relu(const float* z1, const float* s1, float c, int64_t M, int X, float* h, hipStream_t st);
// d h (in dh_dz1 [M, X]) -> d z1 over it, g_s1 [X]; X a multiple of H: a workgroup owns an H-wide column slab
int hyper_relu_bwd(rlx_ctx* ctx, const float* z1, const float* s1, float c, float* dh_dz1, int64_t M, int H, int X, float* g_s1, hipStream_t st);
// x' = l2n(x + a * (ca (l2n(z2) - x))) -> out (may be x); rn [M, 2] the reciprocal clamped norms of z2 and of v
int hyper_lerp(const rlx_ctx* ctx, const float* z2, const float* x, const float* a, float ca, int64_t M, int H, float* out, float* rn,
               hipStream_t st);
// d x' = d (+ d2 where != NULL) -> d z2 over z2, the residual branch's gradient -> dres (may be d), g_a [H]
int hyper_lerp_bwd(rlx_ctx* ctx, float* z2_dz2, const float* x, const float* a, float ca, const float* rn, const float* d, const float* d2,
                   int64_t M, int H, float* dres, float* g_a, hipStream_t st);
// W[:, n] /= max(|W[:, n]|, EPS) for the E matrices [K, N] that lie `stride` floats apart, every entry of the table in ONE launch
struct ColMat { float* W; int64_t stride; int K, N, E; };
int hyper_colnorm(const ColMat* mats, int n, hipStream_t st);

struct HyperBlock { int64_t W1, s1, W2, a; };
struct Hyper {
  int in, H, X, n_blocks, ld;      // ld: row stride of xt
  float shift, c, ca;
  int64_t We, se;
  HyperBlock blk[HYPER_MAX_BLOCKS];
  int64_t n_params;
};

static inline Hyper make_hyper(const rlx_hyper_desc& t) {
  Hyper E{};
  E.in = t.in_dim; E.H = t.hidden; E.X = t.hidden * t.expansion; E.n_blocks = t.n_blocks; E.ld = (t.in_dim + 1 + 3) & ~3;
  E.shift = t.c_shift; E.c = t.scaler_init / t.scaler_scale; E.ca = t.alpha_init / t.alpha_scale;
  const int64_t H = E.H, X = E.X;
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += n; return o; };
  E.We = take((int64_t)(E.in + 1) * H); E.se = take(H);
  for (int b = 0; b < t.n_blocks && b < HYPER_MAX_BLOCKS; ++b) {
    HyperBlock& L = E.blk[b];
    L.W1 = take(H * X); L.s1 = take(X); L.W2 = take(X * H); L.a = take(H);
  }
  E.n_params = off;
  return E;
}

// Activations of one block, kept for the backward.  A forward-only call gives every block the first block's set: a lerp then
// writes x' over x (a wave holds its whole row before it stores).
struct HyperBlockBufs {
  float* x;    // [M, H] the block's input
  float* z1;   // [M, X]
  float* h;    // [M, X]; backward: d h, then d z1
  float* z2;   // [M, H]; backward: d z2
  float* rn;   // [M, 2]
};
struct HyperBufs {
  float *xt, *rn0, *zE;      // [M, ld], [M], [M, H] (backward: d z of the embedder)
  HyperBlockBufs b[HYPER_MAX_BLOCKS];
  float *R, *T, *dxt;        // backward: [M, H] the residual branch's gradient, [M, H] the MLP branch's, [M, ld] d xt (dx wanted only)
};
static inline void hyper_carve(const Hyper& E, int64_t M, bool bwd, bool want_dx, Arena& a, HyperBufs* B) {
  const size_t m = (size_t)M, H = E.H, X = E.X;
  B->xt = a.take(m * E.ld);
  B->rn0 = a.take(m);
  B->zE = a.take(m * H);
  for (int b = 0; b < E.n_blocks; ++b) {
    HyperBlockBufs& k = B->b[b];
    if (b > 0 && !bwd) {
      k = B->b[0];
      continue;
    }
    k.x = a.take(m * H);
    k.z1 = a.take(m * X);
    k.h = a.take(m * X);
    k.z2 = a.take(m * H);
    k.rn = a.take(2 * m);
  }
  B->R = bwd ? a.take(m * H) : nullptr;
  B->T = bwd ? a.take(m * H) : nullptr;
  B->dxt = bwd && want_dx ? a.take(m * E.ld) : nullptr;
}

// split-operand weight images of the two matrices of every block (bwd: the transposed ones too); a no-op below 4096 rows
static inline int hyper_images(rlx_ctx* ctx, const Hyper& E, const float* p, bool bwd, int64_t M, hipStream_t st) {
  BxMat mats[2 * HYPER_MAX_BLOCKS];
  int n = 0;
  for (int b = 0; b < E.n_blocks; ++b) {
    mats[n++] = BxMat{p + E.blk[b].W1, E.H, E.X, true, bwd};
    mats[n++] = BxMat{p + E.blk[b].W2, E.X, E.H, true, bwd};
  }
  return net_images(ctx, mats, n, M, st);
}

// x [M, in] -> out [M, H]; B keeps what hyper_bwd reads
static inline int hyper_fwd(rlx_ctx* ctx, const Hyper& E, const float* p, const float* x, int64_t M, const HyperBufs& B, float* out,
                            hipStream_t st) {
  const int H = E.H, X = E.X;
  const float* zero = zeros_f32(ctx, 4096);      // the bias HyperDense does not have (X <= 4096)
  if (!zero) return RLX_ENOMEM;
  int rc = hyper_embed_in(ctx, x, E.in, E.shift, M, B.xt, E.ld, B.rn0, st);
  if (!rc) rc = launch_gemm_fwd(ctx, B.xt, p + E.We, zero, B.zE, M, H, E.in + 1, RLX_ACT_NONE, st, E.ld);
  if (!rc) rc = hyper_scale_norm(ctx, B.zE, p + E.se, E.c, M, H, B.b[0].x, st);
  for (int b = 0; b < E.n_blocks && !rc; ++b) {
    const HyperBlock& L = E.blk[b];
    const HyperBlockBufs& k = B.b[b];
    rc = gemm_fwd_auto(ctx, k.x, p + L.W1, zero, k.z1, M, X, H, RLX_ACT_NONE, st, H);
    if (!rc) rc = hyper_relu(k.z1, p + L.s1, E.c, M, X, k.h, st);
    if (!rc) rc = gemm_fwd_auto(ctx, k.h, p + L.W2, zero, k.z2, M, H, X, RLX_ACT_NONE, st, X);
    if (!rc) rc = hyper_lerp(ctx, k.z2, k.x, p + L.a, E.ca, M, H, b + 1 < E.n_blocks ? B.b[b + 1].x : out, k.rn, st);
  }
  return rc;
}

// d_out [M, H] -> grads (the flat layout, every entry written) and dx [M, in] (NULL: not wanted); consumes B
static inline int hyper_bwd(rlx_ctx* ctx, const Hyper& E, const float* p, int64_t M, const HyperBufs& B, const float* d_out, float* grads,
                            float* dx, hipStream_t st) {
  const int H = E.H, X = E.X;
  int rc = RLX_OK;
  const float *d = d_out, *d2 = nullptr;      // d (block output) = d + d2
  for (int b = E.n_blocks - 1; b >= 0 && !rc; --b) {
    const HyperBlock& L = E.blk[b];
    const HyperBlockBufs& k = B.b[b];
    rc = hyper_lerp_bwd(ctx, k.z2, k.x, p + L.a, E.ca, k.rn, d, d2, M, H, B.R, grads + L.a, st);                 // z2 <- d z2, R <- residual
    if (!rc) rc = stage_dw(ctx, k.h, X, k.z2, M, X, H, grads + L.W2, nullptr, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, k.z2, p + L.W2, k.h, M, H, X, X, RLX_ACT_NONE, 0, st);                            // h <- d h
    if (!rc) rc = hyper_relu_bwd(ctx, k.z1, p + L.s1, E.c, k.h, M, H, X, grads + L.s1, st);                       // h <- d z1
    if (!rc) rc = stage_dw(ctx, k.x, H, k.h, M, H, X, grads + L.W1, nullptr, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, k.h, p + L.W1, B.T, M, X, H, H, RLX_ACT_NONE, 0, st);                             // T <- MLP branch
    d = B.R;
    d2 = B.T;
  }
  if (!rc) rc = hyper_scale_norm_bwd(ctx, B.zE, p + E.se, E.c, d, d2, M, H, grads + E.se, st);                    // zE <- d z
  if (!rc) {
    ExactDwScope exact(ctx);      // in + 1 rows: the exact engine's guarded tiles
    rc = stage_dw(ctx, B.xt, E.ld, B.zE, M, E.in + 1, H, grads + E.We, nullptr, nullptr, nullptr, st);
  }
  if (rc || !dx) return rc;
  rc = stage_dx(ctx, B.zE, p + E.We, B.dxt, M, H, E.in + 1, E.ld, RLX_ACT_NONE, 0, st);
  return rc ? rc : hyper_embed_in_bwd(ctx, B.dxt, B.xt, B.rn0, E.in, E.ld, M, dx, st);
}

}  // namespace rlx
