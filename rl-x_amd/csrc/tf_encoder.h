// tf_encoder.h -- the pre-norm transformer encoder stack on the host side (rl_x/algorithms/ppo_transformer/flax_full_jit/policy.py:57-158:
// TransformerEncoderLayer / TransformerEncoder), in net_pass.h's style: a descriptor of parameter offsets, the arena carve, and the
// forward and the backward as two functions (a policy puts its decode chain between them).  Per layer
//   ln1 -> fused QKV GEMM -> banded attention (attn.hip) -> output projection -> + x -> ln2 -> Dense(dim_ff) + ReLU -> Dense(d_model) -> + x
// FLAT PARAMETER LAYOUT (ABI), per layer, in this order:
//   ln1 scale, ln1 bias, Wqkv [d, 3 d], bqkv [3 d], Wo [d, d], bo [d], ln2 scale, ln2 bias, W1 [d, ff], b1 [ff], W2 [ff, d], b2 [d]
// GEMMs: launch_gemm_fwd / stage_dx / stage_dw as they are -- the exact engine below 4096 rows, the split-operand engine from 4096
// rows through net_images (tf_encoder_images).
// Residual adds ride on the LayerNorm next to them (norm_act's NormRes): forward, x + branch is formed and stored by the LayerNorm
// that reads it (ln2, and the next layer's ln1); backward, a LayerNorm's input gradient receives the gradient arriving over the
// residual branch as its last addend -- LNbwd first, residual second: a fixed order.  Only the last layer's closing add is a kernel
// of its own (tf_add).  Dropout (tf_dropout, 0 in the reference's config) has no kernel: the entry point refuses a non-zero rate.
// Rows with valid == 0 are don't-care (attn.hip's header): the backward starts from d_out with those rows zeroed, so nothing of
// them reaches a parameter gradient, and dx is exactly 0 there.
#pragma once
#include "net_pass.h"

namespace rlx {

constexpr int TF_MAX_LAYERS = 4;

// ---- attn.hip
// RLX_EUNSUP, naming the field, outside head_dim in {16, 32, 64}, nhead <= 16, 1 <= window <= 64, T >= 1, S >= 1
int band_attn_check(const char* who, int64_t S, int64_t T, int nhead, int head_dim, int window);
int band_attn_fwd(const float* qkv, const int32_t* seg, const uint8_t* valid, int64_t S, int T, int nhead, int head_dim, int window, float* out,
                  float* lse, hipStream_t st);
int band_attn_bwd(const float* qkv, const int32_t* seg, const uint8_t* valid, int64_t S, int T, int nhead, int head_dim, int window,
                  const float* out, const float* lse, const float* d_out, float* dqkv, hipStream_t st);
int tf_add(const float* a, const float* b, float* out, int64_t n, hipStream_t st);                            // n % 4 == 0
int tf_mask_rows(const float* src, const uint8_t* valid, float* out, int64_t M, int d, hipStream_t st);       // d % 4 == 0

struct TfLayer { Block ln1, ln2; int64_t Wqkv, bqkv, Wo, bo, W1, b1, W2, b2; };
struct TfEncoder { int d, nhead, hd, ff, n_layers, window; TfLayer layer[TF_MAX_LAYERS]; int64_t n_params; };

static inline TfEncoder make_tf_encoder(const rlx_tf_desc& t) {
  TfEncoder E{};
  E.d = t.d_model; E.nhead = t.nhead; E.hd = t.nhead > 0 ? t.d_model / t.nhead : 0; E.ff = t.dim_ff; E.n_layers = t.n_layers; E.window = t.window;
  const int64_t d = t.d_model, ff = t.dim_ff;
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += n; return o; };
  auto ln = [&]() {   // a Block with no Linear: norm_act reads out, g, be, norm, act, eps and drop
    Block b{(int)d, (int)d, -1, -1, 0, 0, NORM_LAYER, RLX_ACT_NONE, t.ln_eps, 0.f};
    b.g = take(d); b.be = take(d);
    return b;
  };
  for (int l = 0; l < t.n_layers && l < TF_MAX_LAYERS; ++l) {
    TfLayer& L = E.layer[l];
    L.ln1 = ln();
    L.Wqkv = take(d * 3 * d); L.bqkv = take(3 * d);
    L.Wo = take(d * d); L.bo = take(d);
    L.ln2 = ln();
    L.W1 = take(d * ff); L.b1 = take(ff);
    L.W2 = take(ff * d); L.b2 = take(d);
  }
  E.n_params = off;
  return E;
}

// Activations of one layer, kept for the backward.  A forward-only call gives every layer the first layer's set.
struct TfLayerBufs {
  float* xin;    // [M, d] the layer's input (layer 0: the caller's x, not carved)
  float* xmid;   // [M, d] x + attention branch
  float* y1;     // [M, d] ln1(x); backward: d ln1 out, then d x
  float* qkv;    // [M, 3 d]
  float* att;    // [M, d] attention output (heads concatenated)
  float* lse;    // [M, nhead]
  float* y2;     // [M, d] ln2(xmid); backward: d ln2 out, then d xmid
  float* h1;     // [M, ff] relu(y2 W1 + b1); backward: its dZ
};
struct TfBufs {
  TfLayerBufs l[TF_MAX_LAYERS];
  float* branch;   // [M, d] a branch's output in front of its residual add; backward: d att
  float* dtop;     // [M, d] backward: d_out with the don't-care rows zeroed
  float* dqkv;     // [M, 3 d] backward
};
static inline void tf_encoder_carve(const TfEncoder& E, int64_t M, bool bwd, Arena& a, TfBufs* B) {
  const size_t d = (size_t)E.d;
  for (int l = 0; l < E.n_layers; ++l) {
    TfLayerBufs& b = B->l[l];
    if (l > 0 && !bwd) {      // (xin: set below)
      b = B->l[0];
      continue;
    }
    b.xin = l ? a.take(M * d) : nullptr;
    b.xmid = a.take(M * d);
    b.y1 = a.take(M * d);
    b.qkv = a.take(M * 3 * d);
    b.att = a.take(M * d);
    b.lse = a.take((size_t)M * E.nhead);
    b.y2 = a.take(M * d);
    b.h1 = a.take((size_t)M * E.ff);
  }
  B->branch = a.take(M * d);
  B->dtop = a.take(M * d);
  B->dqkv = bwd ? a.take(M * 3 * d) : nullptr;
  if (!bwd)   // forward only: a layer's input is dead once its ln2 has formed xmid, so one spare buffer serves every layer l > 0
    for (int l = 1; l < E.n_layers; ++l) B->l[l].xin = B->dtop;
}

// split-operand weight images of the four matrices of every layer (bwd: the transposed ones too); a no-op below 4096 rows
static inline int tf_encoder_images(rlx_ctx* ctx, const TfEncoder& E, const float* p, bool bwd, int64_t M, hipStream_t st) {
  BxMat mats[4 * TF_MAX_LAYERS];
  int n = 0;
  for (int l = 0; l < E.n_layers; ++l) {
    const TfLayer& L = E.layer[l];
    mats[n++] = BxMat{p + L.Wqkv, E.d, 3 * E.d, true, bwd};
    mats[n++] = BxMat{p + L.Wo, E.d, E.d, true, bwd};
    mats[n++] = BxMat{p + L.W1, E.d, E.ff, true, bwd};
    mats[n++] = BxMat{p + L.W2, E.ff, E.d, true, bwd};
  }
  return net_images(ctx, mats, n, M, st);
}

// x [S T, d] -> out [S T, d]; B keeps what tf_encoder_bwd reads
static inline int tf_encoder_fwd(rlx_ctx* ctx, const TfEncoder& E, const float* p, const float* x, const int32_t* seg, const uint8_t* valid,
                                 int64_t S, int T, const TfBufs& B, float* out, hipStream_t st) {
  const int64_t M = S * T;
  const int d = E.d, grid = rows_grid(ctx, M);
  int rc = RLX_OK;
  for (int l = 0; l < E.n_layers && !rc; ++l) {
    const TfLayer& L = E.layer[l];
    const TfLayerBufs& b = B.l[l];
    const float* xin = l ? b.xin : x;
    if (l == 0) rc = norm_act(L.ln1, p, x, b.y1, nullptr, grid, M, st);
    else {      // x_l = previous layer's xmid + its feed-forward branch, formed here
      const NormRes res{B.l[l - 1].xmid, b.xin};
      rc = norm_act(L.ln1, p, B.branch, b.y1, nullptr, grid, M, st, nullptr, &res);
    }
    if (!rc) rc = launch_gemm_fwd(ctx, b.y1, p + L.Wqkv, p + L.bqkv, b.qkv, M, 3 * d, d, RLX_ACT_NONE, st, d);
    if (!rc) rc = band_attn_fwd(b.qkv, seg, valid, S, T, E.nhead, E.hd, E.window, b.att, b.lse, st);
    if (!rc) rc = launch_gemm_fwd(ctx, b.att, p + L.Wo, p + L.bo, B.branch, M, d, d, RLX_ACT_NONE, st, d);
    if (!rc) {
      const NormRes res{xin, b.xmid};
      rc = norm_act(L.ln2, p, B.branch, b.y2, nullptr, grid, M, st, nullptr, &res);
    }
    if (!rc) rc = launch_gemm_fwd(ctx, b.y2, p + L.W1, p + L.b1, b.h1, M, E.ff, d, RLX_ACT_RELU, st, d);
    if (!rc) rc = launch_gemm_fwd(ctx, b.h1, p + L.W2, p + L.b2, B.branch, M, d, E.ff, RLX_ACT_NONE, st, E.ff);
  }
  return rc ? rc : tf_add(B.l[E.n_layers - 1].xmid, B.branch, out, M * d, st);
}

// a LayerNorm's backward: dY in Y -> its input gradient + res.add (into res.out, or over Y), and the scale / bias gradients
static inline int tf_ln_bwd(rlx_ctx* ctx, const Block& o, const float* p, const float* Z, float* Y, float* grads, const NormRes& res, int64_t M,
                            hipStream_t st) {
  const int grid = bwd_rows_grid(ctx, M);
  float* part = stage_alloc(ctx, (size_t)grid * norm_part_width(o));
  if (!part) return RLX_ENOMEM;
  const int rc = norm_act(o, p, Z, Y, part, grid, M, st, nullptr, &res);
  return rc ? rc : norm_bwd_reduce(ctx, part, grid, o.out, grads + o.g, grads + o.be, st);
}

// d_out [S T, d] -> grads (the flat layout, every entry written) and dx [S T, d]; consumes B
static inline int tf_encoder_bwd(rlx_ctx* ctx, const TfEncoder& E, const float* p, const float* x, const int32_t* seg, const uint8_t* valid,
                                 int64_t S, int T, const TfBufs& B, const float* d_out, float* grads, float* dx, hipStream_t st) {
  const int64_t M = S * T;
  const int d = E.d, ff = E.ff;
  int rc = tf_mask_rows(d_out, valid, B.dtop, M, d, st);
  const float* dcur = B.dtop;      // d (layer output)
  for (int l = E.n_layers - 1; l >= 0 && !rc; --l) {
    const TfLayer& L = E.layer[l];
    const TfLayerBufs& b = B.l[l];
    // feed-forward branch
    rc = stage_dw(ctx, b.h1, ff, dcur, M, ff, d, grads + L.W2, grads + L.b2, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, dcur, p + L.W2, b.h1, M, d, ff, ff, RLX_ACT_RELU, 1, st);                 // h1 <- dZ1
    if (!rc) rc = stage_dw(ctx, b.y2, d, b.h1, M, d, ff, grads + L.W1, grads + L.b1, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, b.h1, p + L.W1, b.y2, M, ff, d, d, RLX_ACT_NONE, 0, st);                  // y2 <- d ln2 out
    if (!rc) rc = tf_ln_bwd(ctx, L.ln2, p, b.xmid, b.y2, grads, NormRes{dcur, nullptr}, M, st);           // y2 <- d xmid
    // attention branch
    if (!rc) rc = stage_dw(ctx, b.att, d, b.y2, M, d, d, grads + L.Wo, grads + L.bo, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, b.y2, p + L.Wo, B.branch, M, d, d, d, RLX_ACT_NONE, 0, st);               // branch <- d att
    if (!rc) rc = band_attn_bwd(b.qkv, seg, valid, S, T, E.nhead, E.hd, E.window, b.att, b.lse, B.branch, B.dqkv, st);
    if (!rc) rc = stage_dw(ctx, b.y1, d, B.dqkv, M, d, 3 * d, grads + L.Wqkv, grads + L.bqkv, nullptr, nullptr, st);
    if (!rc) rc = stage_dx(ctx, B.dqkv, p + L.Wqkv, b.y1, M, 3 * d, d, d, RLX_ACT_NONE, 0, st);           // y1 <- d ln1 out
    if (!rc) rc = tf_ln_bwd(ctx, L.ln1, p, l ? b.xin : x, b.y1, grads, NormRes{b.y2, l ? nullptr : dx}, M, st);   // y1 (dx) <- d x_l
    dcur = b.y1;
  }
  return rc;
}

}  // namespace rlx
