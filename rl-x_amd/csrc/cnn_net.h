// cnn_net.h -- the convolutional torso of the reference's image families on the host side (rl_x/algorithms/{dqn,ddqn,c51,
// dqn_hl_gauss,pqn}/flax/critic.py), in bro_net.h's style: a descriptor of parameter offsets and layer geometry, the arena carve,
// and the forward and the backward as functions.
//   x [M, C, H, W] uint8  ->  x / 255 as NHWC
//   conv l:   z_l = conv(y_{l-1}, W_l) + b_l (VALID, kernel k_l, stride s_l);  y_l = relu(z_l)            (norm 0)
//                                                                              y_l = relu(LN_c(z_l) g_l + be_l)   (norm 1: pqn)
//   flatten:  f = y_last as [M, OH OW ch_last] -- a view: NHWC is flax's (h, w, c) order
//   hidden:   zd = f Wd + bd;  hd = relu(zd)  or  relu(LN(zd) g + be)
//   output:   out = hd Wo + bo
// LN is flax.linen.LayerNorm with the fast variance of ln_kernels.h: mean, E[z^2] - mean^2 clamped at 0, rsqrt.
// FLAT PARAMETER LAYOUT (ABI): per convolution W [k, k, ci, co] (HWIO), b [co], with norm g, be [co]; then Wd [F, hidden], bd, with
// norm g, be [hidden]; then Wo [hidden, out_dim], bo.
// The convolutions run on cnn.hip (implicit GEMMs on the exact-fp32 MFMA, the staged map in LDS).  The hidden Dense runs on
// launch_gemm_fwd / stage_dw / stage_dx as they are, on the exact engine at every M (no weight images are registered, and the
// weight gradient, which would move to the split-operand engine by itself from 4096 rows, runs inside an ExactDwScope), its LayerNorm + ReLU on
// bro.hip's row kernels (bro_ln / bro_ln_bwd: any eps and rows up to 1024 floats, where norm_act's (LayerNorm, ReLU) pair ends at
// 768 columns and eps 1e-6), the output Dense on the dense head.
// Backward: a layer's gradient arrives as d y_l.  Without norm the ReLU mask 1[y_l > 0] is applied where the weight- and the
// input-gradient kernels load d y_l; with norm k_conv_ln_bwd turns d y_l into d z_l in place and leaves the scale / bias partials.
#pragma once
#include "bro_net.h"

namespace rlx {

constexpr int CNN_MAX_CONV = 3;
constexpr int CNN_BAND_PIXELS = 128;            // a forward workgroup's four waves own one 32-pixel tile each
constexpr size_t CNN_LDS_SOFT = 64 * 1024;      // bands grow up to this many bytes (two workgroups per CU); one row may take the device's limit

// One layer's geometry: the problem, and how each kernel lays its map out in LDS (all strides in floats).
struct ConvGeo {
  int H, W, CI, CO, k, s, OH, OW;
  int u8;                      // the input is the uint8 [M, CI, H, W] observation
  int CIe, T;                  // CI rounded up to even; K steps of the forward: k k CIe / 2
  // forward: Xs[ih][iw % s][ci][iw / s] -- neighbouring output pixels of a row are neighbouring floats
  int QWp, RS;                 // plane stride (odd), input-row stride (padded so that a tile's next output row continues the banks)
  int BR, NB, G;               // output rows per band, bands per image, images per workgroup (G > 1 only where NB == 1)
  size_t lds_fwd;
  // weight gradient: Xs[ih][iw][ci] (NHWC: a K tile's 32 rows are consecutive floats), Ds[pixel][co]
  int BRw, NBw, NPw;           // band rows, bands, the band's pixels rounded up to 16
  size_t lds_wg;
  // input gradient: Ds[oh + HL][co][ow + HL] with a zero halo of HL = ceil(k / s) pixels on every side
  int HL, OWP, RSd, n_tab;     // n_tab: entries of the per-phase step tables, each phase padded to 8
  size_t lds_dg;
  int lds_lim;                 // bytes of dynamic LDS a workgroup may take on the context's device
};

// bytes of dynamic LDS one workgroup may take on the context's device (queried once per device; a failed query is RLX_EHIP)
int cnn_lds_limit(const rlx_ctx* ctx, size_t* out);
// fills every field of g from the problem fields; RLX_EUNSUP where a kernel's smallest band does not fit LDS (`who` names the caller)
int conv_geometry(const rlx_ctx* ctx, ConvGeo* g, bool need_dgrad, const char* who);

// ---- cnn.hip
// y [M, OH, OW, CO] = relu(conv + b), or with g != NULL: z, st [M OH OW, 2] (mean, rstd) kept and y = relu(LN(z) g + be)
int conv_fwd(const ConvGeo& q, const uint8_t* xu, const float* xf, const float* W, const float* b, const float* g, const float* be, float eps,
             int64_t M, float* y, float* z, float* st, hipStream_t stm);
// d y -> d z in place over d (the ReLU mask is 1[y > 0] of the forward's stored y), [d g | d be] through the slab reduction
int conv_ln_bwd(rlx_ctx* ctx, const ConvGeo& q, const float* z, const float* st, const float* g, const float* y, float* d, int64_t M,
                float* g_g, float* g_be, hipStream_t stm);
// gW [k, k, CI, CO], gb [CO] from the layer's input and d (ymask != NULL: d is d y and 1[ymask > 0] is applied at its load)
int conv_wgrad(rlx_ctx* ctx, const ConvGeo& q, const uint8_t* xu, const float* xf, const float* d, const float* ymask, int64_t M, float* gW,
               float* gb, hipStream_t stm);
// dx [M, H, W, CI] from d (ymask as above) through Wt [k k, CO, CI], which conv_wt fills from W
int conv_wt(const ConvGeo& q, const float* W, float* Wt, hipStream_t stm);
int conv_dgrad(const ConvGeo& q, const float* d, const float* ymask, const float* Wt, int64_t M, float* dx, hipStream_t stm);

struct CnnConv { int64_t W, b, g, be; ConvGeo q; };
struct Cnn {
  int n_conv, F, hidden, out, norm;
  float eps;
  CnnConv cv[CNN_MAX_CONV];
  int64_t Wd, bd, gd, bed, Wo, bo, n_params;
};

// offsets and the problem fields of every layer's geometry (conv_geometry completes them); false: a map is smaller than its kernel
static inline bool make_cnn(const rlx_cnn_desc& t, Cnn* E) {
  *E = Cnn{};
  E->n_conv = t.n_conv; E->hidden = t.hidden; E->out = t.out_dim; E->norm = t.norm; E->eps = t.ln_eps;
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += n; return o; };
  int H = t.in_h, W = t.in_w, C = t.in_c;
  for (int l = 0; l < t.n_conv; ++l) {
    CnnConv& L = E->cv[l];
    const int k = t.kernel[l], s = t.stride[l], co = t.ch[l];
    if (k < 1 || s < 1 || H < k || W < k) return false;
    L.q.H = H; L.q.W = W; L.q.CI = C; L.q.CO = co; L.q.k = k; L.q.s = s; L.q.OH = (H - k) / s + 1; L.q.OW = (W - k) / s + 1; L.q.u8 = l == 0;
    L.W = take((int64_t)k * k * C * co); L.b = take(co);
    if (t.norm) { L.g = take(co); L.be = take(co); }
    H = L.q.OH; W = L.q.OW; C = co;
  }
  E->F = H * W * C;
  E->Wd = take((int64_t)E->F * t.hidden); E->bd = take(t.hidden);
  if (t.norm) { E->gd = take(t.hidden); E->bed = take(t.hidden); }
  E->Wo = take((int64_t)t.hidden * t.out_dim); E->bo = take(t.out_dim);
  E->n_params = off;
  return true;
}

struct CnnBufs {
  float *y[CNN_MAX_CONV], *z[CNN_MAX_CONV], *st[CNN_MAX_CONV];      // [M, P_l, ch_l]; z, st [M P_l, 2]: norm only, with a backward
  float *zd, *hd, *std;                                             // [M, hidden] (zd, std [M, 2]: norm only)
  float *d[CNN_MAX_CONV], *Wt;                                      // backward: d y_l, the transposed kernel of one layer
};
static inline void cnn_carve(const Cnn& E, int64_t M, bool bwd, Arena& a, CnnBufs* B) {
  const size_t m = (size_t)M;
  size_t wt = 0;
  for (int l = 0; l < E.n_conv; ++l) {
    const ConvGeo& q = E.cv[l].q;
    const size_t n = m * q.OH * q.OW;
    B->y[l] = a.take(n * q.CO);
    B->z[l] = E.norm ? a.take(n * q.CO) : nullptr;
    B->st[l] = E.norm ? a.take(2 * n) : nullptr;
    B->d[l] = bwd ? a.take(n * q.CO) : nullptr;
    if (l > 0 && wt < (size_t)q.k * q.k * q.CI * q.CO) wt = (size_t)q.k * q.k * q.CI * q.CO;
  }
  B->zd = E.norm ? a.take(m * E.hidden) : nullptr;
  B->std = E.norm ? a.take(2 * m) : nullptr;
  B->hd = a.take(m * E.hidden);
  B->Wt = bwd && wt ? a.take(wt) : nullptr;
}

// x [M, C, H, W] uint8 -> out [M, out_dim]; B keeps what cnn_bwd reads
static inline int cnn_fwd(rlx_ctx* ctx, const Cnn& E, const float* p, const uint8_t* x, int64_t M, const CnnBufs& B, float* out,
                          hipStream_t st) {
  int rc = RLX_OK;
  for (int l = 0; l < E.n_conv && !rc; ++l) {
    const CnnConv& L = E.cv[l];
    rc = conv_fwd(L.q, l ? nullptr : x, l ? B.y[l - 1] : nullptr, p + L.W, p + L.b, E.norm ? p + L.g : nullptr, E.norm ? p + L.be : nullptr,
                  E.eps, M, B.y[l], B.z[l], B.st[l], st);
  }
  const float* f = B.y[E.n_conv - 1];      // the flatten: a view
  if (!rc && !E.norm) rc = gemm_fwd_auto(ctx, f, p + E.Wd, p + E.bd, B.hd, M, E.hidden, E.F, RLX_ACT_RELU, st, E.F);
  if (!rc && E.norm) rc = gemm_fwd_auto(ctx, f, p + E.Wd, p + E.bd, B.zd, M, E.hidden, E.F, RLX_ACT_NONE, st, E.F);
  if (!rc && E.norm) rc = bro_ln(ctx, B.zd, p + E.gd, p + E.bed, nullptr, E.eps, M, E.hidden, B.hd, B.std, st);
  return rc ? rc : fs_head_fwd(B.hd, p + E.Wo, p + E.bo, out, M, E.hidden, E.out, st);
}

// d_out [M, out_dim] -> grads (the flat layout, every entry written); consumes B
static inline int cnn_bwd(rlx_ctx* ctx, const Cnn& E, const float* p, const uint8_t* x, int64_t M, const CnnBufs& B, const float* d_out,
                          float* grads, hipStream_t st) {
  const int n = E.n_conv;
  // hd <- d hd, times 1[hd > 0] without norm (then it is d zd)
  int rc = fs_head_bwd(ctx, B.hd, p + E.Wo, d_out, grads + E.Wo, grads + E.bo, M, E.hidden, E.out, st, E.norm ? RLX_ACT_NONE : RLX_ACT_RELU);
  if (!rc && E.norm)
    rc = bro_ln_bwd(ctx, B.zd, B.std, p + E.gd, p + E.bed, false, B.hd, nullptr, M, E.hidden, B.hd, nullptr, grads + E.gd, grads + E.bed, st);
  if (!rc) {
    ExactDwScope exact(ctx);      // from 4096 rows stage_dw would take the split-operand engine by itself: the torso stays exact fp32
    rc = stage_dw(ctx, B.y[n - 1], E.F, B.hd, M, E.F, E.hidden, grads + E.Wd, grads + E.bd, nullptr, nullptr, st);
  }
  if (!rc) rc = stage_dx(ctx, B.hd, p + E.Wd, B.d[n - 1], M, E.hidden, E.F, E.F, RLX_ACT_NONE, 0, st);      // d y_last, flattened
  for (int l = n - 1; l >= 0 && !rc; --l) {
    const CnnConv& L = E.cv[l];
    const float* mask = E.norm ? nullptr : B.y[l];
    if (E.norm) rc = conv_ln_bwd(ctx, L.q, B.z[l], B.st[l], p + L.g, B.y[l], B.d[l], M, grads + L.g, grads + L.be, st);      // d[l] <- d z_l
    if (!rc) rc = conv_wgrad(ctx, L.q, l ? nullptr : x, l ? B.y[l - 1] : nullptr, B.d[l], mask, M, grads + L.W, grads + L.b, st);
    if (!rc && l > 0) rc = conv_wt(L.q, p + L.W, B.Wt, st);
    if (!rc && l > 0) rc = conv_dgrad(L.q, B.d[l], mask, B.Wt, M, B.d[l - 1], st);
  }
  return rc;
}

}  // namespace rlx
