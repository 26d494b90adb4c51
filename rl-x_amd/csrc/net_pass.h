// net_pass.h -- what the network passes of fastsac.hip, fasttd3.hip, reppo.hip and mpo.hip share on the host side: the launchers of
// dense_head.hip, grid sizes, the scratch-arena carve, key splitting, the split-operand weight images of a pass, and the common
// tails of a norm block's and a first layer's backward.  The passes themselves (which layers, which activations, which streams)
// stay in each algorithm's file.
#pragma once
#include "mlp.h"
#include "gemm_bx.h"
#include "fs_sched.h"

namespace rlx {

// ---- dense_head.hip
// out[M, N] = H[M, K] @ W[K, N] + b (K <= 768, any N)
int fs_head_fwd(const float* H, const float* W, const float* b, float* out, int64_t M, int K, int N, hipStream_t st);
// gW != NULL: weight / bias gradients from H_dH = H (slab partials into the stage arena: head_stage_floats); then dH over H_dH,
// times ReLU'(H) with relu_mask
int fs_head_bwd(rlx_ctx* ctx, float* H_dH, const float* W, const float* d, float* gW, float* gb, int64_t M, int K, int N, hipStream_t st,
                bool relu_mask = false);
// out[M, ld] = [obs (Oc columns) | act (A columns; zeros when NULL) | zero padding]
int fs_concat(const float* obs, int Oc, const float* act, int A, float* out, int ld, int64_t M, hipStream_t st);
// out[i] = normal(bits(key, i of n))
int launch_normal_noise(float* out, int64_t n, uint32_t k0, uint32_t k1, int scheme, hipStream_t st);

// ---- sizes and grids
static inline size_t a64(size_t n) { return (n + 63) & ~size_t(63); }   // every arena buffer starts on a 256-byte boundary

static inline int elem_grid(int64_t n) {   // grid-stride element kernels, 256 threads
  int g = div_up(n, 256);
  return g > 4096 ? 4096 : (g < 1 ? 1 : g);
}
// One wave per row, four rows per workgroup (row-norm forward kernels).  Every caller has M > 0 (the entry points' RLX_REQUIRE on
// B / N / M / batch; MPO's R = 2 B), so the lower clamp never acts.
static inline int rows_grid(const rlx_ctx* ctx, int64_t M) {
  int grid = div_up(M, 4);
  if (grid > ctx->num_cus * 8) grid = ctx->num_cus * 8;
  return grid < 1 ? 1 : grid;
}
static inline int bwd_rows_grid(const rlx_ctx* ctx, int64_t M) {   // 16 rows per workgroup: fewer partial slabs (sac.hip: ln_bwd_grid)
  int grid = div_up(M, 16);
  if (grid > ctx->num_cus * 4) grid = ctx->num_cus * 4;
  return grid < 1 ? 1 : grid;
}
// floats fs_head_bwd takes from the stage arena: at most div_up(M, 32) slabs of [K N | N], each part padded to four floats
static inline size_t head_stage_floats(int K, int N, int64_t M) {
  return a64((size_t)div_up(M, 32) * ((((size_t)K * N + 3) & ~size_t(3)) + (((size_t)N + 3) & ~size_t(3))));
}

// ---- scratch arena: a bump allocator over one scratch slot.  An entry point writes its carve ONCE, as a callable over an Arena&;
// arena_carve runs it over a null base to measure, sizes the slot with that, and runs it again over the slot -- the total cannot
// disagree with the carve.  Over a null base take() returns NULL and only counts.
struct Arena {
  float* base;
  size_t off = 0;   // floats taken so far
  explicit Arena(float* b = nullptr) : base(b) {}
  float* take(size_t n) {
    float* p = base ? base + off : nullptr;
    off += a64(n);
    return p;
  }
};
template <class Carve>
static inline size_t arena_floats(Carve&& carve) {
  Arena m;
  carve(m);
  return m.off;
}
template <class Carve>
static inline int arena_carve(rlx_ctx* ctx, ScratchSlot slot, Carve&& carve, size_t floats = 0) {   // floats: a larger size to hold
  const size_t need = arena_floats(carve);
  float* base = (float*)scratch(ctx, slot, (floats > need ? floats : need) * sizeof(float));
  if (!base) return RLX_ENOMEM;
  Arena a(base);
  carve(a);
  return RLX_OK;
}

struct BxReleaseAll { rlx_ctx* c; ~BxReleaseAll() { bx_release_all(c); } };   // drops the registered weight images at scope exit

// key, *subkeys = split(key, 1 + nsub): advances key_io, sub receives 2 nsub words
static inline void next_key(uint32_t key_io[2], uint32_t* sub, int nsub, int scheme) {
  uint32_t ks[8];
  split_host(key_io, ks, 1 + nsub, scheme);
  key_io[0] = ks[0];
  key_io[1] = ks[1];
  for (int i = 0; i < 2 * nsub; ++i) sub[i] = ks[2 + i];
}

// ---- split-operand weight images for the GEMMs of a pass with >= 4096 rows (gemm_bx.h): launch_gemm_fwd / stage_dx pick them up
// by weight pointer.  The second half of a forked update runs on the side stream under scratch bank 1 (FsFork): the same images
// serve both banks.
static inline int net_images(rlx_ctx* ctx, const BxMat* mats, int n, int64_t M, hipStream_t st) {
  if (M < 4096 || !ctx->gemm_bx || n == 0) return RLX_OK;
  const int rc = bx_prepare_mats(ctx, mats, n, st);
  if (rc) return rc;
  for (int i = 0; i < ctx->bx_n[0]; ++i) ctx->bx_img[1][i] = ctx->bx_img[0][i];
  ctx->bx_n[1] = ctx->bx_n[0];
  return RLX_OK;
}
// the hidden layers of several networks of one layout type (n_hidden, layer[l].{in, out, W}); bwd: the pass needs the transposed
// images too (input gradients)
template <class Layout>
struct NetRef { const float* p; const Layout* L; bool bwd; };
template <class Layout>
static int trunk_images(rlx_ctx* ctx, const NetRef<Layout>* nets, int n, int64_t M, hipStream_t st) {
  BxMat mats[BX_MAX_JOBS];
  int k = 0;
  for (int i = 0; i < n; ++i)
    for (int l = 0; l < nets[i].L->n_hidden; ++l) {
      const auto& o = nets[i].L->layer[l];
      if (o.in % 4 != 0 || k >= BX_MAX_JOBS / 2) continue;      // (a ragged first layer stays on the exact engine)
      mats[k++] = BxMat{nets[i].p + o.W, o.in, o.out, true, nets[i].bwd && l > 0};
    }
  return net_images(ctx, mats, k, M, st);
}

// ---- backward tails
// The row-norm backward kernels leave per-workgroup partials: [grid][D] of d scale (RMSNorm: g_bias == NULL) or [grid][2 D] of
// [d scale | d bias] (LayerNorm).  Their column sums, in workgroup order, are the gradients.
static inline int norm_bwd_reduce(rlx_ctx* ctx, const float* part, int grid, int D, float* g_scale, float* g_bias, hipStream_t st) {
  const int64_t stride = g_bias ? (int64_t)2 * D : (int64_t)D;
  ReduceTable tab;
  tab.n = 0;
  tab.seg[tab.n++] = ReduceSeg{part, g_scale, (int64_t)D, stride, grid, 0, 1.f, 0.f, 1};
  if (g_bias) tab.seg[tab.n++] = ReduceSeg{part + D, g_bias, (int64_t)D, stride, grid, 0, 1.f, 0.f, 1};
  return stage_reduce(ctx, tab, nullptr, nullptr, st);
}
// Input gradient of a first layer W[Kd, N] from dZ [M, N] into dx (row stride lddx): with nc > 0 only the columns [c0, c0 + nc)
// (a policy loss wants dQ/da) through the column-restricted product where it takes the shape, else the whole GEMM.
static inline int first_layer_dx(rlx_ctx* ctx, const float* dZ, const float* W, float* dx, int lddx, int64_t M, int N, int Kd, int c0,
                                 int nc, hipStream_t st) {
  if (dx_cols_ok(N, nc)) return launch_dx_cols(dZ, W + (int64_t)c0 * N, dx + c0, M, N, nc, lddx, st);
  return stage_dx(ctx, dZ, W, dx, M, N, Kd, lddx, RLX_ACT_NONE, 0, st, nullptr);
}

}  // namespace rlx
