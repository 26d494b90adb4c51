// net_pass.h -- the network passes of fastsac.hip, fasttd3.hip, reppo.hip, mpo.hip, fastmpo.hip, espo.hip, tqc.hip, redq.hip, aqe.hip,
// droq.hip, crossq.hip and td3.hip (tqc ... crossq through sac_ens.h / sac_ens.hip, the layer they share; td3.hip takes its descriptor
// rules and row keys from sac_ens.h) on the host side: the launchers of brn.hip (batch
// renormalisation, the column-statistics layer), the launchers of dense_head.hip, grid sizes, the scratch-arena carve, key splitting, the split-operand weight images of a pass, and the passes
// themselves -- a Block (Linear -> [Dropout ->] {no norm | LayerNorm | RMSNorm} -> activation) with its forward, backward, input gradient and
// stage-arena size, and a Chain of up to four blocks plus a dense head.  An algorithm's file keeps its descriptor check, the list
// of blocks, the streams, and what differs in the graph (REPPO's critic).
// The epilogue rule of every input gradient (block_dx, head_bwd): the buffer it writes holds the output H of the block below; a
// plain block (NORM_NONE) with an activation gets act'(H) there, in place, so the buffer then holds that block's dZ; a normed
// block (or no block) gets none -- its norm backward takes dH.
#pragma once
#include "mlp.h"
#include "gemm_bx.h"
#include "fs_sched.h"

namespace rlx {

// ---- dense_head.hip
// out[M, N] = H[M, K] @ W[K, N] + b (any K and N: FastSAC's widths end at 768, FastTD3's at 1024)
int fs_head_fwd(const float* H, const float* W, const float* b, float* out, int64_t M, int K, int N, hipStream_t st);
// gW != NULL: weight / bias gradients from H_dH = H (slab partials into the stage arena: head_stage_floats); then dH over H_dH,
// times act'(H) (act: RLX_ACT_NONE, RELU, TANH or ELU; anything else is RLX_EUNSUP)
int fs_head_bwd(rlx_ctx* ctx, float* H_dH, const float* W, const float* d, float* gW, float* gb, int64_t M, int K, int N, hipStream_t st,
                int act);
// out[M, ld] = [obs (Oc columns) | act (A columns; zeros when NULL) | zero padding]
int fs_concat(const float* obs, int Oc, const float* act, int A, float* out, int ld, int64_t M, hipStream_t st);
// out[i] = normal(bits(key, i of n))
int launch_normal_noise(float* out, int64_t n, uint32_t k0, uint32_t k1, int scheme, hipStream_t st);

// ---- blocks: Linear W[in, out], b -> {no norm | LayerNorm scale g, bias be | RMSNorm scale g} -> act; W / b / g / be are
// offsets in the flat parameter vector (-1: absent), in that order.  The flat layouts are ABI: make_block only advances `off`.
enum NormKind { NORM_NONE = 0, NORM_LAYER = 1, NORM_RMS = 2 };
constexpr float MPO_LN_EPS = 1e-5f;   // torch.nn.LayerNorm default (mpo.hip's blocks; k_mpo_ln_tanh takes the block's eps)
// drop: the rate of a Dropout between the Linear and the norm (droq/flax/critic.py:27-30; 0: none).  It has no parameters.
struct Block { int in, out; int64_t W, b, g, be; int norm, act; float eps; float drop; };
static inline Block make_block(int64_t& off, int in, int out, int norm = NORM_NONE, int act = RLX_ACT_NONE, float eps = 0.f, float drop = 0.f) {
  Block o{in, out, off, 0, -1, -1, norm, act, eps, drop};
  off += (int64_t)in * out;
  o.b = off; off += out;
  if (norm != NORM_NONE) { o.g = off; off += out; }
  if (norm == NORM_LAYER) { o.be = off; off += out; }
  return o;
}
// The dropout keys of one pass (sac_sample.h: droq_layer_key): row i of the pass draws from split((k0, k1), count)[base + stride i]
// -- EnsRowKeys' addressing -- then part j of a split over the E vmapped networks, then part l of a split over the L hidden layers.
// A chain fills l and L in; a pass over a block with drop > 0 needs one, a block with drop == 0 never reads it.
struct DropKeys { uint32_t k0, k1; int scheme; uint32_t base, stride, count; int j, E; int l = 0, L = 1; };
// row norm + activation of a block over [M, out] (dense_head.hip).  part == NULL: forward Y = act(norm(Z)); else backward: dY (in
// Y) -> dZ, per-workgroup partials [grid][norm_part_width].  RLX_EUNSUP for a (norm, act) pair without a kernel, and for dropout
// in front of any other pair than (LayerNorm eps 1e-6, ReLU).  Z stays pre-dropout: both directions regenerate the mask from dk.
int norm_act(const Block& o, const float* p, const float* Z, float* Y, float* part, int grid, int64_t M, hipStream_t st,
             const DropKeys* dk = nullptr);
static inline int norm_part_width(const Block& o) { return (o.be >= 0 ? 2 : 1) * o.out; }   // [d scale | d bias] or [d scale]

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
// Row-norm backward: every workgroup leaves a slab of partial sums, and the reduction's workgroups that own a D-long segment add
// its slabs in a chain of S / 64 dependent round trips -- with one row per wave (1024 workgroups at 4096 rows) that chain was the
// tail of the whole reduction launch (30 us); 16 rows per workgroup leave 256 slabs.
static inline int bwd_rows_grid(const rlx_ctx* ctx, int64_t M) {
  int grid = div_up(M, 16);
  if (grid > ctx->num_cus * 4) grid = ctx->num_cus * 4;
  return grid < 1 ? 1 : grid;
}
// floats fs_head_bwd takes from the stage arena: at most div_up(M, 32) slabs of [K N | N], each part padded to four floats
static inline size_t head_stage_floats(int K, int N, int64_t M) {
  return a64((size_t)div_up(M, 32) * ((((size_t)K * N + 3) & ~size_t(3)) + (((size_t)N + 3) & ~size_t(3))));
}

// ---- brn.hip: batch renormalisation over the ROWS of x [M, D] (row stride ld, a multiple of four, 16-byte aligned; M >= 2), the
// column-statistics layer (crossq/flax/batch_renorm.py:77-130; brn.hip's header has the arithmetic).  One launch serves E networks
// whose buffers lie a fixed distance apart: x by e_x floats (0: one input shared by all), y / dY / dX by e_y, g / b / dg / db by e_p,
// the running statistics by e_s.
struct BrnCfg { float momentum, eps, r_max, d_max; };
struct BrnEns { int E; int64_t e_x, e_y, e_p, e_s; };
static inline int brn_dp(int D) { return (D + 3) & ~3; }
constexpr int BRN_SAVE_ROWS = 7;
// floats per network a training pass leaves for its backward (save: E of them back to back)
static inline size_t brn_save_floats(int D) { return (size_t)BRN_SAVE_ROWS * brn_dp(D); }
int brn_slabs(const rlx_ctx* ctx, int64_t M);                             // row slabs of the column sums: a function of M and num_cus only
size_t brn_work_floats(const rlx_ctx* ctx, int64_t M, int D, int E);      // `work` of a training pass or a backward (reusable once issued)
// y = (x - ra_mean) rsqrt(ra_var + eps) g + b: one launch, no state changes
int brn_fwd_eval(const float* x, int ld, int64_t M, int D, const float* g, const float* b, const float* ra_mean, const float* ra_var,
                 float eps, float* y, const BrnEns& n, hipStream_t st);
// the training pass: y from the batch statistics under the clipped r / d correction (warmed) or plain batch norm (not warmed);
// ra_mean / ra_var advance in place; save receives what brn_bwd needs
int brn_fwd_train(const rlx_ctx* ctx, const float* x, int ld, int64_t M, int D, const float* g, const float* b, float* ra_mean, float* ra_var,
                  const BrnCfg& cfg, bool warmed, float* y, float* save, float* work, const BrnEns& n, hipStream_t st);
// dY (in dY_dX) -> dX, in place; save != NULL: the backward of the training pass that wrote it, else of an eval pass (from ra_mean,
// ra_var and eps).  relu_mask: x is a ReLU's output and dX is multiplied by 1[x > 0].  dg / db (NULL: not wanted): the scale / bias
// gradients.  Padding columns of dX are 0.
int brn_bwd(const rlx_ctx* ctx, const float* x, int ld, int64_t M, int D, const float* g, const float* save, const float* ra_mean,
            const float* ra_var, float eps, float* dY_dX, bool relu_mask, float* dg, float* db, float* work, const BrnEns& n,
            hipStream_t st);

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
// stage_dw on the exact engine for the scope's lifetime (bx_dw_usable reads ctx->gemm_bx)
struct ExactDwScope {
  rlx_ctx* c;
  bool was;
  explicit ExactDwScope(rlx_ctx* ctx) : c(ctx), was(ctx->gemm_bx) { ctx->gemm_bx = false; }
  ~ExactDwScope() { c->gemm_bx = was; }
};

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
// Sum of squares of the gradients, then clip + Adam the torch way (clip_mode 1: torch.nn.utils.clip_grad_norm_; hp.max_grad_norm
// <= 0: no clipping) with hp's Adam constants; sq: REDUCE_MAX_BLOCKS floats; the gradient norm goes to *norm_out
template <class HP>
static inline int torch_clip_adam(float* p, const float* g, float* m, float* v, int64_t n, float* sq, int64_t step, float lr, const HP& hp,
                                  float* norm_out, hipStream_t st, float* polyak_target = nullptr, float tau = 0.f, float weight_decay = 0.f) {
  const int nsq = launch_sumsq_partials(g, n, sq, st);
  RLX_LAUNCH_CHECK();
  return launch_clip_adam(p, g, m, v, n, sq, nsq, step, lr, hp.max_grad_norm > 0.f ? hp.max_grad_norm : -1.f, hp.adam_b1, hp.adam_b2,
                          hp.adam_eps, norm_out, st, nullptr, nullptr, polyak_target, tau, weight_decay, 1);
}
// Input gradient of a first layer W[Kd, N] from dZ [M, N] into dx (row stride lddx): with nc > 0 only the columns [c0, c0 + nc)
// (a policy loss wants dQ/da) through the column-restricted product where it takes the shape, else the whole GEMM.
static inline int first_layer_dx(rlx_ctx* ctx, const float* dZ, const float* W, float* dx, int lddx, int64_t M, int N, int Kd, int c0,
                                 int nc, hipStream_t st) {
  if (dx_cols_ok(N, nc)) return launch_dx_cols(dZ, W + (int64_t)c0 * N, dx + c0, M, N, nc, lddx, st);
  return stage_dx(ctx, dZ, W, dx, M, N, Kd, lddx, RLX_ACT_NONE, 0, st, nullptr);
}

// ---- a block's passes.  x: the block's input [M, in] at row stride ldx; Z: pre-norm values (normed blocks only); H: output
static inline int block_fwd(rlx_ctx* ctx, const Block& o, const float* p, const float* x, int ldx, float* Z, float* H, int64_t M,
                            hipStream_t st, const DropKeys* dk = nullptr) {
  if (o.norm == NORM_NONE) return launch_gemm_fwd(ctx, x, p + o.W, p + o.b, H, M, o.out, o.in, o.act, st, ldx, nullptr);
  const int rc = launch_gemm_fwd(ctx, x, p + o.W, p + o.b, Z, M, o.out, o.in, RLX_ACT_NONE, st, ldx, nullptr);
  return rc ? rc : norm_act(o, p, Z, H, nullptr, rows_grid(ctx, M), M, st, dk);
}
// H holds dH of a normed block (-> dZ, in place) or dZ of a plain one (act' was applied by whoever wrote it).  grads != NULL: the
// block's parameter gradients (flat layout) through the deferred reduction; the norm partial is taken either way.
static inline int block_bwd(rlx_ctx* ctx, const Block& o, const float* p, const float* x, int ldx, const float* Z, float* H, float* grads,
                            int64_t M, hipStream_t st, const DropKeys* dk = nullptr) {
  if (o.norm != NORM_NONE) {
    const int grid = bwd_rows_grid(ctx, M);
    float* part = stage_alloc(ctx, (size_t)grid * norm_part_width(o));
    if (!part) return RLX_ENOMEM;
    int rc = norm_act(o, p, Z, H, part, grid, M, st, dk);
    if (!rc && grads) rc = norm_bwd_reduce(ctx, part, grid, o.out, grads + o.g, o.be >= 0 ? grads + o.be : nullptr, st);
    if (rc) return rc;
  }
  return grads ? stage_dw(ctx, x, ldx, H, M, o.in, o.out, grads + o.W, grads + o.b, nullptr, nullptr, st) : RLX_OK;
}
// floats block_bwd takes from the stage arena: its stage_alloc, and stage_dw's
static inline size_t block_stage_floats(const rlx_ctx* ctx, const Block& o, int64_t M, bool grads) {
  return (o.norm != NORM_NONE ? a64((size_t)bwd_rows_grid(ctx, M) * norm_part_width(o)) : 0) +
         (grads ? a64(stage_dw_floats(ctx, M, o.in, o.out)) : 0);
}
// the epilogue of an input gradient written over the output of block `prev` (the rule in the header): a plain block's activation
static inline int dx_epilogue(const Block* prev) { return prev && prev->norm == NORM_NONE ? prev->act : RLX_ACT_NONE; }
// input gradient of block o from its dZ into `out` [M, in], which holds the output of block prev (or NULL)
static inline int block_dx(rlx_ctx* ctx, const Block& o, const Block* prev, const float* p, const float* dZ, float* out, int64_t M,
                           hipStream_t st) {
  const int ep = dx_epilogue(prev);
  return stage_dx(ctx, dZ, p + o.W, out, M, o.out, o.in, o.in, ep, ep != RLX_ACT_NONE, st, nullptr);
}
// the head step of a block stack from d_head [M, head.out]: the head's parameter gradients (grads != NULL: flat layout, slabs into
// the stage arena), then its input gradient over H [M, head.in], which holds the output of block `below` (or NULL)
static inline int head_bwd(rlx_ctx* ctx, const Block& head, const Block* below, const float* p, float* H, const float* d_head, float* grads,
                           int64_t M, hipStream_t st) {
  return fs_head_bwd(ctx, H, p + head.W, d_head, grads ? grads + head.W : nullptr, grads ? grads + head.b : nullptr, M, head.in, head.out, st,
                     dx_epilogue(below));
}

// ---- a chain of blocks and a dense head
struct Chain { int n_hidden; Block layer[4]; Block head; int64_t n_params; };
// n_hidden blocks of one kind with the widths hidden[], then the head
static inline Chain make_chain(int in, const int* hidden, int n_hidden, int out, int norm, int act, float eps = 0.f, float drop = 0.f) {
  Chain L{};
  L.n_hidden = n_hidden;
  int64_t off = 0;
  for (int l = 0; l < n_hidden; ++l) {
    L.layer[l] = make_block(off, in, hidden[l], norm, act, eps, drop);
    in = hidden[l];
  }
  L.head = make_block(off, in, out);
  L.n_params = off;
  return L;
}
struct ChainBufs { float* Z[4]; float* H[4]; };   // [M, out_l]; the backward overwrites H_l with dH_l / dZ_l
static inline void chain_carve(const Chain& L, int64_t M, Arena& a, ChainBufs* b) {
  for (int l = 0; l < L.n_hidden; ++l) {
    b->Z[l] = L.layer[l].norm != NORM_NONE ? a.take((size_t)M * L.layer[l].out) : nullptr;
    b->H[l] = a.take((size_t)M * L.layer[l].out);
  }
}
// the pass's dropout keys for hidden layer l of the chain (NULL stays NULL)
static inline const DropKeys* chain_drop_keys(const Chain& L, const DropKeys* dk, int l, DropKeys* at) {
  if (!dk) return nullptr;
  *at = *dk;
  at->l = l;
  at->L = L.n_hidden;
  return at;
}
// x: [M, in] at row stride ldx (a multiple of four, zero padded); head_out == NULL: the trunk only; dk: the pass's dropout keys
static inline int chain_fwd(rlx_ctx* ctx, const Chain& L, const float* p, const float* x, int ldx, const ChainBufs& b, float* head_out,
                            int64_t M, hipStream_t st, const DropKeys* dk = nullptr) {
  DropKeys at;
  for (int l = 0; l < L.n_hidden; ++l) {
    const int rc = block_fwd(ctx, L.layer[l], p, l ? b.H[l - 1] : x, l ? L.layer[l].in : ldx, b.Z[l], b.H[l], M, st,
                             chain_drop_keys(L, dk, l, &at));
    if (rc) return rc;
  }
  if (!head_out) return RLX_OK;
  return fs_head_fwd(b.H[L.n_hidden - 1], p + L.head.W, p + L.head.b, head_out, M, L.head.in, L.head.out, st);
}
// backward from d_head [M, head.out]: the head step, then per block from the last: [norm backward, norm reduce], dW, dX.  The
// buffers are consumed.  dx != NULL: the input gradient (row stride lddx; the columns [dx_c0, dx_c0 + dx_nc) only when dx_nc > 0).
// dk: the dropout keys of the forward pass this one answers
static inline int chain_bwd(rlx_ctx* ctx, const Chain& L, const float* p, const float* x, int ldx, const ChainBufs& b, const float* d_head,
                            float* grads, float* dx, int lddx, int64_t M, hipStream_t st, int dx_c0 = 0, int dx_nc = 0,
                            const DropKeys* dk = nullptr) {
  int rc = head_bwd(ctx, L.head, &L.layer[L.n_hidden - 1], p, b.H[L.n_hidden - 1], d_head, grads, M, st);
  DropKeys at;
  for (int l = L.n_hidden - 1; l >= 0 && !rc; --l) {
    const Block& o = L.layer[l];
    rc = block_bwd(ctx, o, p, l ? b.H[l - 1] : x, l ? o.in : ldx, b.Z[l], b.H[l], grads, M, st, chain_drop_keys(L, dk, l, &at));
    if (rc) return rc;
    if (l > 0) rc = block_dx(ctx, o, &L.layer[l - 1], p, b.H[l], b.H[l - 1], M, st);
    else if (dx) rc = first_layer_dx(ctx, b.H[l], p + o.W, dx, lddx, M, o.out, o.in, dx_c0, dx_nc, st);
  }
  return rc;
}
// floats one backward of the chain takes from the stage arena: fs_head_bwd's slabs and every block's
static inline size_t chain_stage_floats(const rlx_ctx* ctx, const Chain& L, int64_t M, bool grads) {
  size_t n = grads ? head_stage_floats(L.head.in, L.head.out, M) : 0;
  for (int l = 0; l < L.n_hidden; ++l) n += block_stage_floats(ctx, L.layer[l], M, grads);
  return n;
}

// weight images of the hidden layers of several chains; bwd: the pass needs the transposed images too (input gradients).
// The budget is the image builder's job table: BX_MAX_JOBS images in one launch, a forward image is one job and a transposed one
// another.  Matrices are taken in the order listed (nets[0] first, layer 0 first) and the list ENDS at the first matrix whose
// jobs no longer fit: that layer and everything after it run on the exact engine.  No descriptor fastsac.hip and fasttd3.hip
// accept gets there -- the largest is FastSAC's critic update with four hidden layers: 4 + 2 * 4 + 2 * (4 + 3) = 26
// jobs (FastTD3: 3 + 2 * 3 + 2 * (3 + 2) = 19).  tqc.hip does, from six critics with three hidden layers on (policy 5, E online
// critics 5 each, E targets 3 each): it lists the nets in the order of their use.  mpo.hip registers its two matrices through
// net_images directly.
struct NetRef { const float* p; const Chain* L; bool bwd; };
static inline int trunk_images(rlx_ctx* ctx, const NetRef* nets, int n, int64_t M, hipStream_t st) {
  BxMat mats[BX_MAX_JOBS];
  int k = 0, jobs = 0;
  bool full = false;
  for (int i = 0; i < n && !full; ++i)
    for (int l = 0; l < nets[i].L->n_hidden; ++l) {
      const Block& o = nets[i].L->layer[l];
      if (o.in % 4 != 0) continue;                               // (a ragged first layer stays on the exact engine)
      const bool trans = nets[i].bwd && l > 0;
      if (jobs + 1 + (trans ? 1 : 0) > BX_MAX_JOBS) { full = true; break; }
      jobs += 1 + (trans ? 1 : 0);
      mats[k++] = BxMat{nets[i].p + o.W, o.in, o.out, true, trans};
    }
  return net_images(ctx, mats, k, M, st);
}

}  // namespace rlx
