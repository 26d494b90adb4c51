// crossq.hip -- CrossQ (rl_x/algorithms/crossq/flax/crossq.py:135-274): SAC without target networks, over networks whose every Dense
// is preceded by a batch renormalisation (brn.hip; critic.py:25-60, policy.py:34-72): x -> BRN -> Dense -> ReLU -> BRN -> ... -> BRN ->
// Dense head.  The reference's two jitted functions are two entry points (FastSAC's critic / policy pair is the precedent), acting a
// third:
//   critic update (:147-206)  key, subkey = split(key); the policy in EVAL mode on s'; ONE block draw normal(subkey, (B, A)); a', logp';
//               every critic in TRAIN mode on the 2 B rows [(s, a); (s', a')] -- one joint pass, so the batch statistics are those of
//               both halves; q = the first B outputs, next_q the last B; y = r + gamma (1 - term) (min_e next_q - alpha logp') under
//               stop_gradient; loss = mean over E and B of (q - y)^2; plain Adam (b1 = critic_adam_b1); the critics' statistics advance.
//               The head gradient of the last B rows is 0, their gradient below the last BRN is not: the backward runs over all 2 B.
//   policy update (:210-274)  key, subkey = split(key); the policy in TRAIN mode on s; a block draw; the critics in EVAL mode (with the
//               statistics as they are); loss = mean(alpha logp - min_e q), the gradient to the minimising critic, split evenly among
//               exact ties; alpha's loss and plain Adam step (sac_ens.hip: k_ens_finish); Adam on the policy; its statistics advance.
//   acting (:135-143)         the policy in EVAL mode; key, subkey = split(key); tanh(mean + std normal(subkey, (N, A))).
// WARM-UP: a layer's w is 1 once its network's count of earlier training passes has reached brn_warmup_steps; a network makes one
// training pass per update, so that count is its optimiser count: q_opt_count for the critics, pi_opt_count for the policy.
// FLAT LAYOUT of one network (ABI): bn0.scale[in], bn0.bias[in], W1[in, H1], b1, bn1.scale[H1], bn1.bias[H1], W2, b2, ..., bnL.scale,
// bnL.bias, W_head[HL, out], b_head; the E critics back to back; the policy's head is SAC's single [H, 2 A].  Its running statistics
// are a vector of their own: bn0.mean[in], bn0.var[in], bn1.mean, bn1.var, ...; `qstats` holds the E critics' back to back.
// A pass runs the E networks' BRN layers in one launch each (brn.hip: three per training pass, one per eval pass) and their GEMMs
// per network on one stream; passes of >= 4096 rows take the split-operand images (cq_images), smaller ones and acting the exact fp32
// engine; reductions run in a fixed order: identical calls give identical bits.
// A wide layer's weight gradient is taken in row bands of W so that each band's slab reduction fits REDUCE_MAX_BLOCKS.
// CPU twin: tests/crossq_twin.py.  The reference's CrossQ is JAX only; see DESIGN.md 4.5h for what is pinned.
#include "sac_ens.h"

namespace rlx {

constexpr int CQ_MAXE = 16, CQ_MAX_WIDTH = 2048;

// offsets of one network: BRN l (l = 0 .. L) normalises D(l) columns -- the input (l = 0) or hidden layer l's output -- at row
// stride ld(l); Dense l (l < L) maps D(l) -> D(l + 1), Dense L is the head
struct CqNet {
  int L, in, out, ld0, width[4];
  int64_t bn[5], W[5], b[5], st[5], n_params, n_stats;
  int D(int l) const { return l ? width[l - 1] : in; }
  int ld(int l) const { return l ? width[l - 1] : ld0; }
};
static CqNet cq_layout(const rlx_mlp_desc& d) {
  CqNet n{};
  n.L = d.n_hidden; n.in = d.in_dim; n.out = d.out_dim; n.ld0 = (d.in_dim + 3) & ~3;
  int64_t off = 0, so = 0;
  for (int l = 0; l <= n.L; ++l) {
    if (l < n.L) n.width[l] = d.hidden[l];
    const int D = n.D(l), next = l < n.L ? d.hidden[l] : d.out_dim;
    n.bn[l] = off; off += 2 * (int64_t)D;
    n.W[l] = off; off += (int64_t)D * next;
    n.b[l] = off; off += next;
    n.st[l] = so; so += 2 * (int64_t)D;
  }
  n.n_params = off; n.n_stats = so;
  return n;
}
static int cq_check_net(const rlx_mlp_desc& d, const std::string& who) {
  RLX_REQUIRE(d.n_hidden >= 1 && d.n_hidden <= 3 && d.in_dim > 0 && d.out_dim > 0, RLX_EINVAL, who + " needs 1..3 hidden layers and positive widths");
  RLX_REQUIRE(d.act == RLX_ACT_RELU && !d.ln_first && !d.has_logstd, RLX_EINVAL, who + " must be act = RLX_ACT_RELU, ln_first = 0, has_logstd = 0");
  for (int l = 0; l < d.n_hidden; ++l)
    RLX_REQUIRE(d.hidden[l] > 0 && d.hidden[l] % 64 == 0 && d.hidden[l] <= CQ_MAX_WIDTH, RLX_EUNSUP,
                who + " hidden widths must be multiples of 64, at most 2048");
  return RLX_OK;
}
static int cq_check_hp(const rlx_crossq_hparams& hp, const std::string& fn) {
  RLX_REQUIRE(hp.ensemble_size >= 1, RLX_EINVAL, fn + ": hp->ensemble_size must be at least 1");
  RLX_REQUIRE(hp.ensemble_size <= CQ_MAXE, RLX_EUNSUP, fn + ": hp->ensemble_size at most 16");
  RLX_REQUIRE(hp.brn_momentum >= 0.f && hp.brn_momentum < 1.f, RLX_EINVAL, fn + ": hp->brn_momentum must be in [0, 1)");
  RLX_REQUIRE(hp.brn_eps > 0.f && hp.brn_r_max >= 1.f && hp.brn_d_max >= 0.f && hp.brn_warmup_steps >= 0, RLX_EINVAL,
              fn + ": hp->brn_eps must be positive, brn_r_max at least 1, brn_d_max and brn_warmup_steps at least 0");
  return RLX_OK;
}

// the activations of E networks' passes over M rows: U[l] the input of BRN l (l >= 1: hidden layer l's output; l = 0 is the caller's
// x, shared by the E networks), N[l] its output -- the backward leaves dZ of hidden layer l there (l >= 1), or d L / d x (l = 0)
struct CqBufs { float *U[5], *N[5], *save[5], *work; };
static void cq_carve(const rlx_ctx* ctx, const CqNet& n, int E, int64_t M, bool train, Arena& a, CqBufs* b) {
  size_t work = 0;
  for (int l = 0; l <= n.L; ++l) {
    b->U[l] = l ? a.take((size_t)E * M * n.ld(l)) : nullptr;
    b->N[l] = a.take((size_t)E * M * n.ld(l));
    b->save[l] = train ? a.take((size_t)E * brn_save_floats(n.D(l))) : nullptr;
    const size_t w = brn_work_floats(ctx, M, n.D(l), E);
    work = w > work ? w : work;
  }
  b->work = a.take(work);
}
static BrnEns cq_ens(const CqNet& n, int E, int64_t M, int l) {
  return BrnEns{E, l ? M * n.ld(l) : 0, M * n.ld(l), n.n_params, n.n_stats};
}
// x [M, ld0] (zero padded) -> head_out [E][M, out]; train: the statistics advance and the saves are written
static int cq_fwd(rlx_ctx* ctx, const CqNet& n, const float* params, float* stats, int E, const float* x, int64_t M, const CqBufs& b,
                  bool train, bool warmed, const BrnCfg& cfg, float* head_out, hipStream_t st) {
  for (int l = 0; l <= n.L; ++l) {
    const int D = n.D(l), ld = n.ld(l);
    const float* xin = l ? b.U[l] : x;
    const float* g = params + n.bn[l];
    float* mean = stats + n.st[l];
    const BrnEns ens = cq_ens(n, E, M, l);
    int rc = train ? brn_fwd_train(ctx, xin, ld, M, D, g, g + D, mean, mean + D, cfg, warmed, b.N[l], b.save[l], b.work, ens, st)
                   : brn_fwd_eval(xin, ld, M, D, g, g + D, mean, mean + D, cfg.eps, b.N[l], ens, st);
    for (int e = 0; e < E && !rc; ++e) {
      const float* p = params + e * n.n_params;
      const float* Ne = b.N[l] + (size_t)e * M * ld;
      if (l < n.L) rc = launch_gemm_fwd(ctx, Ne, p + n.W[l], p + n.b[l], b.U[l + 1] + (size_t)e * M * n.width[l], M, n.width[l], D, RLX_ACT_RELU, st, ld, nullptr);
      else rc = fs_head_fwd(Ne, p + n.W[l], p + n.b[l], head_out + (size_t)e * M * n.out, M, D, n.out, st);
    }
    if (rc) return rc;
  }
  return RLX_OK;
}
// gW[Kd, N] = Hp^T dZ in row bands of W whose slab reduction fits one launch (REDUCE_MAX_BLOCKS); the bias gradient from the first
static int cq_dw(rlx_ctx* ctx, const float* Hp, int ldh, const float* dZ, int64_t M, int Kd, int N, float* gW, float* gB, hipStream_t st) {
  auto blocks = [&](int k) {
    int S = 1;
    (void)choose_mc(M, div_up(k, G_BM) * div_up(N, G_BN), ctx->num_cus, &S);
    const int64_t len = (int64_t)k * N;
    return (int64_t)(S >= 128 ? div_up(len, 64) : div_up(len, 256)) + div_up(N, 16);
  };
  int kb = Kd;
  while (kb > 64 && blocks(kb) > REDUCE_MAX_BLOCKS) kb = ((kb / 2 + 63) / 64) * 64;
  for (int k0 = 0; k0 < Kd; k0 += kb) {
    const int k = Kd - k0 < kb ? Kd - k0 : kb;
    const int rc = stage_dw(ctx, Hp + k0, ldh, dZ, M, k, N, gW + (int64_t)k0 * N, k0 == 0 ? gB : nullptr, nullptr, nullptr, st);
    if (rc) return rc;
  }
  return RLX_OK;
}
// backward from d_head [E][M, out].  grads (flat layout, E back to back) or NULL: input gradient only.  train: the backward of the
// training pass that filled b.save; else of an eval pass.  Leaves d L / d x in b.N[0] ([E][M, ld0]).
static int cq_bwd(rlx_ctx* ctx, const CqNet& n, const float* params, const float* stats, int E, const float* x, int64_t M, const CqBufs& b,
                  bool train, const BrnCfg& cfg, const float* d_head, float* grads, hipStream_t st) {
  int rc = RLX_OK;
  for (int e = 0; e < E && !rc; ++e) {
    const float* p = params + e * n.n_params;
    float* g = grads ? grads + e * n.n_params : nullptr;
    rc = fs_head_bwd(ctx, b.N[n.L] + (size_t)e * M * n.ld(n.L), p + n.W[n.L], d_head + (size_t)e * M * n.out, g ? g + n.W[n.L] : nullptr,
                     g ? g + n.b[n.L] : nullptr, M, n.D(n.L), n.out, st, RLX_ACT_NONE);
  }
  for (int l = n.L; l >= 0 && !rc; --l) {
    const int D = n.D(l), ld = n.ld(l);
    const float* mean = stats + n.st[l];
    rc = brn_bwd(ctx, l ? b.U[l] : x, ld, M, D, params + n.bn[l], train ? b.save[l] : nullptr, mean, mean + D, cfg.eps, b.N[l], l > 0,
                 grads ? grads + n.bn[l] : nullptr, grads ? grads + n.bn[l] + D : nullptr, b.work, cq_ens(n, E, M, l), st);
    for (int e = 0; e < E && !rc && l > 0; ++e) {   // Dense l - 1: D(l - 1) -> D(l), its dZ now in N[l]
      const float* p = params + e * n.n_params;
      float* Nb = b.N[l - 1] + (size_t)e * M * n.ld(l - 1);
      const float* dZ = b.N[l] + (size_t)e * M * ld;
      if (grads) rc = cq_dw(ctx, Nb, n.ld(l - 1), dZ, M, n.D(l - 1), D, grads + e * n.n_params + n.W[l - 1], grads + e * n.n_params + n.b[l - 1], st);
      if (!rc) rc = stage_dx(ctx, dZ, p + n.W[l - 1], Nb, M, D, n.D(l - 1), n.ld(l - 1), RLX_ACT_NONE, 0, st, nullptr);
    }
  }
  return rc;
}

// Split-operand weight images (gemm_bx.h) for the passes of a call with >= 4096 rows, trunk_images' rules over this file's layout:
// a Dense whose input width is no multiple of four stays on the exact engine, the transposed image (input gradients) only above
// the first Dense, matrices in the order listed, and the list ends where the image builder's job table is full.  A network is
// listed only when ITS pass has >= 4096 rows.
struct CqNetRef { const float* p; const CqNet* n; int E; int64_t rows; bool bwd; };
static int cq_images(rlx_ctx* ctx, const CqNetRef* nets, int n_nets, hipStream_t st) {
  std::vector<BxMat> mats;
  int64_t rows = 0;
  for (int i = 0; i < n_nets; ++i) {
    if (nets[i].rows < 4096) continue;
    rows = nets[i].rows > rows ? nets[i].rows : rows;
    for (int e = 0; e < nets[i].E; ++e)
      for (int l = 0; l < nets[i].n->L; ++l)
        if (nets[i].n->D(l) % 4 == 0)
          mats.push_back(BxMat{nets[i].p + e * nets[i].n->n_params + nets[i].n->W[l], nets[i].n->D(l), nets[i].n->width[l], true, nets[i].bwd && l > 0});
  }
  return mats.empty() ? RLX_OK : net_images(ctx, mats.data(), (int)mats.size(), rows, st);
}

// One thread per transition (crossq.py:176-190) over q [E][2 B]: y_b = r_b + gamma (1 - term_b) (min_e q[e, B + b] - alpha logp'_b);
// dq[e, b] = 2 (q[e, b] - y_b) / (B E), dq[e, B + b] = 0; loss_row[b] = mean_e (q[e, b] - y_b)^2
__global__ __launch_bounds__(256) void k_crossq_critic_loss(const float* __restrict__ q, const float* __restrict__ rew, const float* __restrict__ term,
                                                            const float* __restrict__ nlogp, const float* __restrict__ log_alpha,
                                                            float* __restrict__ dq, float* __restrict__ loss_row, int64_t B, int E, float gamma) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float mn = q[B + b];
  for (int e = 1; e < E; ++e) mn = fminf(mn, q[(int64_t)e * 2 * B + B + b]);
  const float yb = rew[b] + gamma * (1.0f - term[b]) * (mn - expf(log_alpha[0]) * nlogp[b]);
  const float gs = 2.0f / ((float)B * (float)E);
  float loss = 0.f;
  for (int e = 0; e < E; ++e) {
    const float d = q[(int64_t)e * 2 * B + b] - yb;
    dq[(int64_t)e * 2 * B + b] = gs * d;
    dq[(int64_t)e * 2 * B + B + b] = 0.f;
    loss = fmaf(d, d, loss);
  }
  loss_row[b] = loss / (float)E;
}
// One thread per transition (crossq.py:236-240): minq_row[b] = min_e qa[e, b]; seed[e, b] = -[qa[e, b] == min] / (B n_ties)
__global__ __launch_bounds__(256) void k_crossq_policy_seed(const float* __restrict__ qa, float* __restrict__ seed, float* __restrict__ minq_row,
                                                            int64_t B, int E) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float mn = qa[b];
  for (int e = 1; e < E; ++e) mn = fminf(mn, qa[(int64_t)e * B + b]);
  int ties = 0;
  for (int e = 0; e < E; ++e) ties += qa[(int64_t)e * B + b] == mn ? 1 : 0;
  const float s = -1.0f / ((float)B * (float)(ties > 0 ? ties : 1));
  for (int e = 0; e < E; ++e) seed[(int64_t)e * B + b] = qa[(int64_t)e * B + b] == mn ? s : 0.f;
  minq_row[b] = mn;
}

// what the three entry points check of the two descriptors and hp; qdesc == NULL: acting
static int cq_prologue(const char* fn, const rlx_mlp_desc* pdesc, const rlx_mlp_desc* qdesc, const rlx_crossq_hparams& hp, const float* states,
                       const float* next_states, EnsDims* d) {
  const std::string f(fn);
  int rc = cq_check_net(*pdesc, f + ": pdesc");
  if (!rc && qdesc) rc = cq_check_net(*qdesc, f + ": qdesc");
  if (!rc) rc = cq_check_hp(hp, f);
  if (rc) return rc;
  if (!qdesc) {
    RLX_REQUIRE(pdesc->out_dim % 2 == 0 && pdesc->out_dim / 2 <= 64, RLX_EINVAL, f + ": pdesc->out_dim must be 2 * act_dim, act_dim at most 64");
    return RLX_OK;
  }
  return ens_prologue(fn, *pdesc, *qdesc, 1, "must be 1", states, next_states, hp.critic_states, hp.critic_next_states, d);
}
// the noise of a sample: the injected block (rlx_dbg_set_sac_noise) or normal(subkey, (B, A)) drawn into `noise`
static int cq_noise(const float* inject, float* noise, int64_t n, const uint32_t sub[2], int scheme, const float** eps, hipStream_t st) {
  *eps = inject ? inject : noise;
  return inject ? RLX_OK : launch_normal_noise(noise, n, sub[0], sub[1], scheme, st);
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int64_t rlx_crossq_param_count(const rlx_mlp_desc* desc) { return desc ? cq_layout(*desc).n_params : -1; }
int64_t rlx_crossq_stats_count(const rlx_mlp_desc* desc) { return desc ? cq_layout(*desc).n_stats : -1; }

int rlx_crossq_act_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, const float* pparams, const float* pstats, const float* obs, int64_t N,
                       uint32_t key_io[2], int scheme, float* action, int deterministic, const rlx_crossq_hparams* hp, void* stream) {
  RLX_REQUIRE(ctx && pdesc && pparams && pstats && obs && key_io && action && hp, RLX_EINVAL, "rlx_crossq_act_f32: NULL pointer");
  RLX_REQUIRE(N > 0, RLX_EINVAL, "rlx_crossq_act_f32: N must be positive");
  RLX_REQUIRE(scheme == RLX_THREEFRY_LEGACY || scheme == RLX_THREEFRY_PARTITIONABLE, RLX_EINVAL, "rlx_crossq_act_f32: unknown threefry scheme");
  int rc = cq_prologue("rlx_crossq_act_f32", pdesc, nullptr, *hp, nullptr, nullptr, nullptr);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const CqNet LP = cq_layout(*pdesc);
  const int A = LP.out / 2;
  CqBufs bp;
  float *xs, *h, *noise, *logp;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    cq_carve(ctx, LP, 1, N, false, a, &bp);
    xs = a.take((size_t)N * LP.ld0);
    h = a.take((size_t)N * 2 * A);
    noise = a.take((size_t)N * A);
    logp = a.take(N);
  });
  if (rc) return rc;
  ExactDwScope exact(ctx);
  bx_release_all(ctx);
  uint32_t key[2] = {key_io[0], key_io[1]}, sub[2];
  next_key(key, sub, 1, scheme);
  const BrnCfg cfg{hp->brn_momentum, hp->brn_eps, hp->brn_r_max, hp->brn_d_max};
  rc = fs_concat(obs, LP.in, nullptr, 0, xs, LP.ld0, N, st);
  if (!rc) rc = cq_fwd(ctx, LP, pparams, const_cast<float*>(pstats), 1, xs, N, bp, false, false, cfg, h, st);
  const float* eps = nullptr;
  if (!rc && deterministic) {   // tanh(mean): a block of zeros for the draw
    eps = noise;
    rc = ens_fill(noise, N * A, 0.f, st);
  } else if (!rc) {
    rc = cq_noise(nullptr, noise, N * A, sub, scheme, &eps, st);   // (acting ignores rlx_dbg_set_sac_noise: its blocks are [B, A])
  }
  if (rc) return rc;
  SacSampleArgs sa;
  sa.mode = 1; sa.ld_out = A; sa.col_off = 0; sa.A = A; sa.ls_min = hp->log_std_min; sa.ls_max = hp->log_std_max; sa.N_global = N;
  sa.act_out = action; sa.logp = logp; sa.eps_inject = eps;
  rc = ens_sample(h, sa, EnsRowKeys{0u, 0u, scheme, 0u, 0u, 1u}, N, st);
  if (rc) return rc;
  key_io[0] = key[0];
  key_io[1] = key[1];
  return RLX_OK;
}

int rlx_crossq_critic_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, const float* pparams, const float* pstats, const rlx_mlp_desc* qdesc,
                                 float* qparams, float* qm, float* qv, float* qstats, const float* log_alpha, const float* states,
                                 const float* next_states, const float* actions, const float* rewards, const float* terminations, int64_t B,
                                 uint32_t key_io[2], int scheme, int64_t* q_opt_count_io, const rlx_crossq_hparams* hp, float* metrics_out,
                                 void* stream) {
  const char* fn = "rlx_crossq_critic_update_f32";
  RLX_REQUIRE(ctx && pdesc && pparams && pstats && qdesc && qparams && qm && qv && qstats && log_alpha && states && next_states && actions &&
                  rewards && terminations && key_io && q_opt_count_io && hp && metrics_out,
              RLX_EINVAL, "rlx_crossq_critic_update_f32: NULL pointer");
  RLX_REQUIRE(B >= 2, RLX_EINVAL, "rlx_crossq_critic_update_f32: B must be at least 2 (one row has no batch variance)");
  RLX_REQUIRE(B <= 0x3fffffffLL, RLX_EUNSUP, "rlx_crossq_critic_update_f32: B at most 2^30 - 1");
  RLX_REQUIRE(scheme == RLX_THREEFRY_LEGACY || scheme == RLX_THREEFRY_PARTITIONABLE, RLX_EINVAL, "rlx_crossq_critic_update_f32: unknown threefry scheme");
  EnsDims d;
  int rc = cq_prologue(fn, pdesc, qdesc, *hp, states, next_states, &d);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int E = hp->ensemble_size, A = d.A;
  const int64_t M = 2 * B;
  const CqNet LP = cq_layout(*pdesc), LQ = cq_layout(*qdesc);
  CqBufs bp, bq;
  float *xq, *xs, *h, *noise, *lpn, *q, *dq, *loss_row, *gq;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    cq_carve(ctx, LP, 1, B, false, a, &bp);
    cq_carve(ctx, LQ, E, M, true, a, &bq);
    xq = a.take((size_t)M * d.ldc);
    xs = a.take((size_t)B * d.ldp);
    h = a.take((size_t)B * 2 * A);
    noise = a.take((size_t)B * A);
    for (float** x : {&lpn, &loss_row}) *x = a.take(B);
    for (float** x : {&q, &dq}) *x = a.take((size_t)E * M);
    gq = a.take((size_t)E * LQ.n_params);
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc) return rc;
  if (!sq) return RLX_ENOMEM;
  bx_release_all(ctx);
  BxReleaseAll bx_all{ctx};
  {
    const CqNetRef nets[2] = {{pparams, &LP, 1, B, false}, {qparams, &LQ, E, M, true}};
    rc = cq_images(ctx, nets, 2, st);
    if (rc) return rc;
  }
  GradScaleScope gscale(ctx, bx_grad_scale(B * E));   // |d loss / d q| is ~ 2 |q - y| / (B E)
  uint32_t key[2] = {key_io[0], key_io[1]}, sub[2];
  next_key(key, sub, 1, scheme);
  const BrnCfg cfg{hp->brn_momentum, hp->brn_eps, hp->brn_r_max, hp->brn_d_max};
  const bool warmed = *q_opt_count_io >= (int64_t)hp->brn_warmup_steps;
  // [(s, a); (s', a')]: a' ~ pi(s') from the policy in eval mode, into the lower half's action columns
  rc = fs_concat(d.cs, d.Oc, actions, A, xq, d.ldc, B, st);
  if (!rc) rc = fs_concat(d.cn, d.Oc, nullptr, A, xq + (size_t)B * d.ldc, d.ldc, B, st);
  if (!rc) rc = fs_concat(next_states, d.Op, nullptr, 0, xs, d.ldp, B, st);
  if (!rc) rc = cq_fwd(ctx, LP, pparams, const_cast<float*>(pstats), 1, xs, B, bp, false, false, cfg, h, st);
  const float* eps = nullptr;
  if (!rc) rc = cq_noise(ctx->dbg_sac_eps[0], noise, B * A, sub, scheme, &eps, st);
  if (rc) return rc;
  SacSampleArgs sa = ens_sample_args(d, hp->log_std_min, hp->log_std_max, B);
  sa.act_out = xq + (size_t)B * d.ldc; sa.logp = lpn; sa.eps_inject = eps;
  rc = ens_sample(h, sa, EnsRowKeys{0u, 0u, scheme, 0u, 0u, 1u}, B, st);
  // the joint pass, the loss, the backward over all 2 B rows
  if (!rc) rc = cq_fwd(ctx, LQ, qparams, qstats, E, xq, M, bq, true, warmed, cfg, q, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_crossq_critic_loss, dim3(div_up(B, 256)), dim3(256), 0, st, (const float*)q, rewards, terminations, (const float*)lpn,
                     log_alpha, dq, loss_row, B, E, hp->gamma);
  RLX_LAUNCH_CHECK();
  rc = ens_mean(loss_row, B, metrics_out + 0, st);
  if (!rc) rc = cq_bwd(ctx, LQ, qparams, qstats, E, xq, M, bq, true, cfg, dq, gq, st);
  const PlainAdamHp ahp{0.f, hp->critic_adam_b1, hp->adam_b2, hp->adam_eps};
  if (!rc) rc = torch_clip_adam(qparams, gq, qm, qv, (int64_t)E * LQ.n_params, sq, *q_opt_count_io + 1, hp->lr_critic, ahp, metrics_out + 7, st);
  if (rc) return rc;
  key_io[0] = key[0];
  key_io[1] = key[1];
  *q_opt_count_io += 1;
  return RLX_OK;
}

int rlx_crossq_policy_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, float* pstats,
                                 const rlx_mlp_desc* qdesc, const float* qparams, const float* qstats, float* log_alpha, float* am, float* av,
                                 const float* states, int64_t B, uint32_t key_io[2], int scheme, int64_t* pi_opt_count_io,
                                 const rlx_crossq_hparams* hp, float* metrics_out, void* stream) {
  const char* fn = "rlx_crossq_policy_update_f32";
  RLX_REQUIRE(ctx && pdesc && pparams && pm && pv && pstats && qdesc && qparams && qstats && log_alpha && am && av && states && key_io &&
                  pi_opt_count_io && hp && metrics_out,
              RLX_EINVAL, "rlx_crossq_policy_update_f32: NULL pointer");
  RLX_REQUIRE(B >= 2, RLX_EINVAL, "rlx_crossq_policy_update_f32: B must be at least 2 (one row has no batch variance)");
  RLX_REQUIRE(B <= 0x3fffffffLL, RLX_EUNSUP, "rlx_crossq_policy_update_f32: B at most 2^30 - 1");
  RLX_REQUIRE(scheme == RLX_THREEFRY_LEGACY || scheme == RLX_THREEFRY_PARTITIONABLE, RLX_EINVAL, "rlx_crossq_policy_update_f32: unknown threefry scheme");
  EnsDims d;
  // (the policy update reads one observation set: hp->critic_states alone serves the critics, critic_next_states only marks the pair)
  int rc = cq_prologue(fn, pdesc, qdesc, *hp, states, states, &d);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int E = hp->ensemble_size, A = d.A;
  const CqNet LP = cq_layout(*pdesc), LQ = cq_layout(*qdesc);
  CqBufs bp, bq;
  float *xp, *xs, *h, *dpi, *noise, *lpc, *qa, *seed, *q_row, *gp;
  rc = arena_carve(ctx, SL_SAC, [&](Arena& a) {
    cq_carve(ctx, LP, 1, B, true, a, &bp);
    cq_carve(ctx, LQ, E, B, false, a, &bq);
    xp = a.take((size_t)B * d.ldc);
    xs = a.take((size_t)B * d.ldp);
    for (float** x : {&h, &dpi}) *x = a.take((size_t)B * 2 * A);
    noise = a.take((size_t)B * A);
    for (float** x : {&lpc, &q_row}) *x = a.take(B);
    for (float** x : {&qa, &seed}) *x = a.take((size_t)E * B);
    gp = a.take(LP.n_params);
  });
  float* sq = (float*)scratch(ctx, SL_NORM, REDUCE_MAX_BLOCKS * sizeof(float));
  if (rc) return rc;
  if (!sq) return RLX_ENOMEM;
  bx_release_all(ctx);
  BxReleaseAll bx_all{ctx};
  {
    const CqNetRef nets[2] = {{pparams, &LP, 1, B, true}, {qparams, &LQ, E, B, true}};
    rc = cq_images(ctx, nets, 2, st);
    if (rc) return rc;
  }
  GradScaleScope gscale(ctx, bx_grad_scale(B));       // the seeds and the policy's head gradient are ~ 1 / B per sample
  uint32_t key[2] = {key_io[0], key_io[1]}, sub[2];
  next_key(key, sub, 1, scheme);
  const BrnCfg cfg{hp->brn_momentum, hp->brn_eps, hp->brn_r_max, hp->brn_d_max};
  const bool warmed = *pi_opt_count_io >= (int64_t)hp->brn_warmup_steps;
  // a ~ pi(s) from the policy in train mode, into the critics' input [cobs | a]
  rc = fs_concat(d.cs, d.Oc, nullptr, A, xp, d.ldc, B, st);
  if (!rc) rc = fs_concat(states, d.Op, nullptr, 0, xs, d.ldp, B, st);
  if (!rc) rc = cq_fwd(ctx, LP, pparams, pstats, 1, xs, B, bp, true, warmed, cfg, h, st);
  const float* eps = nullptr;
  if (!rc) rc = cq_noise(ctx->dbg_sac_eps[1], noise, B * A, sub, scheme, &eps, st);
  if (rc) return rc;
  SacSampleArgs sa = ens_sample_args(d, hp->log_std_min, hp->log_std_max, B);
  sa.act_out = xp; sa.logp = lpc; sa.eps_inject = eps;
  const EnsRowKeys nokeys{0u, 0u, scheme, 0u, 0u, 1u};
  rc = ens_sample(h, sa, nokeys, B, st);
  // the critics in eval mode, the seed under the minimum, their input gradients on the action columns
  if (!rc) rc = cq_fwd(ctx, LQ, qparams, const_cast<float*>(qstats), E, xp, B, bq, false, false, cfg, qa, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_crossq_policy_seed, dim3(div_up(B, 256)), dim3(256), 0, st, (const float*)qa, seed, q_row, B, E);
  RLX_LAUNCH_CHECK();
  rc = cq_bwd(ctx, LQ, qparams, qstats, E, xp, B, bq, false, cfg, seed, nullptr, st);
  if (!rc) rc = ens_policy_grad(h, xp, d.ldc, d.Oc, bq.N[0], d.ldc, (int64_t)B * d.ldc, E, log_alpha, nokeys, dpi, B, A, hp->log_std_min,
                                hp->log_std_max, eps, st);
  if (!rc) rc = cq_bwd(ctx, LP, pparams, pstats, 1, xs, B, bp, true, cfg, dpi, gp, st);
  if (rc) return rc;
  // metrics, alpha's and the policy's plain Adam steps at the policy counter
  const int64_t pstep = *pi_opt_count_io + 1;
  float sched[3];
  adam_schedule_entry(sched, pstep, hp->lr_alpha, hp->alpha_adam_b1, hp->adam_b2);
  rc = ens_finish(q_row, B, lpc, B, nullptr, 0, log_alpha, am, av, metrics_out, hp->target_entropy, sched, hp->alpha_adam_b1, hp->adam_b2,
                  hp->adam_eps, st);
  const PlainAdamHp ahp{0.f, hp->policy_adam_b1, hp->adam_b2, hp->adam_eps};
  if (!rc) rc = torch_clip_adam(pparams, gp, pm, pv, LP.n_params, sq, pstep, hp->lr_policy, ahp, metrics_out + 6, st);
  if (rc) return rc;
  key_io[0] = key[0];
  key_io[1] = key[1];
  *pi_opt_count_io += 1;
  return RLX_OK;
}

}  // extern "C"
