// droq.hip -- DroQ, dropout Q-functions (rl_x/algorithms/droq/flax/droq.py:144-261): REDQ's high update-to-data `update` over critics
// whose hidden blocks are Dense -> Dropout -> LayerNorm -> ReLU (droq/flax/critic.py:25-35), by default two of them.  The update is
// redq.hip's redq_loop (redq_loop.h; redq.hip's header describes the schedule) -- target min over the M selected networks, the loss mean over batch and ensemble, plain Adam and
// Polyak per step over the whole flat critic vector (LayerNorm parameters included), the policy loss on the min over all E with
// the tie split, two counters, metrics [10] -- with what differs stated as a RedqLoopSpec:
//   critic   make_chain(..., NORM_LAYER, RLX_ACT_RELU, 1e-6f, dropout_rate): per hidden block W, b, LN scale, LN bias, then the head W,
//            b; a block's Dropout -> LayerNorm -> ReLU is ONE launch, k_drop_ln_relu (dense_head.hip), forward and backward
//   keys     critic step i: keys = split(key, 3 B + 2), key = keys[0], sample_key = keys[1]; row b: next-action noise keys[2 + 3 b],
//            the online critics' dropout keys[3 + 3 b], the selected targets' keys[4 + 3 b] (droq.py:229-230, :236); policy step: keys
//            = split(key, 2 B + 1), key = keys[0], row b's noise keys[1 + 2 b], the critics' dropout keys[2 + 2 b] (:247-250)
//   dropout  active in EVERY critic pass (critic.py:28, :32: deterministic=False), the targets' and the policy step's input-gradient
//            passes included; a backward pass regenerates the mask of its forward pass from the same keys: no mask is stored
//   masks    the project's own stream from the reference's per-row keys (sac_sample.h: droq_layer_key)
// Two small entry points let a test look at the mask stream and at the fused block on their own.
// CPU twin: tests/droq_twin.py (float64).  The reference's DroQ is JAX only; see DESIGN.md 4.5g for what is pinned.
#include "redq_loop.h"

namespace rlx {

constexpr int DROQ_MAX_WIDTH = 768;   // what the row-norm kernels hold (norm_act)

// flags[b, u] = 1 iff unit u of row b is kept: one thread per element through the whole stream (droq_keep_at)
__global__ __launch_bounds__(256) void k_droq_mask(uint8_t* __restrict__ flags, int64_t B, int D, DropKeys dk, float keep) {
  const int64_t n = B * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / D;
    const uint32_t u = (uint32_t)(i - b * D);
    flags[i] = droq_keep_at(dk.k0, dk.k1, dk.scheme, dk.base + dk.stride * (uint32_t)b, dk.count, (uint32_t)dk.j, (uint32_t)dk.E,
                            (uint32_t)dk.l, (uint32_t)dk.L, u, (uint32_t)D, keep) ? 1 : 0;
  }
}

// what both test entry points check of a mask's address; fn: the entry point's name
static int droq_check_keys(const std::string& fn, const uint32_t* key, int scheme, uint32_t base, uint32_t stride, uint32_t count, int j,
                           int E, int l, int L, int64_t B, int D, float rate) {
  RLX_REQUIRE(key, RLX_EINVAL, fn + ": key is NULL");
  RLX_REQUIRE(scheme == RLX_THREEFRY_LEGACY || scheme == RLX_THREEFRY_PARTITIONABLE, RLX_EINVAL, fn + ": unknown threefry scheme");
  RLX_REQUIRE(B > 0, RLX_EINVAL, fn + ": the row count must be positive");
  RLX_REQUIRE(D > 0 && D % 64 == 0 && D <= DROQ_MAX_WIDTH, RLX_EUNSUP, fn + ": D must be a multiple of 64, at most 768");
  RLX_REQUIRE(rate >= 0.f && rate < 1.f, RLX_EINVAL, fn + ": rate must be in [0, 1)");
  RLX_REQUIRE(E >= 1 && j >= 0 && j < E && L >= 1 && l >= 0 && l < L, RLX_EINVAL, fn + ": needs 0 <= j < E and 0 <= l < L");
  RLX_REQUIRE(count <= 0x7fffffffu && (uint64_t)base + (uint64_t)stride * (uint64_t)(B - 1) < (uint64_t)count, RLX_EINVAL,
              fn + ": base + stride (B - 1) must be below count <= 2^31 - 1");
  return RLX_OK;
}

}  // namespace rlx

using namespace rlx;

extern "C" {

int rlx_droq_mask_u8(rlx_ctx* ctx, const uint32_t key[2], int scheme, uint32_t base, uint32_t stride, uint32_t count, int j, int E, int l,
                     int L, int64_t B, int D, float rate, uint8_t* flags_out, void* stream) {
  RLX_REQUIRE(ctx && flags_out, RLX_EINVAL, "rlx_droq_mask_u8: ctx / flags_out is NULL");
  const int rc = droq_check_keys("rlx_droq_mask_u8", key, scheme, base, stride, count, j, E, l, L, B, D, rate);
  if (rc) return rc;
  const DropKeys dk{key[0], key[1], scheme, base, stride, count, j, E, l, L};
  hipLaunchKernelGGL(k_droq_mask, dim3(elem_grid(B * D)), dim3(256), 0, (hipStream_t)stream, flags_out, B, D, dk, 1.0f - rate);
  RLX_LAUNCH_CHECK();
  return RLX_OK;
}

int rlx_droq_block_f32(rlx_ctx* ctx, const float* Z, float* H_io, const float* scale_bias, const uint32_t key[2], int scheme, uint32_t base,
                       uint32_t stride, uint32_t count, int j, int E, int l, int L, int64_t M, int D, float rate, int backward, float* dg_out,
                       float* db_out, void* stream) {
  RLX_REQUIRE(ctx && Z && H_io && scale_bias, RLX_EINVAL, "rlx_droq_block_f32: NULL pointer (ctx, Z, H_io, scale_bias)");
  RLX_REQUIRE(!backward || (dg_out && db_out), RLX_EINVAL, "rlx_droq_block_f32: the backward needs dg_out and db_out");
  const int rc = droq_check_keys("rlx_droq_block_f32", key, scheme, base, stride, count, j, E, l, L, M, D, rate);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const Block o{D, D, 0, 0, 0, D, NORM_LAYER, RLX_ACT_RELU, 1e-6f, rate};   // (only g, be, the kind and the rate are read)
  const DropKeys dk{key[0], key[1], scheme, base, stride, count, j, E, l, L};
  if (!backward) return norm_act(o, scale_bias, Z, H_io, nullptr, rows_grid(ctx, M), M, st, &dk);
  const int grid = bwd_rows_grid(ctx, M);
  float* part = stage_alloc(ctx, (size_t)grid * norm_part_width(o));
  if (!part) return RLX_ENOMEM;
  const int rc2 = norm_act(o, scale_bias, Z, H_io, part, grid, M, st, &dk);
  return rc2 ? rc2 : norm_bwd_reduce(ctx, part, grid, D, dg_out, db_out, st);
}

int rlx_droq_update_f32(rlx_ctx* ctx, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv, const rlx_mlp_desc* qdesc,
                        float* qparams, float* qm, float* qv, float* qtarget, float* log_alpha, float* am, float* av, const float* states,
                        const float* next_states, const float* actions, const float* rewards, const float* terminations, int64_t B,
                        uint32_t key_io[2], int scheme, int64_t* q_opt_count_io, int64_t* pi_opt_count_io, const rlx_droq_hparams* hp,
                        float* metrics_out, int32_t* subsets_out, void* stream) {
  RLX_REQUIRE(hp && qdesc, RLX_EINVAL, "rlx_droq_update_f32: NULL pointer");
  RLX_REQUIRE(hp->dropout_rate >= 0.f && hp->dropout_rate < 1.f, RLX_EINVAL, "rlx_droq_update_f32: hp->dropout_rate must be in [0, 1)");
  for (int l = 0; l < qdesc->n_hidden && l < 4; ++l)
    RLX_REQUIRE(qdesc->hidden[l] <= DROQ_MAX_WIDTH, RLX_EUNSUP,
                "rlx_droq_update_f32: qdesc hidden widths at most 768 (the LayerNorm kernels hold a row in one wave)");
  const rlx_redq_hparams rhp{hp->gamma, hp->tau, hp->target_entropy, hp->log_std_min, hp->log_std_max, hp->lr_policy, hp->lr_critic,
                             hp->lr_critic_delta, hp->lr_alpha, hp->adam_b1, hp->adam_b2, hp->adam_eps, hp->ensemble_size,
                             hp->in_target_minimization_size, hp->q_update_steps, hp->critic_states, hp->critic_next_states};
  // three keys per row in a critic step (noise, online dropout, target dropout), two in the policy step (noise, dropout)
  const RedqLoopSpec spec{"rlx_droq_update_f32", "droq", NORM_LAYER, 1e-6f, hp->dropout_rate, 1, "must be 1", 0, true, true, redq_check_hp_of,
                          redq_critic_loss, 3u, 2u, {2u, 3u}, {3u, 3u}, {4u, 3u}, {1u, 2u}, {2u, 2u}};
  return redq_loop(ctx, spec, pdesc, pparams, pm, pv, qdesc, qparams, qm, qv, qtarget, log_alpha, am, av, states, next_states, actions,
                   rewards, terminations, B, key_io, scheme, q_opt_count_io, pi_opt_count_io, &rhp, metrics_out, subsets_out, stream);
}

}  // extern "C"
