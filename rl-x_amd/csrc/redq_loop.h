// redq_loop.h -- the high update-to-data `update` redq.hip and droq.hip share (redq_loop, defined in redq.hip with its kernels):
// G critic steps on G fresh batches, each followed by plain Adam of all E critics and Polyak, then one policy / entropy step.  What
// an algorithm sets is the critic chain (its norm and dropout rate) and where a step's keys sit in its split: REDQ has one key per
// row, DroQ three in a critic step and two in the policy step.  The schedule, the arithmetic and the launch order are redq.hip's.
#pragma once
#include "sac_ens.h"

namespace rlx {

constexpr int REDQ_MAXE = 16;
constexpr int REDQ_MAXG = 64;

struct RedqKeySlot { uint32_t base, stride; };   // row b's key of one use: split(step_key, count)[base + stride b]
struct RedqLoopSpec {
  const char* fn;     // the entry point's name, in front of its messages
  const char* algo;   // "redq" / "droq", in front of the descriptor and hyper-parameter messages
  int critic_norm;    // the critics' hidden blocks: NORM_NONE (Dense -> ReLU) or NORM_LAYER (Dense -> Dropout -> LayerNorm -> ReLU)
  float critic_eps, critic_drop;
  uint32_t critic_keys_per_row, policy_keys_per_row;   // a critic step splits its key critic_keys_per_row B + 2 ways (key, sample_key,
                                                       // the rows' keys), the policy step policy_keys_per_row B + 1 ways (key, the rows')
  RedqKeySlot next_noise, online_drop, target_drop;    // critic step: a' ~ pi(s'), the E online critics' and the M targets' dropout
  RedqKeySlot cur_noise, policy_drop;                  // policy step: a~ ~ pi(s_0), the E critics' dropout on (s_0, a~)
};

// ensemble_size E, in_target_minimization_size M, q_update_steps G (redq/flax/default_config.py:18-20)
int redq_check_hp(const rlx_redq_hparams& hp, const char* algo);

// rlx_redq_update_f32's arguments (include/rlx_hip.h) under the layout of `spec`
int redq_loop(rlx_ctx* ctx, const RedqLoopSpec& spec, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
              const rlx_mlp_desc* qdesc, float* qparams, float* qm, float* qv, float* qtarget, float* log_alpha, float* am, float* av,
              const float* states, const float* next_states, const float* actions, const float* rewards, const float* terminations,
              int64_t B, uint32_t key_io[2], int scheme, int64_t* q_opt_count_io, int64_t* pi_opt_count_io, const rlx_redq_hparams* hp,
              float* metrics_out, int32_t* subsets_out, void* stream);

}  // namespace rlx
