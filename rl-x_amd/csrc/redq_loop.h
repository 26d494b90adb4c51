// redq_loop.h -- the high update-to-data `update` redq.hip, droq.hip and aqe.hip share (redq_loop, defined in redq.hip, whose header
// describes the schedule): G critic steps on G fresh batches, each followed by plain Adam of all E critics and Polyak, then one
// policy / entropy step.  What an algorithm sets is a RedqLoopSpec: the critic chain (its norm and dropout rate) and head width, where
// a step's keys sit in its split (REDQ and AQE have one key per row, DroQ three in a critic step and two in the policy step), which
// targets a critic step evaluates, the critic loss, the value the policy ascends, and the hyper-parameter check.
#pragma once
#include "sac_ens.h"

namespace rlx {

constexpr int REDQ_MAXE = 16;
constexpr int REDQ_MAXG = 64;

// the values a critic loss reads: q [E][B][H] from the online critics and qn [M][B][H] from the M evaluated targets, of whose M H
// values per transition K enter the target (AQE: the K lowest of the pool; REDQ and DroQ take the minimum of M at H = 1)
struct RedqLossDims { int E, H, M, K; };
struct RedqLoopSpec;
// y [B], dq [E][B][H] = d loss / d q, loss_row [B]; loss_out [1] = the mean of loss_row
typedef int (*RedqLossFn)(const float* q, const float* qn, const float* rew, const float* term, const float* nlogp, const float* log_alpha,
                          int64_t B, const RedqLossDims& n, float gamma, float* y, float* dq, float* loss_row, float* loss_out, hipStream_t st);
typedef int (*RedqCheckHpFn)(const rlx_redq_hparams& hp, const RedqLoopSpec& spec);

struct RedqKeySlot { uint32_t base, stride; };   // row b's key of one use: split(step_key, count)[base + stride b]
struct RedqLoopSpec {
  const char* fn;     // the entry point's name, in front of its messages
  const char* algo;   // "redq" / "droq" / "aqe", in front of the descriptor and hyper-parameter messages
  int critic_norm;    // the critics' hidden blocks: NORM_NONE (Dense -> ReLU) or NORM_LAYER (Dense -> Dropout -> LayerNorm -> ReLU)
  float critic_eps, critic_drop;
  int heads;                 // H = qdesc->out_dim, the outputs of one critic: a transition has T = E H values
  const char* heads_rule;    // how the message on qdesc->out_dim states it
  int dropped;               // of the targets' pooled values the K = M H - dropped lowest are kept (0 where the loss takes the minimum)
  // a critic step's targets: a random M-subset (sample_key = keys[1] of its split, the rows' keys from 2 on) or, without one, all E
  // in index order (no sample_key and no host shuffle: the rows' keys from 1 on, one key fewer in the split)
  bool target_subset;
  // the policy ascends the minimum over the E critics (k_redq_policy_seed: the gradient to the minimising critic, seeds ~ 1 / B,
  // q_value the mean of the row minima) or the mean over all T values (the constant seed -1 / (B T), q_value the mean over B T)
  bool policy_min;
  RedqCheckHpFn check_hp;    // redq_check_hp_of, or the algorithm's own over hp, `heads` and `dropped`
  RedqLossFn critic_loss;
  uint32_t critic_keys_per_row, policy_keys_per_row;   // a critic step splits its key critic_keys_per_row B + 2 ways (key, sample_key,
                                                       // the rows' keys; + 1 without a subset), the policy step policy_keys_per_row B + 1
                                                       // ways (key, the rows')
  RedqKeySlot next_noise, online_drop, target_drop;    // critic step: a' ~ pi(s'), the E online critics' and the M targets' dropout
  RedqKeySlot cur_noise, policy_drop;                  // policy step: a~ ~ pi(s_0), the E critics' dropout on (s_0, a~)
};

// ensemble_size E, in_target_minimization_size M, q_update_steps G (redq/flax/default_config.py:18-20)
int redq_check_hp(const rlx_redq_hparams& hp, const char* algo);
inline int redq_check_hp_of(const rlx_redq_hparams& hp, const RedqLoopSpec& spec) { return redq_check_hp(hp, spec.algo); }
// REDQ's and DroQ's critic loss: the minimum over the M selected targets, the mean over batch and ensemble (n.H = 1)
int redq_critic_loss(const float* q, const float* qn, const float* rew, const float* term, const float* nlogp, const float* log_alpha,
                     int64_t B, const RedqLossDims& n, float gamma, float* y, float* dq, float* loss_row, float* loss_out, hipStream_t st);

// rlx_redq_update_f32's arguments (include/rlx_hip.h) under the layout of `spec`; without a target subset hp->
// in_target_minimization_size is ensemble_size and subsets_out NULL
int redq_loop(rlx_ctx* ctx, const RedqLoopSpec& spec, const rlx_mlp_desc* pdesc, float* pparams, float* pm, float* pv,
              const rlx_mlp_desc* qdesc, float* qparams, float* qm, float* qv, float* qtarget, float* log_alpha, float* am, float* av,
              const float* states, const float* next_states, const float* actions, const float* rewards, const float* terminations,
              int64_t B, uint32_t key_io[2], int scheme, int64_t* q_opt_count_io, int64_t* pi_opt_count_io, const rlx_redq_hparams* hp,
              float* metrics_out, int32_t* subsets_out, void* stream);

}  // namespace rlx
