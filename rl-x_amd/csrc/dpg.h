// dpg.h -- what the deterministic-policy-gradient updates share (fasttd3.hip, td3.hip): the backward of the policy's tanh head from
// the critics' input gradients.  The kernel and its launcher are in td3.hip.
#pragma once
#include "net_pass.h"

namespace rlx {

// d loss / d head [M, A] of the policy through its tanh: (da1 + da2) (1 - a^2), a = the action the critics saw (their input
// columns [c0, c0 + A), row stride lda), da_k = the critics' input gradients on those columns; da2 == NULL: one critic, da1 alone
int dpg_tanh_bwd(const float* x, const float* da1, const float* da2, int lda, int c0, float* dhead, int64_t M, int A, hipStream_t st);

}  // namespace rlx
