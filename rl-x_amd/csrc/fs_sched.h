// fs_sched.h -- the stream fork / join of the twin-critic off-policy updates (fastsac.hip, fasttd3.hip, td3.hip: a critic pair whose two
// halves go to two streams; espo.hip: the critic step of an epoch) and the deferred parameter-gradient reduction (those three,
// reppo.hip and mpo.hip: the backward passes of a step gather all their slab partials into one reduction launch).  Nothing here
// touches the arithmetic; the epilogue rule of the input gradients is net_pass.h's, which includes this file.
#pragma once
#include "mlp.h"
#include "gemm_bx.h"

namespace rlx {

// Fork / join of the update's two independent halves (critic 1 || critic 2; target passes || online passes): the side half runs
// on ctx->side under scratch bank 1.  With option two_streams = 0 both halves stay on the caller's stream.
struct FsFork {
  rlx_ctx* c;
  hipStream_t main_st, side_st;
  bool on;
  int next_ev = 0;
  FsFork(rlx_ctx* ctx, hipStream_t st) : c(ctx), main_st(st), side_st(st), on(false) {}
  int begin() {
    if (!c->two_streams) return RLX_OK;
    const int rc = ctx_sac_streams(c);
    if (rc) return rc;
    side_st = c->side;
    on = side_st != main_st;
    return RLX_OK;
  }
  int fork() {   // the side stream sees everything issued on the main stream so far
    if (!on) return RLX_OK;
    hipEvent_t e = c->sac_ev[next_ev++ % 6];
    RLX_HIP_TRY(hipEventRecord(e, main_st));
    RLX_HIP_TRY(hipStreamWaitEvent(side_st, e, 0));
    return RLX_OK;
  }
  int join() {   // the main stream waits for the side stream
    c->bank = 0;
    if (!on) return RLX_OK;
    hipEvent_t e = c->sac_ev[next_ev++ % 6];
    RLX_HIP_TRY(hipEventRecord(e, side_st));
    RLX_HIP_TRY(hipStreamWaitEvent(main_st, e, 0));
    return RLX_OK;
  }
  hipStream_t side() { c->bank = on ? 1 : 0; return side_st; }   // (sets the scratch bank the following launches use)
  hipStream_t main() { c->bank = 0; return main_st; }
  ~FsFork() { c->bank = 0; }
};

// One reduction launch for ALL the parameter-gradient partials of an update's backward passes (head slabs, LayerNorm scale /
// bias partials, weight-gradient slabs of every layer of every network): 14 launches of ~12 us per FastSAC network otherwise.
struct FsDefer {
  rlx_ctx* c;
  ReduceDefer d;
  explicit FsDefer(rlx_ctx* ctx) : c(ctx) {}
  int begin(size_t floats) {
    d.base = (float*)scratch(c, SL_STAGE, floats * sizeof(float));
    if (!d.base) return RLX_ENOMEM;
    d.cap = floats;
    d.off = 0;
    d.tab.n = 0;
    c->defer = &d;
    return RLX_OK;
  }
  int finish(hipStream_t st) { return stage_reduce_flush(c, nullptr, nullptr, st); }   // the one reduction launch
  ~FsDefer() { if (c->defer == &d) c->defer = nullptr; }
};
// FsDefer plus the split-operand gradient scale of a pass over `rows` rows, for the scope's lifetime
struct BwdPass : FsDefer {
  GradScaleScope gscope;
  BwdPass(rlx_ctx* ctx, int64_t rows) : FsDefer(ctx), gscope(ctx, bx_grad_scale(rows)) {}
};

}  // namespace rlx
