"""GPU: recurrent PPO (ppo_lstm.hip, lstm_kernels.h, the decoder branch of k_rollout_step) against the float64 oracle
(oracle/ppo_lstm.py) over the shapes check_lstm_desc accepts: the sequence minibatch pass, the whole update past its first Adam step on
both stream schedules, the acting step over the corners of the fused decoder's envelope and just outside it, and the refusals.  The
cases, what each reaches and the bars: tests/ppo_lstm_cases.py; which GEMMs a case must run on which engine: the selection mirror in
tests/net_paths.py (ppo_lstm_pass), asserted here from the profiler rows.  tests/test_ppo_lstm_cases.py holds the cases' inputs to
half of each bar in float32 on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import net_paths as npth
import ppo_lstm_cases as lc
from oracle import nets
from rlx_amd.hip import PpoHparams, mlp_desc
from rlx_amd.hip import lib as L
from rlx_amd.hip.lib import lstm_policy_desc

pytestmark = pytest.mark.gpu

OPTION_DEFAULTS = {"gemm_bx": 1, "bx_debug": 0, "two_streams": 1, "fused_recurrent_act": 1}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _hp(mgn=0.5):
    hp = PpoHparams()
    hp.clip_range, hp.entropy_coef, hp.critic_coef, hp.max_grad_norm = lc.CLIP, lc.ENT, lc.VF, mgn
    hp.adam_b1, hp.adam_b2, hp.adam_eps = 0.9, 0.999, lc.ADAM_EPS
    return hp


def _ldesc(spec):
    return lstm_policy_desc(spec.O, spec.A, spec.E, spec.H, spec.torso, spec.share, 1 if spec.cell == "gru" else 0,
                            1 if spec.combine == "film" else 0)


def _cdesc(cs):
    return mlp_desc(cs.in_dim, cs.hidden, cs.out_dim, cs.act, cs.ln_first, cs.has_logstd)


def _ran(rows):
    return {(r["kernel"], r["engine"], r["M"], r["N"], r["K"]): r["launches"] for r in rows}


class _options:
    """set_option pairs around a call; the shared context gets its defaults back whatever happens"""

    def __init__(self, ctx, options):
        self.ctx, self.options = ctx, options

    def __enter__(self):
        for k, v in self.options.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.options:
            self.ctx.set_option(k, OPTION_DEFAULTS[k])


def _minibatch(ctx, dev, c, options, profile=True):
    pg, cg, met = torch.zeros(c.spec.n_params, device=dev), torch.zeros(c.cs.n_params, device=dev), torch.zeros(8, device=dev)
    dev_in = [_t(x, dev) for x in c.rollout] + [_t(c.env_idx, dev)]
    rows, open_ = None, False
    with _options(ctx, options):
        try:
            if profile:
                ctx.prof_begin()
                open_ = True
            ctx.ppo_lstm_minibatch_fwd_bwd(_ldesc(c.spec), _t(c.p, dev), pg, _cdesc(c.cs), _t(c.cp, dev), cg, met, *dev_in, _hp())
            torch.cuda.synchronize()
            if profile:
                open_ = False
                ctx.prof_end()
                rows = ctx.prof_rows()
        finally:
            if open_:                  # a refused or failed call: the shared context does not keep the profiler open
                ctx.prof_end()
    return met.cpu().numpy(), pg.cpu().numpy(), cg.cpu().numpy(), rows


def _report(tag, rows, blocks, whole):
    print(f"{tag} metrics (got, float64, allowed):", {k: tuple(float(f"{x:.6g}") for x in v) for k, v in rows.items()})
    worst = max((max(b[0] / b[1], b[2] / b[3]), k) for k, b in blocks.items())
    print(f"{tag} ||dg||/||g|| vs float64: policy {whole['policy']:.2e} critic {whole['critic']:.2e}; worst block {worst[1]} at "
          f"{worst[0]:.2f} of its bar")


@pytest.mark.parametrize("name,label", [(n, l) for n, l, _ in lc.RUNS])
def test_minibatch_pass_vs_float64_oracle(ctx, dev, name, label):
    c = lc.case(name)
    options = lc.run_options(name, label)
    expect = c.expect(options)
    met, gp, gc, prof = _minibatch(ctx, dev, c, options)
    ran = {k: v for k, v in _ran(prof).items() if k[0] in npth.GEMM_KERNELS}
    rows, blocks, whole = lc.compare(c.spec, c.T, c.ne, c.oracle, met, gp, gc)
    tag = f"recurrent shape {name} [{label}]"
    print(f"{tag} recurrent product: {expect['recurrent']}, full tiles: {expect['full_tiles']}; GEMM rows:", sorted(ran.items()))
    _report(tag, rows, blocks, whole)
    if c.T * c.ne >= npth.SPLIT_ROWS:
        # the GEMMs the selection mirror predicts, on the engines it predicts, with its launch counts -- and no others
        bad = {k: (ran.get(k), expect["rows"].get(k)) for k in set(ran) | set(expect["rows"]) if ran.get(k) != expect["rows"].get(k)}
        assert not bad, bad
        assert expect["split"] and any(k[1] == npth.ENGINE_SPLIT for k in ran)
    else:
        # below 4096 rows nothing runs on the split engine; the policy's GEMMs all show (the critic's may share a row with them)
        assert not any(k[1] == npth.ENGINE_SPLIT for k in ran), ran
        assert all(ran.get(k, 0) >= n for k, n in expect["rows"].items()), (expect["rows"], ran)
    lc.assert_within(rows, blocks, whole)


@pytest.mark.parametrize("name", lc.UPDATE_NAMES)
def test_whole_update_past_the_first_adam_step_on_both_schedules(ctx, dev, name):
    """T steps of N = 2 ne envs, two epochs: four updates from opt_count = 3 with non-zero Adam moments and global-norm clipping
    active, against the oracle loop (float64 autograd, float32 optimizer state) on the same env-index permutation -- on the default
    schedule (the critic and the torso's weight gradients on the side stream) and with two_streams = 0.  A buffer one stream overwrites
    while the other still reads it shows here, not in the single-stream minibatch entry."""
    u = lc.UPDATES[name].build()
    out, p_e, c_e = u.trajectory64
    n_upd = u.n_upd
    assert out[0]["gradients/policy_grad_norm"] > u.max_grad_norm and out[0]["gradients/critic_grad_norm"] > u.max_grad_norm   # clipping acts
    cols = {"loss/policy_gradient_loss": 0, "loss/critic_loss": 1, "loss/entropy_loss": 2, "policy_ratio/approx_kl": 3,
            "policy_ratio/clip_fraction": 4, "gradients/policy_grad_norm": 8, "gradients/critic_grad_norm": 9}
    exp = np.array([[o[k] for k in cols] for o in out])
    first_bars = [(rtol, atol) for _, rtol, atol in lc.METRICS] + [(0.0, 2.0 / (u.T * u.ne)), (1e-5, 0.0), (1e-5, 0.0)]
    lr = np.full(n_upd, lc.LR, np.float32)
    got_by_schedule = {}
    for two in (1, 0):
        P, C, pm, pv, cm, cv = (_t(x, dev) for x in (u.p, u.cp, u.pm, u.pv, u.cm, u.cv))
        met = torch.zeros(n_upd, 10, device=dev)
        with _options(ctx, {"two_streams": two}):
            key, cnt = ctx.ppo_lstm_update(_ldesc(u.spec), P, pm, pv, _cdesc(u.cs), C, cm, cv, *[_t(x, dev) for x in u.rollout],
                                           lc.UPD_EPOCHS, u.T * u.ne, u.key, lc.OPT_COUNT0, lr, _hp(u.max_grad_norm), met)
            torch.cuda.synchronize()
        assert np.array_equal(key, u.key_out) and cnt == lc.OPT_COUNT0 + n_upd
        got = met.cpu().numpy().astype(np.float64)[:, list(cols.values())]
        got_by_schedule[two] = got
        tag = f"recurrent update {name} [two_streams={two}]"
        print(f"{tag}: metrics |got - float64| / max(|float64|, 1e-3), per update:",
              [[float(f"{x:.1e}") for x in row] for row in np.abs(got - exp) / np.maximum(np.abs(exp), 1e-3)])
        for i, (rtol, atol) in enumerate(first_bars):
            np.testing.assert_allclose(got[0, i], exp[0, i], rtol=rtol, atol=atol, err_msg=list(cols)[i])
        later = [0, 1, 2, 3, 5, 6]
        np.testing.assert_allclose(got[:, later], exp[:, later], rtol=2e-3, atol=2e-5)
        for which, g, e, start in (("policy", P, p_e, u.p), ("critic", C, c_e, u.cp)):
            d = np.abs(g.cpu().numpy().astype(np.float64) - e)
            share = (d <= 2e-5 + 1e-3 * np.abs(e)).mean()
            print(f"{tag}: {which} parameters after {n_upd} updates: max |dp| {d.max():.2e}, within 2e-5 + 1e-3 |e|: {share:.6f}")
            assert share > 0.999, (which, d.max(), share)
            assert d.max() <= 2 * lc.LR * n_upd, (which, d.max())
            assert np.abs(e.astype(np.float64) - start).max() > 1e-4, which
    # the two schedules against each other, at the first update's bars
    a, b = got_by_schedule[1], got_by_schedule[0]
    for i, (rtol, atol) in enumerate(first_bars):
        np.testing.assert_allclose(a[0, i], b[0, i], rtol=rtol, atol=atol, err_msg=list(cols)[i])


# ---------------------------------------------------------------------------------------------------------------- the acting step
def _act(ctx, dev, a, fused, images):
    """one rlx_ppo_lstm_act_f32 call on the case -> (outputs dict, launches of k_rollout_step it made)"""
    n, A = a.n, a.A
    cd, hd = _t(a.c, dev), _t(a.h, dev)
    out = dict(action=torch.empty(n, A, device=dev), processed=torch.empty(n, A, device=dev), value=torch.empty(n, device=dev),
               logp=torch.empty(n, device=dev))
    Pd, Cd = _t(a.p, dev), _t(a.cp, dev)
    ld, cdsc = _ldesc(a.spec), _cdesc(a.cs)
    with _options(ctx, {"fused_recurrent_act": fused}):
        try:
            if images:      # the decoder's hidden layers on the fp16 pipe from images laid out once per rollout
                ctx.ppo_lstm_rollout_begin(ld, Pd, cdsc, Cd)
            else:           # explicitly: the context remembers images by parameter address, and the allocator reuses addresses
                ctx.rollout_end()
            before = ctx.get_counter("ro_step_launches")
            k2 = ctx.ppo_lstm_act(ld, Pd, cdsc, Cd, _t(a.obs, dev), cd, hd, a.key, out["action"], out["processed"], out["value"],
                                  out["logp"], clip_and_rescale=True, act_low=_t(a.lo, dev), act_high=_t(a.hi, dev),
                                  critic_obs=None if a.cobs is None else _t(a.cobs, dev))
            torch.cuda.synchronize()
            launches = ctx.get_counter("ro_step_launches") - before
        finally:
            ctx.rollout_end()
    assert np.array_equal(k2, a.key_out)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["c"], got["h"] = cd.cpu().numpy(), hd.cpu().numpy()
    return got, launches


def _act_check(a, got, worst):
    exp = dict(c=a.c2, h=a.h2, action=a.action, logp=a.logp, value=a.value, processed=a.processed)     # (GRU: c untouched)
    for k, (rtol, atol) in lc.ACT_BARS.items():
        frac = float((np.abs(got[k] - exp[k]) / (atol + rtol * np.abs(exp[k]))).max())
        worst[k] = max(worst.get(k, 0.0), frac)
        np.testing.assert_allclose(got[k], exp[k], rtol=rtol, atol=atol, err_msg=k)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("torso", lc.ACT_TORSO, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("E", lc.ACT_E)
def test_act_over_the_corners_of_the_fused_decoder(ctx, dev, E, torso, cell):
    """every (A, O, n) corner at this (E, torso, cell): the fused launch without and with the rollout's weight images, and the same
    case layer by layer (fused_recurrent_act = 0), each against the float64 oracle at _act_case's bars; one corner per n with a
    critic of another input width, depth and hidden widths reading its own rows (critic_obs)."""
    worst, seed = {}, 0
    other = nets.MLPSpec(23, [256, 128], 1, nets.ACT_ELU, True, False)
    for A in lc.ACT_A:
        for O in lc.ACT_O:
            for n in lc.ACT_N:
                seed += 1
                critic = other if (A, O) == (32, 1) else None
                a = lc.ActCase(E, torso, A, O, n, cell, critic=critic, seed=1000 * E + 10 * sum(torso) + seed)
                assert a.fused(1) and not a.fused(0)
                for fused, images, want in ((1, False, 1), (1, True, 1), (0, False, 0)):
                    got, launches = _act(ctx, dev, a, fused, images)
                    assert launches == want, (A, O, n, fused, images, launches)
                    _act_check(a, got, worst)
    print(f"recurrent act E={E} torso={torso} {cell}: worst fraction of each bar over {seed} corners x 3 paths:",
          {k: float(f"{v:.2f}") for k, v in worst.items()})


@pytest.mark.parametrize("what", sorted(lc.ACT_OUTSIDE))
def test_act_just_outside_the_decoder_envelope_takes_the_generic_path(ctx, dev, what):
    E, torso, A, combine = lc.ACT_OUTSIDE[what]
    worst = {}
    for i, (cell, n) in enumerate((("lstm", 33), ("gru", 33), ("lstm", 1), ("gru", 65))):
        a = lc.ActCase(E, torso, A, 17, n, cell, combine=combine, seed=7000 + i)
        assert not a.fused(1)
        for images in (False, True):
            got, launches = _act(ctx, dev, a, 1, images)
            assert launches == 0, (what, cell, n, launches)
            _act_check(a, got, worst)
    print(f"recurrent act outside the envelope ({what}): worst fraction of each bar:", {k: float(f"{v:.2f}") for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name", sorted(lc.REFUSED))
def test_refused_shapes_answer_with_their_message_and_leave_the_context_usable(ctx, dev, name):
    """each clause of check_lstm_desc through the acting step, the minibatch pass and the whole update: code and message, key and
    opt_count untouched (no kernel runs on the shape: the check is every entry's first step after its NULL and size checks), and the
    context then serves a small accepted case correctly"""
    O, A, E, H, torso, cell, combine = lc.REFUSED[name]
    code, msg = npth.lstm_check_desc(O, A, E, H, torso, cell, combine)
    ld = lstm_policy_desc(O, A, E, H, torso, False, cell, combine)
    cs = nets.make_spec("B", 5, 1, False)
    cdsc = _cdesc(cs)
    T, N, ne = 2, 8, 4
    z = lambda *s: torch.zeros(*s, device=dev)
    big = z(1 << 20)                               # parameters, moments and gradients of any description above
    wide = z(T, N, 128)                            # observation / action rows of any width above
    F = ctypes.POINTER(ctypes.c_float)
    keep = []                                      # every tensor handed over stays alive to the end of the test
    f = lambda t_: (keep.append(t_), L._ptr(t_, torch.float32))[1]
    hp = _hp()
    st = L._stream()
    lib = ctx.lib
    KEY = (7, 11)

    def refused(rc):
        err = lib.rlx_last_error().decode()
        assert rc == code and msg in err, (rc, err)

    key = (ctypes.c_uint32 * 2)(*KEY)
    refused(lib.rlx_ppo_lstm_act_f32(ctx.h, ctypes.byref(ld), f(big), ctypes.byref(cdsc), f(big), f(wide), None, f(z(N, 128)), f(z(N, 128)),
                                     key, L.THREEFRY_PARTITIONABLE, f(wide), f(wide), f(z(N)), f(z(N)), N, 0, None, None, 0, N, 0, st))
    assert tuple(key) == KEY
    idx = torch.arange(ne, dtype=torch.int32, device=dev)
    refused(lib.rlx_ppo_lstm_minibatch_fwd_bwd_f32(ctx.h, ctypes.byref(ld), f(big), f(big), ctypes.byref(cdsc), f(big), f(big), f(z(8)),
                                                   f(wide), f(wide), f(z(T, N)), f(z(T, N)), f(z(T, N)), f(z(T, N)), f(z(N, 128)),
                                                   f(z(N, 128)), L._ptr(idx, torch.int32), ne, T, N,
                                                   ctypes.byref(hp), st))
    cnt = ctypes.c_int64(5)
    lr = np.full(4, lc.LR, np.float32)
    refused(lib.rlx_ppo_lstm_update_f32(ctx.h, ctypes.byref(ld), f(big), f(big), f(big), ctypes.byref(cdsc), f(big), f(big), f(big), f(wide),
                                        f(wide), f(z(T, N)), f(z(T, N)), f(z(T, N)), f(z(T, N)), f(z(N, 128)), f(z(N, 128)), T, N, 2, T * ne,
                                        key, L.THREEFRY_PARTITIONABLE, ctypes.byref(cnt), lr.ctypes.data_as(F), ctypes.byref(hp), f(z(4, 10)),
                                        st))
    assert tuple(key) == KEY and cnt.value == 5
    torch.cuda.synchronize()
    assert bool((big == 0).all())                  # nothing was written
    # the context serves the next call, and serves it right
    c = lc.case(lc.AFTER_REFUSAL)
    met, gp, gc, _ = _minibatch(ctx, dev, c, {}, profile=False)
    lc.assert_within(*lc.compare(c.spec, c.T, c.ne, c.oracle, met, gp, gc))
