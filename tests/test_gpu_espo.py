"""GPU: ESPO's epoch loop (rlx_espo_update_f32, rl-x_amd/csrc/espo.hip) against the reference fixture
(tests/golden/espo_reference.npz) through the float64 twin that reproduces it to 1e-12 (tests/espo_twin.py): every fixture case
at the project's bars; the device-side stop bit for bit against a run that simply has fewer epochs, at every chunk length; two
identical calls and one / two streams give identical bits; every refusal of the envelope."""
import numpy as np
import pytest
import torch

import espo_cases as ec
from espo_cases import Run
from rlx_amd.hip import ACT_ELU, ACT_TANH, mlp_desc
from rlx_amd.hip import lib as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", range(ec.n_cases()))
def test_update_matches_the_reference(ctx, dev, c):
    fc = ec.load(c)
    st, met, run, info = fc.twin()
    assert run == fc.epochs_run and ec.margins_ok(info)
    r = Run(ctx, dev, fc)
    ec.check_against_twin(r, fc.state(), st, met, run)
    for name, key, tol in (("p_after", "p", 1e-5), ("pm_after", "pm", 1e-5), ("pv_after", "pv", 5e-5), ("c_after", "c", 1e-5),
                           ("cm_after", "cm", 1e-5), ("cv_after", "cv", 5e-5)):
        idx, val, _ = fc.sampled(name)
        assert ec._rel(r.out[key][idx], val) < tol, (name, ec._rel(r.out[key][idx], val))
    assert r.run == fc.epochs_run
    ref = fc.metrics
    assert np.all(np.abs(r.metrics[:run, :7] - ref) <= 1e-5 * np.maximum(np.abs(ref), 1.0))


_STOP = {}


def _stop_case():
    """E = 8 epochs whose ratio_delta sets a new maximum at epochs 2, 3 and 7 (so a threshold between the running maximum and the
    epoch's value stops exactly there), each threshold at least 1 % off every value it is compared with: the first seed that does"""
    if not _STOP:
        for seed in range(200):
            fc = ec.random_case(1000 + seed, 9, 3, 64, 120, 16, 8, lr=3e-3)
            rd = fc.twin(max_ratio_delta=np.inf)[1][:, 3]
            thr = {0: 0.5 * rd[0]}
            for k in (2, 3, 7):
                lo = rd[:k].max()
                if rd[k] > 1.05 * lo:
                    thr[k] = 0.5 * (lo + rd[k])
            if len(thr) == 4:
                _STOP.update(fc=fc, thr=thr)
                break
    assert _STOP, "no seed gave the stop pattern"
    return _STOP["fc"], _STOP["thr"]


@pytest.mark.parametrize("k", [0, 2, 3, 7])
@pytest.mark.parametrize("chunk", [1, 3, None])
def test_stop_is_exact(ctx, dev, chunk, k):
    """a run of E = 8 epochs that stops after epoch k == a run of k + 1 epochs with no threshold, bit for bit: parameters, moments,
    metrics rows 0..k, epochs_run and the optimizer count; rows past k keep the sentinel.  k = 0, a chunk's last (2) and first (3)
    epoch at chunk 3, and E - 1; chunk 1, 3 and the default (one chunk)."""
    fc, thr = _stop_case()
    _, _, run, info = fc.twin(max_ratio_delta=thr[k])
    assert run == k + 1 and ec.margins_ok(info, 1e-2)
    stopped = Run(ctx, dev, fc, chunk=chunk, max_ratio_delta=thr[k])
    short = Run(ctx, dev, fc, max_epochs=k + 1, max_ratio_delta=np.inf)
    assert stopped.run == short.run == k + 1 and stopped.count == k + 1
    assert stopped.same_bits(short, k + 1)
    assert np.all(stopped.metrics[k + 1:] == ec.SENTINEL) and np.all(np.isfinite(stopped.metrics[:k + 1]))
    assert stopped.metrics[k, 3] > thr[k] and np.all(stopped.metrics[:k, 3] <= thr[k])
    if k < 7:       # one more epoch would have moved the parameters: the gate, not luck
        longer = Run(ctx, dev, fc, max_epochs=k + 2, max_ratio_delta=np.inf)
        assert longer.out["p"].tobytes() != stopped.out["p"].tobytes() and longer.out["c"].tobytes() != stopped.out["c"].tobytes()


@pytest.mark.parametrize("op", ["mean", "median"])
def test_identical_calls_and_stream_schedules_give_identical_bits(ctx, dev, op):
    fc = ec.random_case(77, 17, 6, 256, 700, 257, 4, op=op, max_ratio_delta=np.inf)
    a, b = Run(ctx, dev, fc), Run(ctx, dev, fc)
    assert a.run == 4 and a.same_bits(b, 4) and np.all(np.isfinite(a.metrics[:, :7]))
    one = Run(ctx, dev, fc, two_streams=0)
    assert one.same_bits(a, 4)
    st2 = ec.f32_state(dict(a.out, count=a.count))       # a second call: non-zero moments, steps 5..8
    c, d = Run(ctx, dev, fc, st=st2, two_streams=0, chunk=2), Run(ctx, dev, fc, st=st2, two_streams=1, chunk=5)
    assert c.same_bits(d, 4) and c.count == 8 and not c.same_bits(a, 4)


def test_a_nan_ratio_delta_does_not_stop_and_skips_the_policy_steps(ctx, dev):
    """espo.py:277: NaN > max_ratio_delta is False.  A NaN old log-prob makes ratio_delta and the policy gradient NaN: every epoch
    runs, the policy keeps its parameters (the library's non-finite rule), the critic trains"""
    fc = ec.random_case(5, 8, 2, 64, 64, 16, 3, op="median", max_ratio_delta=0.01)
    fc.log_probs = fc.log_probs.copy()
    fc.log_probs[fc.idx[:, 0]] = np.nan
    r = Run(ctx, dev, fc)
    assert r.run == 3 and np.all(np.isnan(r.metrics[:, 3])) and np.all(np.isnan(r.metrics[:, 5]))
    assert r.out["p"].tobytes() == fc.p0.astype(np.float32).astype(np.float64).tobytes() and not r.out["pm"].any()
    assert np.all(np.isfinite(r.metrics[:, [1, 6]])) and r.out["c"].tobytes() != fc.c0.astype(np.float32).astype(np.float64).tobytes()


def _call(ctx, dev, fc, pd=None, cd=None, mb=None, E=None, B=None, op=0, idx=None, pidx="keep", cidx="keep", states=None):
    t = lambda x, dt=np.float32: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dt))).to(dev)
    dpd, dcd = ec.descs(fc)
    pd, cd = pd or dpd, cd or dcd
    hp = ec.espo_hp(fc.h)
    hp.delta_op = op
    mb, E = fc.mb if mb is None else mb, fc.E if E is None else E
    ix = torch.zeros(max(E, 1), max(mb, 1), dtype=torch.int32, device=dev) if idx is None else t(idx, np.int32)
    p, c = torch.zeros(400000, device=dev), torch.zeros(400000, device=dev)
    x = t(fc.states if states is None else states)
    if B is not None:
        x = x[:B].contiguous()
    fp, fcx = fc.indices()
    pi = (None if fp is None else t(fp, np.int32)) if isinstance(pidx, str) else pidx
    ci = (None if fcx is None else t(fcx, np.int32)) if isinstance(cidx, str) else cidx
    met = torch.full((max(E, 1), 8), ec.SENTINEL, device=dev)
    import ctypes
    cnt, run = ctypes.c_int64(0), ctypes.c_int32(-5)
    f, i32 = torch.float32, torch.int32
    rc = ctx.lib.rlx_espo_update_f32(
        ctx.h, ctypes.byref(pd), L._ptr(p, f), L._ptr(p.clone(), f), L._ptr(p.clone(), f), ctypes.byref(cd), L._ptr(c, f), L._ptr(c.clone(), f),
        L._ptr(c.clone(), f), L._ptr(x, f), int(x.shape[1]), L._ptr(pi, i32, True), 0 if pi is None else int(pi.numel()), L._ptr(ci, i32, True),
        0 if ci is None else int(ci.numel()), L._ptr(t(fc.actions), f), L._ptr(t(fc.log_probs), f), L._ptr(t(fc.returns), f),
        L._ptr(t(fc.advantages), f), int(x.shape[0]), L._ptr(ix, i32), int(mb), int(E), ctypes.byref(cnt), 1e-3, ctypes.byref(hp),
        L._ptr(met, f), ctypes.byref(run), L._stream())
    torch.cuda.synchronize()
    msg = ctx.lib.rlx_last_error().decode()
    assert cnt.value == 0 and not p.any() and not c.any() and bool((met == ec.SENTINEL).all())      # a refused call changes nothing
    return rc, msg


EINVAL, EUNSUP = -1, -4


def test_refusals(ctx, dev):
    fc = ec.random_case(3, 8, 3, 64, 40, 8, 2)
    tanh = lambda i, h, o, ls, n=2, act=ACT_TANH, ln=False: mlp_desc(i, h[:n], o, act, ln, ls)
    cases = [
        (dict(mb=1), EUNSUP, "mb"), (dict(mb=4097), EUNSUP, "mb"), (dict(mb=41), EINVAL, "mb <= B"), (dict(E=0), EINVAL, "max_epochs"),
        (dict(op=2), EINVAL, "delta_op"), (dict(op=-1), EINVAL, "delta_op"),
        (dict(pd=tanh(8, [64, 64], 65, True)), EUNSUP, "out_dim"), (dict(pd=tanh(8, [64, 64], 0, True)), EUNSUP, "out_dim"),
        (dict(pd=tanh(8, [96, 96], 3, True)), EUNSUP, "hidden"), (dict(pd=tanh(8, [576, 576], 3, True)), EUNSUP, "hidden"),
        (dict(pd=tanh(8, [64, 128], 3, True)), EUNSUP, "hidden"), (dict(cd=tanh(8, [128, 128], 1, False)), EUNSUP, "same hidden width"),
        (dict(pd=tanh(8, [64, 64, 64], 3, True, n=3)), EUNSUP, "pdesc"), (dict(pd=tanh(8, [64, 64], 3, True, act=ACT_ELU)), EUNSUP, "pdesc"),
        (dict(pd=tanh(8, [64, 64], 3, True, ln=True)), EUNSUP, "pdesc"), (dict(pd=tanh(8, [64, 64], 3, False)), EUNSUP, "has_logstd"),
        (dict(cd=tanh(8, [64, 64], 1, True)), EUNSUP, "cdesc"), (dict(cd=tanh(8, [64, 64], 2, False)), EUNSUP, "cdesc->out_dim"),
        (dict(pd=tanh(7, [64, 64], 3, True)), EINVAL, "pdesc->in_dim"), (dict(cd=tanh(9, [64, 64], 1, False)), EINVAL, "cdesc->in_dim"),
        (dict(pidx=torch.arange(5, dtype=torch.int32, device=dev)), EINVAL, "n_pidx"),
        (dict(idx=np.full((2, 8), 40)), EINVAL, "idx"), (dict(idx=np.full((2, 8), -1)), EINVAL, "idx"),
        (dict(pidx=torch.tensor([0, 1, 2, 3, 4, 5, 6, 8], dtype=torch.int32, device=dev)), EINVAL, "pidx"),
        (dict(cidx=torch.tensor([0, 1, 2, 3, 4, 5, -1, 7], dtype=torch.int32, device=dev)), EINVAL, "cidx"),
    ]
    for kw, code, word in cases:
        rc, msg = _call(ctx, dev, fc, **kw)
        assert rc == code and word in msg and msg.startswith("rlx_espo_update_f32"), (kw, rc, msg)
    assert Run(ctx, dev, fc).run >= 1                          # the same problem inside the envelope is taken
