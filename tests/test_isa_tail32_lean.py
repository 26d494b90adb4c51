"""CPU: the gfx950 code of the lean form of the eight-wave tail (k_tail32_bx_lean<ELU, 256>, option tail32_lean = 1, the default) next
to the kernel it replaces (k_tail32_bx<ELU, 256, 8>) and the four-wave form (k_tail32_bx<ELU, 256, 4>), from ppo.hip cross-compiled
with build.py's flags.  Only the kernels' metadata (registers, spills) and their s_barrier and v_mfma lines are read.

Every tail32 kernel holds both networks' bodies (the policy's and the critic's, chosen by a uniform branch), so the counts are
those of two bodies: 96 v_mfma (2 x (phase A's 8 blocks + phase C's 8 blocks) x three plane products) and, in the earlier
eight-wave form, 14 s_barrier.

The lean form must
  - stay at two workgroups of eight waves per CU: at most 128 VGPRs, no spilled register;
  - hold the same 96 v_mfma;
  - hold fewer s_barrier than the earlier form's 14: the metric sums have LDS slots of their own, so the barrier that kept the head's
    weight-gradient partials out of them is gone from both bodies (12).
(The dZ2 epilogue keeps its ds_read_u16 of the H2 planes: building act'(H2) once on waves 4-7 was tried and did not shorten the tile.)
The two earlier entries must still be there with their registers: 120 VGPRs / 0 spilled and 84 / 0."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-x_amd"))
import build as rlx_build  # noqa: E402

MFMA, BARRIERS_BEFORE = 96, 14


@pytest.fixture(scope="module")
def ppo_asm():
    if not os.path.exists(rlx_build.HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "ppo.s")
        cmd = [rlx_build.HIPCC] + rlx_build.CFLAGS + ["-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                                                      os.path.join(rlx_build.CSRC, "ppo.hip"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(out).read()


def _kernels(asm, prefix):
    """{mangled name: (VGPRs, spilled VGPRs, events)} of the kernels whose mangled name starts with prefix.  events: the kernel's
    s_barrier ("bar") and v_mfma ("mfma") lines in code order."""
    meta = {m.group(1): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"\.name:\s+(_Z\w+)\n(?:(?!\.name:).*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:(?!\.name:).*\n)*?"
                                 r"\s+\.vgpr_spill_count:\s+(\d+)", asm)}
    out = {}
    for m in re.finditer(r"^(" + re.escape(prefix) + r"\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):
        ev = []
        for ln in m.group(2).splitlines():
            op = ln.split(None, 1)[0] if ln.strip() else ""
            if op == "s_barrier":
                ev.append("bar")
            elif op.startswith("v_mfma"):
                ev.append("mfma")
        out[m.group(1)] = meta[m.group(1)] + (ev,)
    return out


def _one(asm, prefix):
    k = _kernels(asm, prefix)
    assert len(k) == 1, (prefix, sorted(k))
    (name, v), = k.items()
    return (name,) + v


def test_earlier_entries_keep_their_registers(ppo_asm):
    # k_tail32_bx<ACT = 1 (ELU), N2 = 256, NWV>
    for nwv, vgprs in ((8, 120), (4, 84)):
        name, v, s, ev = _one(ppo_asm, f"_ZN3rlx11k_tail32_bxILi1ELi256ELi{nwv}EE")
        print(f"{name}: {v} VGPRs, {s} spilled, {ev.count('mfma')} v_mfma, {ev.count('bar')} s_barrier")
        assert (v, s) == (vgprs, 0), (name, v, s)
        assert ev.count("mfma") == MFMA, (name, ev.count("mfma"))


def test_lean_form(ppo_asm):
    name, v, s, ev = _one(ppo_asm, "_ZN3rlx16k_tail32_bx_leanILi1ELi256EE")
    _, _, _, old = _one(ppo_asm, "_ZN3rlx11k_tail32_bxILi1ELi256ELi8EE")
    print(f"{name}: {v} VGPRs, {s} spilled, {ev.count('mfma')} v_mfma, {ev.count('bar')} s_barrier (earlier form: {old.count('bar')})")
    assert v <= 128 and s == 0, (name, v, s)
    assert ev.count("mfma") == MFMA and old.count("mfma") == MFMA, (ev.count("mfma"), old.count("mfma"))
    assert old.count("bar") == BARRIERS_BEFORE, old.count("bar")
    assert ev.count("bar") == BARRIERS_BEFORE - 2, ev.count("bar")          # one barrier fewer in each network's body
