"""CPU: the gfx950 code of the handover form of the fused first-layer backward (k_dx_l1bwd_stats<2, 8, ELU, TWIN>, option
l1_stats_handover = 1, the default) next to the forms it replaces (k_dx_l1bwd<2, 8, ELU, LN, BX, TWIN, ROW1 = true>) and of k_l12fwd,
from l1fused.hip cross-compiled with build.py's flags.  Only register and spill counts from the kernels' metadata and the number of
s_barrier in each kernel's code are read.

The handover form loads the rows' LayerNorm mean and 1 / std instead of rebuilding them, so the workgroup barrier between the
per-wave partial sums and their fold is gone: one s_barrier fewer in the kernel (all of its barriers sit in the row-tile loop: the
tile-top barrier, the staging barrier of the single-buffered path, the two reductions' -- now one reduction's).  It must not pay
for that with registers: no more spilled VGPRs than the ROW1 forms of the same build, which sit at the 256-register limit.
k_l12fwd's code does not change (it could always write the statistics array; the host now hands it one next to h1): its spill
count stays what it was before the option existed."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-x_amd"))
import build as rlx_build  # noqa: E402

L12_SPILLS_BEFORE = 6


@pytest.fixture(scope="module")
def l1fused_asm():
    if not os.path.exists(rlx_build.HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "l1fused.s")
        cmd = [rlx_build.HIPCC] + rlx_build.CFLAGS + ["-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                                                      os.path.join(rlx_build.CSRC, "l1fused.hip"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(out).read()


def _kernels(asm, prefix):
    """{mangled name: (VGPRs, spilled VGPRs, s_barrier count)} of the kernels whose mangled name starts with prefix; a kernel's code
    runs from its label to its .Lfunc_end (it may hold an early s_endpgm)"""
    meta = {m.group(1): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"\.name:\s+(_Z\w+)\n(?:(?!\.name:).*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:(?!\.name:).*\n)*?"
                                 r"\s+\.vgpr_spill_count:\s+(\d+)", asm)}
    out = {}
    for m in re.finditer(r"^(" + re.escape(prefix) + r"\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):
        out[m.group(1)] = meta[m.group(1)] + (len(re.findall(r"^\s*s_barrier\b", m.group(2), re.M)),)
    return out


def test_handover_form_drops_a_barrier_without_spilling_more(l1fused_asm):
    # k_dx_l1bwd_stats<NT = 2, NW = 8, ACT = 1 (ELU), TWIN>  against  k_dx_l1bwd<2, 8, 1, LN = true, BX = true, TWIN, ROW1 = true>
    new = _kernels(l1fused_asm, "_ZN3rlx16k_dx_l1bwd_statsILi2ELi8ELi1E")
    row1 = {k: v for k, v in _kernels(l1fused_asm, "_ZN3rlx10k_dx_l1bwdILi2ELi8ELi1ELb1ELb1E").items() if "ELb1EEEvNS" in k}
    assert len(new) == 2 and len(row1) == 2, (sorted(new), sorted(row1))       # single and twin launch of each form
    for twin in ("ELb0EEEvNS", "ELb1EEEvNS"):
        (kn, (vn, sn, bn)), = [(k, v) for k, v in new.items() if twin in k]
        (kr, (vr, sr, br)), = [(k, v) for k, v in row1.items() if twin.replace("EEEvNS", "ELb1EEEvNS") in k]
        print(f"{kn}: {vn} VGPRs, {sn} spilled, {bn} s_barrier;  {kr}: {vr} VGPRs, {sr} spilled, {br} s_barrier")
        assert vn <= 256, (kn, vn)
        assert sn <= sr, (kn, sn, kr, sr)
        assert bn == br - 1, (kn, bn, kr, br)


def test_k_l12fwd_spills_unchanged(l1fused_asm):
    # k_l12fwd<ACT = 1 (ELU), NT2 = 1 (hidden[1] = 256, the benchmark's nets), TWIN, NTS, ROW1>: plain, twin and nontemporal launch of both forms
    ks = _kernels(l1fused_asm, "_ZN3rlx8k_l12fwdILi1ELi1E")
    assert len(ks) == 6, sorted(ks)
    for k, (vgpr, spill, _) in ks.items():
        assert vgpr <= 128, (k, vgpr)
        assert spill == L12_SPILLS_BEFORE, (k, spill)
