"""CPU: the gfx950 code of k_dx_l1bwd<2, 8, ELU, LN, BX> and k_l12fwd with the LayerNorm row statistics computed once per wave and
row (option ln_row_once = 1, the default) and in the earlier form (= 0), from l1fused.hip cross-compiled with build.py's flags.

What is counted is v_rsq_f32, the heart of the 11-instruction group hipcc emits for rsqrtf (denormal guard: compare, scale,
v_rsq_f32, rescale, select).  The earlier form holds one group per row and use -- 2 x 16 in k_dx_l1bwd's two element-wise loops
plus one for the dW1 operand's scale, 16 in k_l12fwd's normalise loop plus one for the statistics array -- the new form one per
tile (ln_row_stats; the dW1 scale and the statistics array take its value).  The ln_row_once = 0 instantiations must still
hold the earlier counts: they are the code that was there before, kept for the A/B.  Neither form may spill more registers than
the kernels did before the option existed (7 and 6: both sit at their register limit, 256 and 128)."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-x_amd"))
import build as rlx_build  # noqa: E402

DX_SPILLS_BEFORE, L12_SPILLS_BEFORE = 7, 6


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
    """{mangled name: (v_rsq_f32 count, spilled VGPRs)} of the kernels whose mangled name starts with prefix"""
    spills = {m.group(1): int(m.group(2))
              for m in re.finditer(r"\.name:\s+(_Z\w+)\n(?:(?!\.name:).*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", asm)}
    out = {}
    for m in re.finditer(r"^(" + re.escape(prefix) + r"\w*):[^\n]*\n(.*?)s_endpgm", asm, re.M | re.S):
        out[m.group(1)] = (len(re.findall(r"^\s*v_rsq_f32", m.group(2), re.M)), spills[m.group(1)])
    return out


def test_k_dx_l1bwd_row_statistics_once(l1fused_asm):
    # k_dx_l1bwd<NT = 2, NW = 8, ACT = 1 (ELU), LN = true, BX = true, TWIN, ROW1>
    ks = _kernels(l1fused_asm, "_ZN3rlx10k_dx_l1bwdILi2ELi8ELi1ELb1ELb1E")
    new = {k: v for k, v in ks.items() if "ELb1EEEvNS" in k}       # ROW1 = true: the default (launch_l1fused)
    old = {k: v for k, v in ks.items() if "ELb0EEEvNS" in k}
    assert len(new) == 2 and len(old) == 2, sorted(ks)            # single and twin launch of each form
    for k, (rsq, spill) in new.items():
        assert rsq <= 2, (k, rsq)
        assert spill <= DX_SPILLS_BEFORE, (k, spill)
    for k, (rsq, spill) in old.items():
        assert rsq == 33, (k, rsq)
        assert spill <= DX_SPILLS_BEFORE, (k, spill)


def test_k_l12fwd_row_statistics_once(l1fused_asm):
    # k_l12fwd<ACT = 1 (ELU), NT2 = 1 (hidden[1] = 256, the benchmark's nets), TWIN, NTS, ROW1>
    ks = _kernels(l1fused_asm, "_ZN3rlx8k_l12fwdILi1ELi1E")
    new = {k: v for k, v in ks.items() if "ELb1EEEvNS" in k}
    old = {k: v for k, v in ks.items() if "ELb0EEEvNS" in k}
    assert len(new) == 3 and len(old) == 3, sorted(ks)            # plain, twin and nontemporal launch of each form
    for k, (rsq, spill) in new.items():
        assert rsq <= 2, (k, rsq)
        assert spill <= L12_SPILLS_BEFORE, (k, spill)
    for k, (rsq, spill) in old.items():
        assert rsq == 17, (k, rsq)
        assert spill <= L12_SPILLS_BEFORE, (k, spill)
