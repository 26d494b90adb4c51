"""CPU: the gfx950 code of the wrapped-refill form of the fused first-layer backward (k_dx_l1bwd_stats_wrap<2, 8, ELU, TWIN>, option
l1_wrap_refill = 1, the default) next to the form it replaces (k_dx_l1bwd_stats<2, 8, ELU, TWIN>), from l1fused.hip cross-compiled
with build.py's flags.  Only the kernels' metadata and their s_waitcnt vmcnt(N), s_barrier, v_mfma and global_load_dwordx4 lines
are read.

The K loop of the main product holds two 16-k blocks of weight fragments in registers (NT * 2 = 4 loads of 16 bytes per block) and
refills a block's slot behind its products.  With the refill behind a condition the compiler cannot count the loads in flight and
opens the second block with s_waitcnt vmcnt(0): the refill issued six MFMAs earlier is drained, an L2 round trip per two blocks.
The new form refills unconditionally (the last two refills fetch the first-layer image for the z1 recompute, which therefore has no
loads of its own: eight 16-byte loads fewer in the kernel), so every wait in its innermost loop leaves at least one block's four
loads in flight.  The same scan applied to the earlier form must find its vmcnt(0): that is what shows the scan looks at the right
loop.  Registers, barriers and MFMAs: the new form must not pay with spills, and it has the same barriers and products."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-x_amd"))
import build as rlx_build  # noqa: E402

NT = 2
NEW = "_ZN3rlx21k_dx_l1bwd_stats_wrapI"
OLD = "_ZN3rlx16k_dx_l1bwd_statsI"
ARGS = "Li2ELi8ELi1E"          # NT = 2, NW = 8, ACT = 1 (ELU)


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
    """{mangled name: dict(vgpr, spill, barriers, mfma, loads, body)} of the kernels whose mangled name starts with prefix; a kernel's
    code runs from its label to its .Lfunc_end"""
    meta = {m.group(1): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"\.name:\s+(_Z\w+)\n(?:(?!\.name:).*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:(?!\.name:).*\n)*?"
                                 r"\s+\.vgpr_spill_count:\s+(\d+)", asm)}
    out = {}
    for m in re.finditer(r"^(" + re.escape(prefix) + r"\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):
        body = m.group(2)
        out[m.group(1)] = dict(vgpr=meta[m.group(1)][0], spill=meta[m.group(1)][1],
                               barriers=len(re.findall(r"^\s*s_barrier\b", body, re.M)),
                               mfma=len(re.findall(r"^\s*v_mfma", body, re.M)),
                               loads=len(re.findall(r"^\s*global_load_dwordx4\b", body, re.M)), body=body)
    return out


def _k_loop_waits(body):
    """vmcnt values waited for inside the innermost loop that holds the main product: the basic blocks from a label marked
    'This Inner Loop Header' to the next block that is not 'in Loop: Header=<that label>', taken for the inner loop with the most
    MFMAs (the K loop: 2 blocks x 3 plane products x NT column tiles; the other inner loops of the kernel stage rows and hold none)"""
    lines = body.split("\n")
    best = (0, None)
    for i, ln in enumerate(lines):
        if "This Inner Loop Header" not in ln:
            continue
        # the label is on this line or, where the header has a parent loop, on the line above
        m = re.match(r"^\.L(BB\d+_\d+):", ln) or re.match(r"^\.L(BB\d+_\d+):", lines[i - 1])
        assert m, ln
        head = m.group(1)
        mfma, waits = 0, []
        for l2 in lines[i + 1:]:
            if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l2) and f"Header={head} " not in l2 + " ":
                break
            mfma += bool(re.match(r"^\s*v_mfma", l2))
            waits += [int(v) for v in re.findall(r"s_waitcnt[^\n]*vmcnt\((\d+)\)", l2)]
        if mfma > best[0]:
            best = (mfma, waits)
    assert best[0] == 2 * 3 * NT, best       # both blocks of the unrolled pair
    return best[1]


def _pairs(asm):
    new, old = _kernels(asm, NEW + ARGS), _kernels(asm, OLD + ARGS)
    assert len(_kernels(asm, NEW)) == 2 and len(new) == 2, sorted(_kernels(asm, NEW))       # single and twin launch, nothing else
    assert len(old) == 2, sorted(old)
    for twin in ("ELb0EEEvNS", "ELb1EEEvNS"):
        (kn, n), = [(k, v) for k, v in new.items() if twin in k]
        (ko, o), = [(k, v) for k, v in old.items() if twin in k]
        yield kn, n, ko, o


def test_two_kernels_without_more_registers_barriers_or_products(l1fused_asm):
    for kn, n, ko, o in _pairs(l1fused_asm):
        print(f"{kn}: {n['vgpr']} VGPRs, {n['spill']} spilled, {n['barriers']} s_barrier, {n['mfma']} v_mfma, {n['loads']} global_load_dwordx4;  "
              f"{ko}: {o['vgpr']} VGPRs, {o['spill']} spilled, {o['barriers']} s_barrier, {o['mfma']} v_mfma, {o['loads']} global_load_dwordx4")
        assert n["vgpr"] <= 256, (kn, n["vgpr"])
        assert n["spill"] <= o["spill"], (kn, n["spill"], ko, o["spill"])
        assert n["barriers"] == o["barriers"], (kn, n["barriers"], ko, o["barriers"])
        assert n["mfma"] == o["mfma"], (kn, n["mfma"], ko, o["mfma"])
        # the z1 recompute's fragments (2 blocks x NT column tiles x 2 planes) come out of the main loop's registers
        assert n["loads"] == o["loads"] - 8, (kn, n["loads"], ko, o["loads"])


def test_k_loop_keeps_a_block_of_fragments_in_flight(l1fused_asm):
    for kn, n, ko, o in _pairs(l1fused_asm):
        wn, wo = _k_loop_waits(n["body"]), _k_loop_waits(o["body"])
        print(f"{kn}: K-loop vmcnt waits {wn};  {ko}: {wo}")
        assert 0 in wo, (ko, wo)                      # the scan sees the drained wait of the earlier form ...
        assert wn and min(wn) >= 2 * NT, (kn, wn)     # ... and none in the new one: one block's NT * 2 loads stay in flight
