"""CPU: the gfx950 code of the prefetching form of the fused first + second layer forward (k_l12fwd_pf<ELU, NT2 = 1, TWIN, NTS>,
option l12_prefetch = 1, the default) next to the form it replaces (k_l12fwd<ELU, 1, TWIN, NTS, ROW1 = true>), from l1fused.hip
cross-compiled with build.py's flags.  Only the kernels' metadata (registers, spills) and their s_waitcnt, s_barrier,
global_load_dwordx4 and v_mfma lines are read.

Both forms hold three s_barrier, all in the row-tile loop and in this order in the code: the tile-top barrier, the one between the
LayerNorm partial sums and their fold, the one that completes the h1 image -- and 24 v_mfma: the 12 of the z1 product between the
first two barriers (two 16-k blocks x two column tiles x three plane products), the 12 of the layer-2 K loop behind the third
(the loop body's two blocks and the two peeled ones).

The new form must
  - stay at two workgroups per CU: at most 128 VGPRs, no more spilled registers than the earlier form (6);
  - hold the same barriers and MFMAs;
  - reach the last z1 MFMA from the tile-top barrier without s_waitcnt vmcnt(0) (the earlier form has eight there: four spill
    reloads, the first 16-k block's last fragment, the second block's serial round trips) and without requesting a fragment (no
    global_load_dwordx4: the operands are in registers);
  - keep the K loop's prefetch depth: in the loop body and in the peeled blocks EVERY vmcnt at least the earlier form's highest there
    (2: one whole 16-k block's fragments stay in flight; the earlier form also waits 1 in the body and 0 in its last block), and no
    vmcnt(0) at all (the peeled blocks refill now, so their last wait no longer drains).
The six earlier entries (plain, twin, nontemporal launch x both statistics forms) must still be there."""
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
Z1_MFMA, K_BODY_MFMA, K_MFMA = 12, 6, 12
K_DEPTH = 2      # fragment loads of one 16-k block of W2's image per wave at hidden[1] = 256: one column tile x two planes


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
    """{mangled name: (VGPRs, spilled VGPRs, events)} of the kernels whose mangled name starts with prefix.  events: the kernel's
    s_barrier ("bar"), v_mfma ("mfma"), global_load_dwordx4 ("ld4") and s_waitcnt vmcnt(n) (("wait", n)) lines in code order."""
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
            elif op == "global_load_dwordx4":
                ev.append("ld4")
            elif op == "s_waitcnt":
                w = re.search(r"vmcnt\((\d+)\)", ln)
                if w:
                    ev.append(("wait", int(w.group(1))))
        out[m.group(1)] = meta[m.group(1)] + (ev,)
    return out


def _phases(ev):
    """-> (events from the tile-top barrier to the last z1 MFMA, K loop body, peeled blocks): see the module docstring"""
    bars = [i for i, e in enumerate(ev) if e == "bar"]
    assert len(bars) == 3, len(bars)
    z1 = ev[bars[0] + 1:bars[1]]
    assert z1.count("mfma") == Z1_MFMA, z1.count("mfma")
    last = max(i for i, e in enumerate(z1) if e == "mfma")
    k = ev[bars[2] + 1:]
    assert k.count("mfma") == K_MFMA, k.count("mfma")
    idx = [i for i, e in enumerate(k) if e == "mfma"]
    return z1[:last + 1], k[:idx[K_BODY_MFMA - 1] + 1], k[idx[K_BODY_MFMA - 1] + 1:idx[-1] + 1]


def _waits(ev):
    return [e[1] for e in ev if isinstance(e, tuple)]


def test_earlier_entries_still_there(l1fused_asm):
    old = _kernels(l1fused_asm, "_ZN3rlx8k_l12fwdILi1ELi1E")
    assert len(old) == 6, sorted(old)
    assert len(_kernels(l1fused_asm, "_ZN3rlx8k_l12fwdILi1ELi2E")) == 6       # hidden[1] = 512: no new form


def test_prefetch_form_opens_a_tile_without_drained_waits(l1fused_asm):
    # k_l12fwd_pf<ACT = 1 (ELU), NT2 = 1, TWIN, NTS>  against  k_l12fwd<1, 1, TWIN, NTS, ROW1 = true>
    new = _kernels(l1fused_asm, "_ZN3rlx11k_l12fwd_pfILi1ELi1E")
    old = {k: v for k, v in _kernels(l1fused_asm, "_ZN3rlx8k_l12fwdILi1ELi1E").items() if "ELb1EEEvNS" in k}
    assert len(new) == 3 and len(old) == 3, (sorted(new), sorted(old))          # plain, twin and nontemporal launch of each form
    for form in ("ELb0ELb0E", "ELb1ELb0E", "ELb0ELb1E"):                        # <TWIN, NTS>
        (kn, (vn, sn, en)), = [(k, v) for k, v in new.items() if form + "EEvNS" in k]
        (ko, (vo, so, eo)), = [(k, v) for k, v in old.items() if form + "Lb1EEEvNS" in k]
        zn, bn, pn = _phases(en)
        zo, bo, po = _phases(eo)
        print(f"{kn}: {vn} VGPRs, {sn} spilled; tile top -> last z1 MFMA waits {_waits(zn)} ({zn.count('ld4')} fragment loads), "
              f"K loop body {_waits(bn)}, peeled {_waits(pn)}")
        print(f"{ko}: {vo} VGPRs, {so} spilled; tile top -> last z1 MFMA waits {_waits(zo)} ({zo.count('ld4')} fragment loads), "
              f"K loop body {_waits(bo)}, peeled {_waits(po)}")
        assert vn <= 128, (kn, vn)
        assert sn <= L12_SPILLS_BEFORE and so == L12_SPILLS_BEFORE, (kn, sn, ko, so)
        assert en.count("bar") == eo.count("bar") and en.count("mfma") == eo.count("mfma"), (kn, ko)
        assert 0 not in _waits(zn), (kn, _waits(zn))
        assert zn.count("ld4") == 0, (kn, zn.count("ld4"))
        assert 0 in _waits(zo) and zo.count("ld4") == 8, (ko, _waits(zo))     # what the new form removes is there in the earlier one
        # the prefetch depth: EVERY wait of the new form leaves at least as many loads in flight as the deepest wait of the earlier
        # form in the same part of the loop -- one whole 16-k block's fragments (K_DEPTH loads), the depth the loop is written for
        assert max(_waits(bo)) == K_DEPTH and max(_waits(po)) == K_DEPTH, (ko, _waits(bo), _waits(po))
        assert _waits(bn) and min(_waits(bn)) >= max(_waits(bo)), (kn, _waits(bn), _waits(bo))
        assert _waits(pn) and min(_waits(pn)) >= max(_waits(po)), (kn, _waits(pn), _waits(po))
        assert 0 not in _waits(bn) + _waits(pn), (kn, _waits(bn), _waits(pn))
