"""Python mirror of the host selection arithmetic the FastSAC / FastTD3 passes go through (rl-x_amd/csrc: net_pass.h, dense_head.hip,
mlp.hip, gemm_bx.h / gemm_bx.hip, fastsac.hip) and the ensemble-SAC family's (sac_ens.h, redq.hip's redq_loop, tqc.hip): which kernel,
which grid and which GEMM engine a shape gets; and of what crossq.hip and brn.hip decide on the host (cq_images' lists, cq_dw's bands,
the column sums' slabs, the element-wise walk).  The shape tests recompute each case's claims from these, and build the engine --
for the ensemble family the launches per engine -- each profiled GEMM row has to show."""

BX_MAX_JOBS = 32          # gemm_bx.h
SPLIT_ROWS = 4096         # net_images / bx_dw_usable: rows from which the split-operand engine serves a pass
HEAD_FWD_MAX_LDS = 128 * 1024
F16_MAX = 65504.0
X_WLIMIT, X_ALIMIT = 1023.0, 4094.0     # gemm_bx.h: |weight| and |activation| inside the fp16 window of the split operands


def div_up(a, b):
    return -(-a // b)


def pad4(n):
    return (n + 3) & ~3


def dx_cols_ok(K, nc):
    """mlp.hip dx_cols_ok: launch_dx_cols takes a first layer of width K and nc input columns"""
    return 1 <= nc <= 64 and K % 4 == 0 and (16 * (K + 4) + K * nc) * 4 <= HEAD_FWD_MAX_LDS


def head_nj(K, N):
    """dense_head.hip fs_head_bwd: the tiled kernel's NJ (2 / 4 / 8 / 12), 0 = the untiled kernel"""
    TK = K // 8
    TN = 256 // TK if 0 < TK <= 256 else 0
    nj = div_up(N, TN) if TN else 99
    if not (K % 8 == 0 and nj <= 12 and 16 * (K + N) * 4 <= 48 * 1024):
        return 0
    return 2 if nj <= 2 else 4 if nj <= 4 else 8 if nj <= 8 else 12


def head_masked_threads(K):
    """threads of k_fs_head_dw_tiled with tk >= TK (idle)"""
    TK = K // 8
    return 256 - TK * (256 // TK)


def rows_grid(num_cus, M):
    """net_pass.h rows_grid -> (workgroups, capped)"""
    g = div_up(M, 4)
    return (num_cus * 8, True) if g > num_cus * 8 else (max(g, 1), False)


def bwd_rows_grid(num_cus, M):
    g = div_up(M, 16)
    return (num_cus * 4, True) if g > num_cus * 4 else (max(g, 1), False)


def elem_grid(n):
    """net_pass.h elem_grid / fs_concat: 256-thread blocks, at most 4096 -> (blocks, capped)"""
    g = div_up(n, 256)
    return (4096, True) if g > 4096 else (max(g, 1), False)


def policy_grad_grid(B, A):
    """rlx_fastsac_policy_update_f32: k_fs_policy_grad's grid, at most 2048 blocks"""
    g = div_up(B * A, 256)
    return (2048, True) if g > 2048 else (g, False)


def sample_rows_per_block(A):
    """k_fs_sample: (rows per 256-thread block, idle trailing threads)"""
    rpb = 256 // A
    return rpb, 256 - rpb * A


def bx_grad_scale(rows):
    """gemm_bx.h bx_grad_scale: 8 * 2^ceil(log2 rows)"""
    s, r = 8.0, 1
    while r < rows and s < 1e9:
        r, s = r << 1, s * 2.0
    return s


def bx_dw_usable(bx, M, Kd, ldh, N):
    return bool(bx) and M >= SPLIT_ROWS and N % 4 == 0 and ldh % 4 == 0 and ldh >= pad4(Kd)


def trunk_images(nets):
    """net_pass.h trunk_images over nets = [(in_dim, hidden, bwd)] -> (matrices, jobs, {(net index, layer)} that got images).  The
    list ends at the first matrix whose jobs (one forward image, one transposed for an input gradient) pass BX_MAX_JOBS."""
    mats, jobs, have = 0, 0, set()
    for i, (in_dim, hidden, bwd) in enumerate(nets):
        d = in_dim
        for l, w in enumerate(hidden):
            if d % 4 == 0:
                need = 1 + (1 if bwd and l > 0 else 0)
                if jobs + need > BX_MAX_JOBS:
                    return mats, jobs, have
                mats, jobs = mats + 1, jobs + need
                have.add((i, l))
            d = w
    return mats, jobs, have


def expected_engines(update, bx, B, p_in, p_hidden, c_in, c_hidden, A):
    """{(kernel, M, N, K): engine} of every trunk GEMM the profiler sees in one `update` ("critic" / "policy") of FastSAC or FastTD3
    (prof rows: k_gemm_fwd (rows, out, in); k_gemm_dx (rows, in, out); k_gemm_dw (in, out, rows)).  c_in = critic obs + A.
    Split-operand engine (1) from 4096 rows on, when it is switched on: every forward whose in % 4 == 0 and whose image fitted
    the job table, every input gradient of a layer l > 0, every weight gradient bx_dw_usable accepts (row pitches are padded to 4)."""
    if update == "critic":       # policy, two targets (forward only), two online critics (forward, backward with weight gradients)
        nets = [(p_in, p_hidden, False), (c_in, c_hidden, False), (c_in, c_hidden, False), (c_in, c_hidden, True), (c_in, c_hidden, True)]
        grads, dx_first = {3, 4}, set()
    else:                        # policy (backward with weight gradients), two critics (input gradients down to the action columns)
        nets = [(p_in, p_hidden, True), (c_in, c_hidden, True), (c_in, c_hidden, True)]
        grads, dx_first = {0}, {1, 2}
    on = bool(bx) and B >= SPLIT_ROWS
    have = trunk_images(nets)[2] if on else set()
    out = {}

    def put(key, eng):
        assert out.setdefault(key, eng) == eng, ("two GEMMs of one shape on different engines", key)
    for i, (in_dim, hidden, bwd) in enumerate(nets):
        d = in_dim
        for l, w in enumerate(hidden):
            put(("k_gemm_fwd", B, w, d), 1 if (i, l) in have else 0)
            if bwd and l > 0:
                put(("k_gemm_dx", B, d, w), 1 if (i, l) in have else 0)
            if bwd and l == 0 and i in dx_first and not dx_cols_ok(w, A):
                put(("k_gemm_dx", B, d, w), 0)                      # first_layer_dx's whole-GEMM fallback: no transposed image
            if i in grads:
                put(("k_gemm_dw", d, w, B), 1 if bx_dw_usable(on, B, d, pad4(d), w) else 0)
            d = w
    return out


# ------------------------------------------------------------------------ the ensemble-SAC family (sac_ens.h, redq.hip, tqc.hip)
def ens_lanes_per_row(A):
    """sac_ens.h ens_lanes_per_row: threads that share a row in k_ens_sample / k_ens_policy_grad -- the power of two at or above A,
    at most 64"""
    ap = 1
    while ap < A and ap < 64:
        ap <<= 1
    return ap


def ens_sample_rows_per_block(A):
    """k_ens_sample / k_ens_policy_grad: (rows per 256-thread block, idle lanes per row)"""
    ap = ens_lanes_per_row(A)
    return 256 // ap, ap - A


def drop_ln_relu_form(D):
    """dense_head.hip launch_drop_ln_relu: NJMAX of the k_drop_ln_relu instance a block of D units gets (4: the lean form, D <= 256;
    12: the wide one, D <= 768)"""
    assert D % 64 == 0 and 0 < D <= 768
    return 4 if D <= 256 else 12


def ens_nets(algo, step, p_in, p_hidden, c_in, c_hidden, E, M=None):
    """The list redq_loop (REDQ and DroQ: M selected targets; AQE: M = E) hands to trunk_images in front of a critic step ("critic")
    and of the policy step ("policy"), and rlx_tqc_update_f32's one list ("update"), in their order.  A net is
    (in_dim, hidden, bwd, fwd, grads, dxa): trunk_images' (in_dim, hidden, bwd) and the passes that use the images -- forward
    passes, backward passes with weight gradients, backward passes for the input gradient on the action columns alone."""
    pol, cri = (p_in, tuple(p_hidden)), (c_in, tuple(c_hidden))
    if algo == "tqc":               # policy on s' and on s, one backward; online critics on (s, a) with gradients and on (s, a~) for dQ/da
        assert step == "update"
        return [pol + (True, 2, 1, 0)] + [cri + (True, 2, 1, 1)] * E + [cri + (False, 1, 0, 0)] * E
    M = E if algo == "aqe" else M
    if step == "critic":
        return [pol + (False, 1, 0, 0)] + [cri + (False, 1, 0, 0)] * M + [cri + (True, 1, 1, 0)] * E
    assert step == "policy"
    return [pol + (True, 1, 1, 0)] + [cri + (True, 1, 0, 1)] * E


def image_cut(nets):
    """where trunk_images' list ends: (net index, layer) of the first matrix without an image although its input width is aligned,
    None when every aligned matrix got one"""
    have = trunk_images([n[:3] for n in nets])[2]
    for i, (in_dim, hidden, *_) in enumerate(nets):
        d = in_dim
        for l, w in enumerate(hidden):
            if d % 4 == 0 and (i, l) not in have:
                return i, l
            d = w
    return None


def expected_engine_counts(steps, bx, B, A):
    """{(kernel, M, N, K): {engine: launches}} of every trunk GEMM the profiler sees over `steps`: one ens_nets list per trunk_images
    call, each with the passes that follow it (expected_engines' rules and prof-row shapes).  Where a list ends inside a network,
    or between two networks of one shape, that shape shows on both engines."""
    on = bool(bx) and B >= SPLIT_ROWS
    out = {}

    def put(key, eng, n):
        if n:
            e = out.setdefault(key, {})
            e[eng] = e.get(eng, 0) + n
    for nets in steps:
        have = trunk_images([n[:3] for n in nets])[2] if on else set()
        for i, (in_dim, hidden, bwd, fwd, grads, dxa) in enumerate(nets):
            assert bwd or not (grads or dxa)
            d = in_dim
            for l, w in enumerate(hidden):
                eng = 1 if (i, l) in have else 0
                put(("k_gemm_fwd", B, w, d), eng, fwd)
                if l > 0:
                    put(("k_gemm_dx", B, d, w), eng, grads + dxa)
                elif not dx_cols_ok(w, A):
                    put(("k_gemm_dx", B, d, w), 0, dxa)             # first_layer_dx's whole-GEMM fallback: no transposed image
                put(("k_gemm_dw", d, w, B), 1 if bx_dw_usable(on, B, d, pad4(d), w) else 0, grads)
                d = w
    return out


def check_engine_counts(rows, expected):
    """every profiled trunk GEMM row against expected_engine_counts: the same shapes, and per shape the same launches per engine"""
    seen = {}
    for q in rows:
        if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw"):
            e = seen.setdefault((q["kernel"], q["M"], q["N"], q["K"]), {})
            e[q["engine"]] = e.get(q["engine"], 0) + q["launches"]
    bad = {k: (seen.get(k), expected.get(k)) for k in set(seen) | set(expected) if seen.get(k) != expected.get(k)}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------- CrossQ (crossq.hip, brn.hip)
G_BM, G_BN, G_BK = 128, 128, 32     # gemm.h
REDUCE_MAX_BLOCKS = 4096            # mlp.h
BRN_SLAB_ROWS = 64                  # brn.hip


def choose_mc(M, tiles, num_cus):
    """mlp.hip choose_mc: the M-split of a weight-gradient GEMM -> (slab rows, slabs)"""
    S = max(div_up(num_cus, tiles), 1)
    Mc = max(div_up(div_up(M, S), G_BK) * G_BK, G_BK)
    return Mc, max(div_up(M, Mc), 1)


def cq_dw_blocks(num_cus, M, k, N):
    """crossq.hip cq_dw: the workgroups the slab reduction of a band of k rows of W [., N], and of the bias, is counted at"""
    S = choose_mc(M, div_up(k, G_BM) * div_up(N, G_BN), num_cus)[1]
    return div_up(k * N, 64 if S >= 128 else 256) + div_up(N, 16)


def cq_dw_bands(num_cus, M, Kd, N):
    """crossq.hip cq_dw: the row bands of W [Kd, N] in which a Dense's weight gradient over M rows is taken -- the band is halved (to a
    multiple of 64) until cq_dw_blocks fits REDUCE_MAX_BLOCKS -> the band sizes, in order"""
    kb = Kd
    while kb > 64 and cq_dw_blocks(num_cus, M, kb, N) > REDUCE_MAX_BLOCKS:
        kb = div_up(kb // 2, 64) * 64
    return [min(kb, Kd - k0) for k0 in range(0, Kd, kb)]


def brn_rows_per_slab(num_cus, M):
    """brn.hip brn_rows_per_slab: the rows one workgroup of k_brn_colsum sums -- BRN_SLAB_ROWS until M passes what 4 num_cus slabs hold"""
    cap = 4 * max(num_cus, 1)
    return div_up(M, cap) if div_up(M, BRN_SLAB_ROWS) > cap else BRN_SLAB_ROWS


def brn_walk(M, ld):
    """the grid-stride walk of k_brn_apply_* over the float4 groups of [M, ld] (BrnWalk) -> (groups, most steps a thread takes,
    step_cg, whether a step can carry into the next row: the `cg >= ld4` branch)"""
    ld4, groups = ld // 4, M * (ld // 4)
    stride = elem_grid(groups)[0] * 256
    step_cg = stride % ld4
    return groups, div_up(groups, stride), step_cg, groups > stride and step_cg > 0


def cq_nets(update, p_in, p_hidden, c_in, c_hidden, E, B):
    """The networks of rlx_crossq_critic_update_f32 ("critic": the policy in eval mode on s', B rows; the E critics' joint training pass
    of 2 B rows, backward with weight gradients) and of rlx_crossq_policy_update_f32 ("policy": the policy's training pass and the E
    critics in eval mode for dQ/da, all of B rows), in cq_images' order -> [(rows of the network's pass, net in ens_nets' form)]"""
    pol, cri = (p_in, tuple(p_hidden)), (c_in, tuple(c_hidden))
    if update == "critic":
        return [(B, pol + (False, 1, 0, 0))] + [(2 * B, cri + (True, 1, 1, 0))] * E
    assert update == "policy"
    return [(B, pol + (True, 1, 1, 0))] + [(B, cri + (True, 1, 0, 1))] * E


def cq_image_list(update, p_in, p_hidden, c_in, c_hidden, E, B):
    """the list cq_images hands to the image builder, in the form ens_nets returns (image_cut and trunk_images take it): a network is
    listed only when ITS pass has SPLIT_ROWS rows or more"""
    return [n for rows, n in cq_nets(update, p_in, p_hidden, c_in, c_hidden, E, B) if rows >= SPLIT_ROWS]


def cq_engine_counts(updates, bx, num_cus, p_in, p_hidden, c_in, c_hidden, E, B):
    """{(kernel, M, N, K): {engine: launches}} of every trunk GEMM of the given updates, from expected_engine_counts per row count of
    a call's passes -- the image list is one per call, a listed network's launches are counted at its own rows -- with what CrossQ does
    differently from the ensemble family: the first Dense's input gradient is always the whole GEMM on the exact engine (cq_bwd: BRN 0
    needs all of it), and a weight gradient is one launch per band of cq_dw_bands, every band on its Dense's engine"""
    out = {}

    def add(key, eng, n):
        if n:
            out.setdefault(key, {})
            out[key][eng] = out[key].get(eng, 0) + n
    for update in updates:
        nets = cq_nets(update, p_in, p_hidden, c_in, c_hidden, E, B)
        listed = [(rows, n) for rows, n in nets if rows >= SPLIT_ROWS]
        # per row count the whole image list, the launches of the networks at other row counts struck out; an unlisted network alone
        groups = [(r, [n if rows == r else n[:3] + (0, 0, 0) for rows, n in listed]) for r in sorted({rows for rows, _ in listed})]
        groups += [(rows, [n]) for rows, n in nets if rows < SPLIT_ROWS]
        for rows, g in groups:
            first = {("k_gemm_dx", rows, n[0], n[1][0]) for n in g}
            assert not first & {("k_gemm_dx", rows, d, w) for n in g for d, w in zip(n[1], n[1][1:])}, "a hidden Dense of a first one's shape"
            for (kernel, M, N, K), engines in expected_engine_counts([g], bx, rows, 0).items():       # (A 0: no dx_cols kernel here)
                if (kernel, M, N, K) in first:
                    continue                                                                          # counted below
                for eng, launches in engines.items():
                    if kernel == "k_gemm_dw":
                        for k in cq_dw_bands(num_cus, rows, M, N):
                            add((kernel, k, N, K), eng, launches)
                    else:
                        add((kernel, M, N, K), eng, launches)
            for in_dim, hidden, _, _, grads, dxa in g:
                add(("k_gemm_dx", rows, in_dim, hidden[0]), 0, grads + dxa)
    return out


def check_engines(rows, expected):
    """every profiled trunk GEMM row has the engine the selection code gives its shape, and every expected shape was seen"""
    seen = {}
    for q in rows:
        if q["kernel"] in ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw"):
            seen.setdefault((q["kernel"], q["M"], q["N"], q["K"]), set()).add(q["engine"])
    bad = {k: (sorted(v), expected.get(k)) for k, v in seen.items() if v != {expected.get(k)}}
    assert not bad, bad
    assert set(expected) <= set(seen), sorted(set(expected) - set(seen))


# ------------------------------------------------- PPO minibatch pass (ppo.hip, l1fused.hip, gemm_bx.hip, mlp.hip: net_fwd_bwd / twin_fwd_bwd)
ACT_TANH, ACT_ELU, ACT_RELU = 0, 1, 2          # rlx_hip.h
ENGINE_EXACT, ENGINE_SPLIT, ENGINE_HBM = 0, 1, 2   # profiler rows: exact-fp32 GEMM, split-operand fp16 pipe, bandwidth-bound launch (common.h)
HEAD_ROWS, T32_ROWS, TL_K3 = 64, 32, 128       # ppo.hip
LF_PFX = 2                                     # l1fused.hip RLX_LF_PFX
PPO_DEFAULTS = dict(ppo_twin=-1, ppo_tail=-1, l12_fused=1, dw_merge=1, dw_recompute=1, gemm_bx=1, l1fwd_mfma=1, disable_l1fused=0)


def ppo_opts(options=None):
    o = dict(PPO_DEFAULTS)
    o.update(options or {})
    assert set(o) == set(PPO_DEFAULTS), sorted(set(o) - set(PPO_DEFAULTS))
    return o


def row_pitch(O):
    """ppo.hip row_pitch: the stride of gathered observation rows -- wide rows are zero padded to a multiple of 4"""
    return pad4(O) if O > 32 and O % 4 else O


def mlp_check_desc(O, hidden, A, act, ln_first):
    """mlp.hip check_desc -> None, or the message of the RLX_EUNSUP / RLX_EINVAL it raises"""
    if not 1 <= len(hidden) <= 3:
        return "mlp: n_hidden must be 1..3"
    if not 1 <= O <= 8192:
        return "mlp: in_dim must be 1..8192"
    if not (O <= 32 or not ln_first or len(hidden) >= 2):
        return "mlp: LayerNorm after a wide first layer needs at least two hidden layers"
    if not (hidden[0] % 64 == 0 and 64 <= hidden[0] <= 512):
        return "mlp: hidden[0] must be a multiple of 64 in [64, 512]"
    if any(h % 4 or h < 4 for h in hidden[1:]):
        return "mlp: hidden dims must be multiples of 4"
    if not 1 <= A <= 64:
        return "mlp: out_dim must be 1..64"
    if act not in (ACT_TANH, ACT_ELU, ACT_RELU):
        return "mlp: unknown activation"
    return None


def mlp_blocks(O, hidden, A, ln_first, has_logstd):
    """the flat parameter layout (rlx_hip.h; make_layout) -> ([(name, offset, length)], n_params)"""
    out, off, d = [], 0, O
    for l, h in enumerate(hidden):
        blocks = [(f"W{l}", d * h), (f"b{l}", h)] + ([(f"ln_scale{l}", h), (f"ln_bias{l}", h)] if ln_first and l == 0 else [])
        for name, n in blocks:
            out.append((name, off, n))
            off += n
        d = h
    for name, n in (("Wh", d * A), ("bh", A)) + ((("logstd", A),) if has_logstd else ()):
        out.append((name, off, n))
        off += n
    return out, off


def l1fwd_mfma_supported(O, hidden, act, ln_first):
    return hidden[0] == 512 and act == ACT_ELU and ln_first and O <= 32


def l12fwd_supported(O, hidden, act, ln_first):
    return l1fwd_mfma_supported(O, hidden, act, ln_first) and len(hidden) >= 2 and hidden[1] in (256, 512)


def l1fused_supported(O, hidden, act, ln_first):
    combo = (hidden[0] == 512 and act == ACT_ELU and ln_first) or (hidden[0] == 256 and act in (ACT_TANH, ACT_RELU) and not ln_first)
    return combo and len(hidden) >= 2 and O <= 32 and hidden[1] % 32 == 0 and hidden[1] <= 512


def bx_mlp_images(O, hidden, act, ln_first, on):
    """gemm_bx.hip bx_prepare_mlp(with_bwd): {(layer, transposed)} of the split weight images a pass of `on` (gemm_bx and >= SPLIT_ROWS
    rows) registers: both images of every hidden layer l >= 1 with aligned widths, the first layer's forward image for the fused
    first-layer backward"""
    have = set()
    if not on:
        return have
    for l in range(1, len(hidden)):
        if hidden[l - 1] % 4 == 0 and hidden[l] % 4 == 0:
            have |= {(l, 0), (l, 1)}
    if have and O <= 32 and l1fused_supported(O, hidden, act, ln_first):
        have.add((0, 0))
    return have


def l1fused_bx(O, hidden, act, ln_first, have):
    """l1fused.hip l1fused_bx_images: the fused first-layer backward runs its main product on the split engine"""
    N2 = hidden[1]
    return N2 % 128 == 0 and N2 % (16 * LF_PFX) == 0 and (1, 1) in have and (0, 0) in have


def tail_rows(hidden, act, mb, opts):
    """ppo.hip tail_rows: rows per workgroup of the tail form a minibatch takes"""
    can32 = hidden[1] == 256 and act == ACT_ELU and mb % T32_ROWS == 0
    want32 = opts["ppo_tail"] == 2 or (opts["ppo_tail"] < 0 and (mb <= 8192 or mb > 16384))
    return T32_ROWS if can32 and want32 else HEAD_ROWS


def tail_shape_ok(hidden, A, mb, opts):
    """ppo.hip tail_shape_ok (Gaussian policy or critic): last hidden layer + head + loss + both input gradients in one launch"""
    return bool(opts["ppo_tail"] and opts["gemm_bx"] and len(hidden) == 3 and hidden[2] == TL_K3 and hidden[1] % G_BN == 0 and
                hidden[1] <= 512 and A <= 8 and mb >= 4096 and mb % HEAD_ROWS == 0)


def head_kernel(hidden, A, tail):
    """which kernel evaluates head and loss of one network: inside the tail, k_head_loss_fast<K / 4> or the LDS-staged k_head_loss"""
    K = hidden[-1]
    return "tail" if tail else f"fast{K}" if A <= 8 and K in (64, 128, 256) else "generic"


def dw_merge_ok(hidden, mb, opts):
    on = bool(opts["gemm_bx"])
    return bool(opts["dw_merge"]) and len(hidden) == 3 and bx_dw_usable(on, mb, hidden[1], hidden[1], hidden[2]) and \
        bx_dw_usable(on, mb, hidden[0], hidden[0], hidden[1])


def twin_shapes_ok(O, hidden, A, act, ln_first, mb, opts):
    """ppo.hip twin_shapes_ok for one process, a Gaussian policy and a critic of the policy's trunk reading the policy's rows through
    rlx_ppo_minibatch_fwd_bwd_f32 (which takes the twin pass only at ppo_twin = 1; at -1 the whole-update entries decide by size:
    twin_default)"""
    if opts["ppo_twin"] == 0 or (opts["ppo_twin"] < 0 and mb > 16384):
        return False
    if not opts["gemm_bx"] or opts["disable_l1fused"] or not opts["l1fwd_mfma"]:
        return False
    if len(hidden) < 2 or A > 8 or any(h % 4 for h in hidden[1:]) or hidden[-1] not in (64, 128, 256):
        return False
    if mb < SPLIT_ROWS or not l1fwd_mfma_supported(O, hidden, act, ln_first) or not l1fused_supported(O, hidden, act, ln_first):
        return False
    return all(bx_dw_usable(True, mb, hidden[l - 1], hidden[l - 1], hidden[l]) for l in range(1, len(hidden)))


def twin_default(O, hidden, A, act, ln_first, mb, gather_group_rows=524288, gather_records=True):
    """what rlx_ppo_update_f32 picks at ppo_twin = -1 on one GPU: twin launches from 6144 (grouped gathers below) to 16384 rows"""
    o = ppo_opts()
    if mb < 6144 and gather_records and gather_group_rows > mb and O + A + 3 <= 128:
        return False
    return twin_shapes_ok(O, hidden, A, act, ln_first, mb, o)


def ppo_refusal(O, hidden, A, act, ln_first, mb, repitch=True):
    """(code, message) of the error the minibatch pass answers a shape with, None when it runs.  repitch: the pass gathers wide rows
    at row_pitch(O) (without it a wide O that is no multiple of 4 is refused by mlp_trunk_fwd)"""
    msg = mlp_check_desc(O, hidden, A, act, ln_first) or mlp_check_desc(O, hidden, 1, act, ln_first)
    if msg:
        return (-1 if "unknown activation" in msg else -4), msg
    if O > 32 and (O if not repitch else row_pitch(O)) % 4:
        return -4, "mlp: wide inputs need a row stride that is a multiple of 4"
    for out in (A, 1):                  # launch_head_loss: the LDS-staged kernel holds 64 rows of the last hidden layer and the head
        K = hidden[-1]
        if head_kernel(hidden, out, tail_shape_ok(hidden, out, mb, ppo_opts())) == "generic" and \
                (HEAD_ROWS * (K + 1) + K * out + 2 * HEAD_ROWS * out + 2 * out) * 4 > 160 * 1024:
            return -4, "ppo head: last hidden layer too wide for the LDS-staged head kernel"
    return None


def _net_rows(O, hidden, A, act, ln_first, mb, opts, policy):
    """net_fwd_bwd of ONE network -> (paths dict, [(kernel, engine, M, N, K)] one entry per launch)"""
    nh, on = len(hidden), bool(opts["gemm_bx"]) and mb >= SPLIT_ROWS
    have = bx_mlp_images(O, hidden, act, ln_first, on)
    tail = tail_shape_ok(hidden, A, mb, opts) and {(2, 0), (2, 1)} <= have
    wide, rows = O > 32, []
    nl = nh - 1 if tail else nh
    # ---- forward (mlp_trunk_fwd)
    l12 = bool(opts["l12_fused"]) and not wide and nl >= 2 and mb >= SPLIT_ROWS and l12fwd_supported(O, hidden, act, ln_first) and \
        {(0, 0), (1, 0)} <= have
    if l12:
        first, l_next = "l12fwd", 2
        rows.append(("k_l12fwd", ENGINE_SPLIT, mb, hidden[1], 512))
    elif not wide:
        l_next = 1
        if opts["l1fwd_mfma"] and mb >= 1024 and l1fwd_mfma_supported(O, hidden, act, ln_first):
            first = "l1fwd_mfma"
            rows.append(("k_l1fwd_mfma", ENGINE_HBM, mb, 512, 0))
        else:
            first = "l1"                                 # k_l1: no profiler row
    else:
        first, l_next = "wide_ln" if ln_first else "wide", 1
        rows.append(("k_gemm_fwd", ENGINE_EXACT, mb, hidden[0], O))      # (no image of a wide first layer)
    for l in range(l_next, nl):
        rows.append(("k_gemm_fwd", ENGINE_SPLIT if (l, 0) in have else ENGINE_EXACT, mb, hidden[l], hidden[l - 1]))
    # ---- head and loss
    head = head_kernel(hidden, A, tail)
    rows.append(("k_tail", ENGINE_SPLIT, mb, TL_K3, hidden[1]) if tail else ("k_head_loss", ENGINE_HBM, mb, hidden[-1], A))
    # ---- backward (mlp_trunk_bwd)
    fuse_l1 = not wide and l1fused_supported(O, hidden, act, ln_first) and not opts["disable_l1fused"]
    merge = tail and dw_merge_ok(hidden, mb, opts)
    ldx = row_pitch(O)
    merge2 = bool(opts["dw_merge"]) and nh == 2 and wide and not ln_first and not fuse_l1 and (1, 1) in have and \
        bx_dw_usable(on, mb, hidden[0], hidden[0], hidden[1]) and bx_dw_usable(on, mb, O, ldx, hidden[0])
    l1bwd = ("k_dx_l1bwd", ENGINE_SPLIT if fuse_l1 and l1fused_bx(O, hidden, act, ln_first, have) else ENGINE_EXACT, mb, hidden[0],
             hidden[1] if nh >= 2 else 0)
    if merge2:
        rows.append(("k_gemm_dx", ENGINE_SPLIT, mb, hidden[0], hidden[1]))
        rows.append(("k_gemm_dw", ENGINE_SPLIT, O + hidden[0], hidden[0] + hidden[1], mb))
        dw = "merge2"
    else:
        if merge and fuse_l1:
            rows.append(l1bwd)
        for l in range(nh - 1, 0, -1):
            d_in, d_out = hidden[l - 1], hidden[l]
            if merge:
                if l == 1:
                    rows.append(("k_gemm_dw", ENGINE_SPLIT, hidden[0] + hidden[1], hidden[1] + hidden[2], mb))
            else:
                rows.append(("k_gemm_dw", ENGINE_SPLIT if bx_dw_usable(on, mb, d_in, d_in, d_out) else ENGINE_EXACT, d_in, d_out, mb))
            if (l == 1 and fuse_l1) or (tail and l == nh - 1):
                continue
            rows.append(("k_gemm_dx", ENGINE_SPLIT if (l, 1) in have else ENGINE_EXACT, mb, d_in, d_out))
        if fuse_l1 and not merge:
            rows.append(l1bwd)
        if wide:
            rows.append(("k_gemm_dw", ENGINE_SPLIT if bx_dw_usable(on, mb, O, ldx, hidden[0]) else ENGINE_EXACT, O, hidden[0], mb))
        dw = "merged" if merge else "separate"
    n_params = mlp_blocks(O, hidden, A, ln_first, policy)[1]
    segs = 2 * nh + (2 if ln_first else 0) + 2 + (4 if policy else 1)
    rows.append(("k_reduce_segments", ENGINE_HBM, n_params + (3 if policy else 1), segs, 0))
    no_h1 = bool(opts["dw_recompute"]) and tail and l12 and merge and hidden[0] == 512 and act == ACT_ELU
    paths = dict(tail=(tail_rows(hidden, act, mb, opts) if tail else 0), first=first, l1bwd="fused" if fuse_l1 else "unfused",
                 l1bwd_split=fuse_l1 and l1bwd[1] == ENGINE_SPLIT, dw=dw, head=head, h1_stored=not no_h1)
    return paths, rows


def _twin_rows(O, hidden, A, act, ln_first, mb, opts):
    """twin_fwd_bwd: every launch covers both networks"""
    nh = len(hidden)
    have = bx_mlp_images(O, hidden, act, ln_first, True)
    tail = tail_shape_ok(hidden, A, mb, opts)
    rows = []
    l12 = bool(opts["l12_fused"]) and l12fwd_supported(O, hidden, act, ln_first)
    rows.append(("k_l12fwd", ENGINE_SPLIT, mb, hidden[1], 512) if l12 else ("k_l1fwd_mfma", ENGINE_HBM, mb, 512, 0))
    for l in range(2 if l12 else 1, nh - 1 if tail else nh):
        rows.append(("k_gemm_fwd", ENGINE_SPLIT, mb, hidden[l], hidden[l - 1]))
    if tail:
        rows.append(("k_tail", ENGINE_SPLIT, mb, TL_K3, hidden[1]))      # (the twin head kernel k_head_loss_pc has no profiler row)
    merge = bool(opts["dw_merge"]) and tail and nh == 3
    for l in range(nh - 1, 0, -1):
        if merge:
            if l == 1:
                rows.append(("k_gemm_dw", ENGINE_SPLIT, hidden[0] + hidden[1], hidden[1] + hidden[2], mb))
        else:
            rows.append(("k_gemm_dw", ENGINE_SPLIT, hidden[l - 1], hidden[l], mb))
        if l == 1:
            break
        if not (tail and l == nh - 1):
            rows.append(("k_gemm_dx", ENGINE_SPLIT, mb, hidden[l - 1], hidden[l]))
    rows.append(("k_dx_l1bwd", ENGINE_SPLIT, mb, hidden[0], hidden[1]))
    np_, nc_ = mlp_blocks(O, hidden, A, ln_first, True)[1], mlp_blocks(O, hidden, 1, ln_first, False)[1]
    rows.append(("k_reduce_segments", ENGINE_HBM, np_ + 3 + nc_ + 1, 2 * (2 * nh + (2 if ln_first else 0) + 2) + 5, 0))
    no_h1 = l12 and bool(opts["dw_recompute"]) and merge and hidden[0] == 512 and act == ACT_ELU
    paths = dict(tail=(tail_rows(hidden, act, mb, opts) if tail else 0), first="l12fwd" if l12 else "l1fwd_mfma", l1bwd="fused",
                 l1bwd_split=True, dw="merged" if merge else "separate", head=head_kernel(hidden, A, tail), h1_stored=not no_h1)
    return paths, rows, have


def ppo_pass(O, hidden, A, act, ln_first, mb, options=None):
    """One rlx_ppo_minibatch_fwd_bwd_f32 call on mb rows (policy [O -> hidden -> A] with logstd, critic of the same trunk) ->
    dict(twin: the twin pass runs, twin_ok: it is admissible, policy / critic: the paths of each network (tail: 0 / 32 / 64 rows,
    first: l12fwd / l1fwd_mfma / l1 / wide / wide_ln, l1bwd: fused / unfused, dw: merged / separate / merge2, head: tail / fast64 /
    fast128 / fast256 / generic), rows: {(kernel, engine, M, N, K): launches} the profiler must show)."""
    hidden, opts = tuple(hidden), ppo_opts(options)
    assert ppo_refusal(O, hidden, A, act, ln_first, mb) is None
    admissible = twin_shapes_ok(O, hidden, A, act, ln_first, mb, dict(opts, ppo_twin=1))
    twin = False
    if opts["ppo_twin"] == 1 and admissible:
        tp, trows, have = _twin_rows(O, hidden, A, act, ln_first, mb, opts)
        # twin_images: both networks need every image of the pass, the fused first-layer backward's included
        twin = l1fused_bx(O, hidden, act, ln_first, have) and all({(l, 0), (l, 1)} <= have for l in range(1, len(hidden)))
    out = {}
    if twin:
        pp = cp = tp
        launches = trows
    else:
        pp, prow = _net_rows(O, hidden, A, act, ln_first, mb, opts, True)
        cp, crow = _net_rows(O, hidden, 1, act, ln_first, mb, opts, False)
        launches = prow + crow
    for r in launches:
        out[r] = out.get(r, 0) + 1
    return dict(twin=twin, twin_ok=admissible, policy=pp, critic=cp, rows=out)


# ------------------------------------------------- recurrent PPO (ppo_lstm.hip: check_lstm_desc, lstm_minibatch; rollout.hip: the decoder)
LSTM_H, LSTM_ROWS = 64, 16                     # lstm_kernels.h: hidden units of the cell, envs per workgroup of the sequence kernels
CELL_LSTM, CELL_GRU, COMBINE_CONCAT, COMBINE_FILM = 0, 1, 0, 1      # rlx_hip.h
RLX_EINVAL, RLX_EUNSUP = -1, -4
RO_ROWS, RO_MAXH, RO_MAXN = 32, 512, 256       # rollout.hip
LSTM_DEFAULTS = dict(gemm_bx=1, bx_debug=0)
GEMM_KERNELS = ("k_gemm_fwd", "k_gemm_dx", "k_gemm_dw")


def lstm_check_desc(O, A, E, H, torso, cell, combine):
    """ppo_lstm.hip check_lstm_desc, clause by clause in its order -> None, or (code, message) of the refusal"""
    D1, D2, D3 = torso
    if not 1 <= O <= 32:
        return RLX_EUNSUP, "ppo_lstm: obs_dim must be 1..32 (encoders use the small-K fused layer)"
    if H != LSTM_H:
        return RLX_EUNSUP, "ppo_lstm: lstm_hidden_dim must be 64 in this build"
    if cell not in (CELL_LSTM, CELL_GRU):
        return RLX_EINVAL, "ppo_lstm: cell must be RLX_CELL_LSTM or RLX_CELL_GRU"
    if combine not in (COMBINE_CONCAT, COMBINE_FILM):
        return RLX_EINVAL, "ppo_lstm: combine must be RLX_COMBINE_CONCAT or RLX_COMBINE_FILM"
    if not (E % 64 == 0 and 64 <= E <= 512):
        return RLX_EUNSUP, "ppo_lstm: obs_encoding_dim must be a multiple of 64"
    if not (D1 % 64 == 0 and 64 <= D1 <= 512):
        return RLX_EUNSUP, "ppo_lstm: torso[0] must be a multiple of 64 in [64, 512]"
    if not (D2 % 4 == 0 and D2 >= 4):
        return RLX_EUNSUP, "ppo_lstm: torso[1] must be a positive multiple of 4"
    if not (D3 % 4 == 0 and D3 >= 4):
        return RLX_EUNSUP, "ppo_lstm: torso[2] must be a positive multiple of 4"
    if not 1 <= A <= 64:
        return RLX_EUNSUP, "ppo_lstm: act_dim must be 1..64"
    return None


def lstm_blocks(O, A, E, torso, share, gru, film):
    """the flat layout of the recurrent policy (rlx_hip.h; lstm_layout) -> ([(name, offset, length)], n_params)"""
    H, (D1, D2, D3) = LSTM_H, torso
    K1 = E if film else E + H
    names = []
    for enc in (["enc_l"] if share else ["enc_l", "enc_o"]):
        names += [(enc + ".W", O * E), (enc + ".b", E), (enc + ".g", E), (enc + ".be", E)]
    if gru:
        names += [("gru.Wi", E * 3 * H), ("gru.bi", 3 * H), ("gru.Wh_rz", H * 2 * H), ("gru.Wh_n", H * H), ("gru.bhn", H)]
    else:
        names += [("lstm.Wi", E * 4 * H), ("lstm.Wh", H * 4 * H), ("lstm.bh", 4 * H)]
    names += [("lstm_ln.g", H), ("lstm_ln.be", H)]
    if film:
        names += [("film.W", H * 2 * E), ("film.b", 2 * E)]
    names += [("t1.W", K1 * D1), ("t1.b", D1), ("t1.g", D1), ("t1.be", D1), ("t2.W", D1 * D2), ("t2.b", D2), ("t3.W", D2 * D3), ("t3.b", D3),
              ("head.W", D3 * A), ("head.b", A), ("logstd", A)]
    out, off = [], 0
    for name, n in names:
        out.append((name, off, n))
        off += n
    return out, off


def rollout_net_ok(in_dim, hidden, out_dim):
    """rollout.hip fill_net: a feed-forward net the fused acting kernels take"""
    if not (1 <= len(hidden) <= 3 and 1 <= in_dim <= 32 and out_dim >= 1):
        return False
    if hidden[0] < 64 or hidden[0] % 64 or hidden[0] > RO_MAXH:
        return False
    for l in range(1, len(hidden)):
        if hidden[l] not in (128, 256) or hidden[l - 1] % (2 * G_BK):
            return False
    return out_dim * RO_ROWS <= 1024


def lstm_act_fused(E, torso, A, film, c_in, c_hidden, fused_recurrent_act=1):
    """rlx_ppo_lstm_act_f32: the decoder (latent LayerNorm, torso, head, sampling) and the critic run as ONE k_rollout_step launch
    (rollout_decoder_supported); otherwise layer by layer on the generic path"""
    K0, (D1, D2, D3) = E + LSTM_H, torso
    dec = K0 % 64 == 0 and 64 <= K0 <= RO_MAXN and D1 % 256 == 0 and D1 <= RO_MAXH and D2 in (128, 256) and D3 in (128, 256) and \
        A * RO_ROWS <= 1024
    return bool(fused_recurrent_act) and not film and dec and rollout_net_ok(c_in, c_hidden, 1)


def ppo_lstm_pass(O, A, E, torso, share, gru, film, T, ne, c_in=None, c_hidden=(512, 256, 128), options=None):
    """One rlx_ppo_lstm_minibatch_fwd_bwd_f32 call on T * ne rows with the critic [c_in -> c_hidden -> 1] (ELU, LayerNorm first) ->
    dict(rows: {(kernel, engine, M, N, K): launches} of the GEMM kernels (GEMM_KERNELS) the profiler must show -- the policy's dense
    layers through launch_gemm_fwd / stage_dx / stage_dw, the critic's through net_fwd_bwd --, split: the policy's images exist,
    recurrent: "split" / "exact" product in k_lstm_seq_* (None for the GRU), full_tiles: every 16-env tile of the recurrence is full)."""
    o = dict(LSTM_DEFAULTS)
    o.update(options or {})
    assert set(o) == set(LSTM_DEFAULTS)
    H, (D1, D2, D3), M = LSTM_H, torso, T * ne
    K1, gates = (E if film else E + H), (3 if gru else 4)
    bx = bool(o["gemm_bx"])
    split = bx and M >= SPLIT_ROWS            # bx_prepare_mats: t1, t2, t3 and Wi, both images (every width is a multiple of 4)
    e = ENGINE_SPLIT if split else ENGINE_EXACT
    launches = [("k_gemm_fwd", e, M, gates * H, E), ("k_gemm_fwd", e, M, D1, K1), ("k_gemm_fwd", e, M, D2, D1), ("k_gemm_fwd", e, M, D3, D2),
                ("k_gemm_dx", e, M, D2, D3), ("k_gemm_dx", e, M, D1, D2), ("k_gemm_dx", e, M, K1, D1), ("k_gemm_dx", e, M, E, gates * H)]
    dws = [(D2, D3), (D1, D2), (K1, D1)]
    if film:          # the FiLM Dense pair has no image: exact engine whatever the size
        launches += [("k_gemm_fwd", ENGINE_EXACT, M, 2 * E, H), ("k_gemm_dx", ENGINE_EXACT, M, H, 2 * E)]
        dws.append((H, 2 * E))
    dws += [(H, 2 * H), (H, H), (E, 3 * H)] if gru else [(H, 4 * H), (E, 4 * H)]
    launches += [("k_gemm_dw", ENGINE_SPLIT if bx_dw_usable(bx, M, Kd, Kd, N) else ENGINE_EXACT, Kd, N, M) for Kd, N in dws]
    if M >= SPLIT_ROWS:       # (the critic's rows: mirrored from 4096 rows on only, like ppo_pass)
        _, crow = _net_rows(O if c_in is None else c_in, tuple(c_hidden), 1, ACT_ELU, True, M, ppo_opts(dict(gemm_bx=o["gemm_bx"])), False)
        launches += [r for r in crow if r[0] in GEMM_KERNELS]
    rows = {}
    for r in launches:
        rows[r] = rows.get(r, 0) + 1
    recurrent = None if gru else ("split" if bx and not (o["bx_debug"] & 256) else "exact")
    return dict(rows=rows, split=split, recurrent=recurrent, full_tiles=ne % LSTM_ROWS == 0)
