"""REPPO golden vectors produced by EXECUTING the reference's own code (rl_x/algorithms/reppo/pytorch):

    python tests/golden/make_reppo_golden.py          # needs the reference checkout; writes tests/golden/reppo_reference.npz

The modules `Policy` (policy.py), `Critic` (critic.py) and `ObservationNormalizer` (observation_normalizer.py) are loaded by file
path, and the closures `critic_loss_fn`, `policy_loss_fn`, `rollout_evaluate_next` and `compute_td_lambda_targets` of
`REPPO.train` (reppo.py:118-219) are compiled from the reference file's AST and run against a stand-in `self` (the helpers of
make_reference_golden.py), in float64 on float32-representable inputs, with Adam optimisers built as the reference builds them
(reppo.py:97-98; fused=False on the CPU).  A float64 nn.RMSNorm(eps=None) would use float64's epsilon: the modules' eps is set to
float32's, what the float32 reference computes.  Parameters come from tests/reppo_twin.py's make_params (numpy, seeded).  The
N(0, 1) draws of torch.randn_like come from a seeded generator, rounded to float32, and are stored.  The file holds inputs and
outputs only (batch, noise, scalars + seeded samples of gradients, updated parameters and Adam moments), plus a `source` field.

Cases: 0 every row inside the KL bound (old policy == policy); 1 an old policy that differs, kl_bound between two rows' KL
values near the median (a mix of both branches of the `where`); 2 gradient clipping active (max_grad_norm far below both
gradient norms); 3 policy hidden 128 != critic hidden 64, 151 bins over v +-100 (the reference's support), policy_min_std 0.05,
auxiliary_loss_coefficient 0.5, targets beyond +-100 and on both edges (the clamp), an old policy that differs.  Every case has
terminations and truncations in its minibatch.  Cases 0-2 store one `hidden` and use HP's settings; a case with overrides
stores `policy_hidden`, `critic_hidden` and the CASE_KEYS it runs with."""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_reference_golden import REF, _sampled, load_by_path, save, train_closures  # noqa: E402

import reppo_twin as tw  # noqa: E402

CASES = (  # (obs, act, hidden, nr_bins, batch, kl samples, param seed, old-policy seed, max_grad_norm, overrides)
    (9, 3, 64, 21, 40, 4, 31, None, 0.5, {}),
    (7, 2, 64, 51, 48, 6, 32, 77, 0.5, {}),
    (9, 3, 64, 21, 40, 4, 33, 78, 0.002, {}),
    # hidden (policy, critic), the reference's bins and value range, a minimum std and an auxiliary coefficient != 1; targets
    # beyond +-v_max and one on each edge (the clamp)
    (9, 3, (128, 64), 151, 48, 5, 34, 79, 0.5, dict(v_min=-100.0, v_max=100.0, policy_min_std=0.05, auxiliary_loss_coefficient=0.5,
                                                    wide_targets=True)),
)
HP = dict(gamma=0.99, gae_lambda=0.95, v_min=-10.0, v_max=10.0, learning_rate=3e-4, policy_min_std=0.0, auxiliary_loss_coefficient=1.0,
          init_entropy_coefficient=0.05, init_kl_coefficient=0.02, target_entropy_multiplier=0.5)
# the settings a case may override; a case that overrides one also stores it (and both widths), the others keep their keys
CASE_KEYS = ("v_min", "v_max", "policy_min_std", "auxiliary_loss_coefficient")


def policy_linears(P):
    lins = [m for m in P.torso if isinstance(m, torch.nn.Linear)]
    rms = [m for m in P.torso if isinstance(m, torch.nn.RMSNorm)]
    return [(lins[0], rms[0]), (lins[1], rms[1]), (P.head, None)]


def critic_linears(C):
    out = []
    for seq in (C.encoder, C.critic_head, C.pred_head):
        lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
        rms = [m for m in seq if isinstance(m, torch.nn.RMSNorm)]
        out += [(lins[0], rms[0]), (lins[1], None)]
    # flat order (include/rlx_hip.h): encoder, critic_head, pred_head -- as listed
    return out


def flat(blocks, extra, f):
    parts = []
    for lin, rms in blocks:
        parts += [f(lin.weight).T.contiguous().reshape(-1), f(lin.bias).reshape(-1)]
        if rms is not None:
            parts.append(f(rms.weight).reshape(-1))
    parts += [f(e).reshape(-1) for e in extra]
    return torch.cat([p.to(torch.float64) for p in parts]).numpy().copy()


def load(blocks, extra, vec):
    t = torch.from_numpy(np.asarray(vec, np.float64))
    off = 0
    with torch.no_grad():
        for lin, rms in blocks:
            i, o = lin.in_features, lin.out_features
            lin.weight.copy_(t[off:off + i * o].reshape(i, o).T); off += i * o
            lin.bias.copy_(t[off:off + o]); off += o
            if rms is not None:
                rms.weight.copy_(t[off:off + o]); off += o
        for e in extra:
            e.copy_(t[off:off + e.numel()].reshape(e.shape)); off += e.numel()
    assert off == t.numel(), (off, t.numel())


def adam_state(opt, params, key):
    return [opt.state[p][key] if p in opt.state else torch.zeros_like(p) for p in params]


def make_reppo():
    import torch.nn as nn
    sys.path.insert(0, REF)
    pol = load_by_path("rl_x/algorithms/reppo/pytorch/policy.py", "ref_reppo_policy")
    cri = load_by_path("rl_x/algorithms/reppo/pytorch/critic.py", "ref_reppo_critic")
    onm = load_by_path("rl_x/algorithms/reppo/pytorch/observation_normalizer.py", "ref_reppo_obs_norm")
    dtype = torch.float64
    torch.set_default_dtype(dtype)
    out = {"source": "reference:rl_x/algorithms/reppo/pytorch (executed)", "n_cases": len(CASES)}
    raw_randn_like = torch.randn_like
    sp = types.SimpleNamespace
    rel = "rl_x/algorithms/reppo/pytorch/reppo.py"
    try:
        for case, (O, A, H, NB, B, K, seed, old_seed, mgn, over) in enumerate(CASES):
            k = "c%d_" % case
            Hp, Hc = H if isinstance(H, tuple) else (H, H)
            hpc = dict(HP, **{n: over[n] for n in CASE_KEYS if n in over})
            g = torch.Generator().manual_seed(500 + case)
            r32 = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64).to(torch.float32).to(dtype)
            low, high = -np.ones(A, np.float32), np.ones(A, np.float32)
            env = sp(single_action_space=sp(low=low, high=high, shape=(A,)), single_observation_space=sp(shape=(O,)))
            P = pol.Policy(env, Hp, hpc["policy_min_std"], HP["init_entropy_coefficient"], HP["init_kl_coefficient"], np.arange(O), "cpu").to(dtype)
            OP = pol.Policy(env, Hp, hpc["policy_min_std"], HP["init_entropy_coefficient"], HP["init_kl_coefficient"], np.arange(O), "cpu").to(dtype)
            C = cri.Critic(env, Hc, NB, hpc["v_min"], hpc["v_max"], np.arange(O), "cpu").to(dtype)
            for m in list(P.modules()) + list(OP.modules()) + list(C.modules()):
                if isinstance(m, nn.RMSNorm):
                    m.eps = tw.RMS_EPS
            p, q = tw.make_params(seed, O, O, A, Hp, Hc, NB, hpc["v_min"], hpc["v_max"], HP["init_entropy_coefficient"], HP["init_kl_coefficient"])
            old_p = p if old_seed is None else tw.make_params(old_seed, O, O, A, Hp, Hc, NB, hpc["v_min"], hpc["v_max"])[0]
            pb, ob, cb = policy_linears(P), policy_linears(OP), critic_linears(C)
            pe, oe, ce = [P.log_entropy_coefficient, P.log_kl_coefficient], [OP.log_entropy_coefficient, OP.log_kl_coefficient], [C.zero_distribution]
            load(pb, pe, p)
            load(ob, oe, old_p)
            load(cb, ce, q)
            for prm in OP.parameters():
                prm.requires_grad = False
            states, next_states = r32(B, O), r32(B, O)
            actions = torch.tanh(r32(B, A)).to(torch.float32).to(dtype)
            rewards, targets = (r32(B) * 2.0).to(torch.float32).to(dtype), (r32(B) * 3.0).to(torch.float32).to(dtype)
            next_features = (r32(B, Hc) * 0.5).to(torch.float32).to(dtype)
            terms = (torch.rand(B, generator=g) < 0.2).to(dtype)
            truncs = (torch.rand(B, generator=g) < 0.15).to(dtype) * (1.0 - terms)
            eps_eval, eps_new, eps_old = r32(B, A), r32(B, A), r32(K, B, A)
            if over.get("wide_targets"):      # TD-lambda targets past the support: several beyond +-v_max, one on each edge
                v = hpc["v_max"]
                targets = (r32(B) * (0.6 * v)).to(torch.float32).to(dtype)
                targets[:4] = torch.tensor([v, -v, 2.5 * v, -1.375 * v], dtype=dtype)
            hpc.update(nr_kl_samples=K, max_grad_norm=mgn, target_entropy=A * HP["target_entropy_multiplier"], kl_bound=0.1)
            if old_seed is not None:          # kl_bound between two rows' KL values near the median, far from both
                kl = tw.policy_loss(torch.tensor(p, dtype=dtype), tw.policy_layout(O, A, Hp), old_p, q, tw.critic_layout(O, A, Hc, NB),
                                    states.numpy(), states.numpy(), eps_new, eps_old, hpc)[2]
                s = np.sort(kl)
                i = max(range(B // 4, 3 * B // 4), key=lambda j: s[j + 1] - s[j])
                hpc["kl_bound"] = float(np.float32(0.5 * (s[i] + s[i + 1])))
            queue = []

            def randn_like(x, **kw):
                e = queue.pop(0)
                assert tuple(e.shape) == tuple(x.shape), (e.shape, x.shape)
                return e.to(x.dtype)
            torch.randn_like = randn_like
            v_min, v_max = hpc["v_min"], hpc["v_max"]
            bw = (v_max - v_min) / (NB - 1)
            me = sp(policy=P, old_policy=OP, critic=C, gamma=HP["gamma"], v_min=v_min, v_max=v_max, kl_bound=hpc["kl_bound"],
                    auxiliary_loss_coefficient=hpc["auxiliary_loss_coefficient"], nr_kl_samples=K, target_entropy=hpc["target_entropy"],
                    max_grad_norm=mgn, bf16_mixed_precision_training=False)
            me.policy_optimizer = torch.optim.Adam(P.parameters(), lr=HP["learning_rate"], fused=False)
            me.critic_optimizer = torch.optim.Adam(C.parameters(), lr=HP["learning_rate"], fused=False)
            ns = {"torch": torch, "nn": nn, "math": math, "self": me, "autocast": torch.autocast,
                  "hl_gauss_centers": torch.linspace(v_min, v_max, NB),
                  "hl_gauss_support": torch.linspace(v_min - bw / 2, v_max + bw / 2, NB + 1), "hl_gauss_sigma": bw * 0.75}
            critic_fn, policy_fn, eval_next, td = train_closures(
                rel, ["critic_loss_fn", "policy_loss_fn", "rollout_evaluate_next", "compute_td_lambda_targets"], ns)
            if over:
                out.update({k + "policy_hidden": Hp, k + "critic_hidden": Hc}, **{k + n: hpc[n] for n in CASE_KEYS})
            else:
                out[k + "hidden"] = H
            out.update({k + "obs_dim": O, k + "act_dim": A, k + "nr_bins": NB, k + "batch": B, k + "nr_kl_samples": K,
                        k + "param_seed": seed, k + "old_seed": -1 if old_seed is None else old_seed, k + "max_grad_norm": mgn,
                        k + "kl_bound": hpc["kl_bound"], k + "states": states, k + "next_states": next_states, k + "actions": actions,
                        k + "rewards": rewards, k + "targets": targets, k + "next_features": next_features, k + "terms": terms,
                        k + "truncs": truncs, k + "eps_eval": eps_eval, k + "eps_new": eps_new, k + "eps_old": eps_old})
            # --- rollout_evaluate_next (reppo.py:195-204)
            queue.append(eps_eval)
            with torch.no_grad():
                nf, nv, sr = eval_next(next_states, rewards)
            out.update({k + "eval_next_features": nf, k + "eval_next_value": nv, k + "eval_soft_reward": sr})
            # --- one critic step (reppo.py:119-136), then one policy step on the updated critic (reppo.py:376-380)
            cm = critic_fn(states, actions, targets, rewards, next_features, terms, truncs)
            out[k + "critic_metrics"] = np.array([float(x) for x in cm])
            cparams = list(C.parameters())
            gq = flat(cb, ce, lambda t: t.grad)
            out.update(_sampled(k + "gcritic", gq, 100 + case))
            out.update(_sampled(k + "qparams_after", flat(cb, ce, lambda t: t.detach()), 200 + case))
            st = dict(zip(cparams, adam_state(me.critic_optimizer, cparams, "exp_avg_sq")))
            out.update(_sampled(k + "qv_after", flat(cb, ce, lambda t: st[t]), 300 + case))
            for prm in cparams:
                prm.requires_grad = False
            queue.extend([eps_new, eps_old])
            pm = policy_fn(states)
            for prm in cparams:
                prm.requires_grad = True
            out[k + "policy_metrics"] = np.array([float(x) for x in pm])
            out.update(_sampled(k + "gpolicy", flat(pb, pe, lambda t: t.grad), 400 + case))
            out.update(_sampled(k + "pparams_after", flat(pb, pe, lambda t: t.detach()), 500 + case))
            assert not queue
            # --- compute_td_lambda_targets (reppo.py:207-219) on a [T, N] rollout with dones
            T, N = 11, 6
            sr_, nv_ = r32(T, N), r32(T, N) * 5.0
            te_ = (torch.rand(T, N, generator=g) < 0.15).to(dtype)
            tr_ = (torch.rand(T, N, generator=g) < 0.1).to(dtype) * (1.0 - te_)
            out.update({k + "td_soft_rewards": sr_, k + "td_next_values": nv_, k + "td_terms": te_, k + "td_truncs": tr_,
                        k + "td_targets": td(sr_, nv_, te_, tr_, HP["gamma"], HP["gae_lambda"])})
        # --- ObservationNormalizer (float32 buffers and count): five updates, then normalize
        norm = onm.ObservationNormalizer((5,), True, "cpu")
        g = torch.Generator().manual_seed(600)
        xs = [(torch.randn(64, 5, generator=g, dtype=torch.float64) * torch.arange(1, 6) + 2.0).to(torch.float32) for _ in range(5)]
        for x in xs:
            norm.update(x)
        out.update({"norm_inputs": torch.stack(xs), "norm_mean": norm.mean, "norm_var": norm.var, "norm_count": norm.count,
                    "norm_out": norm.normalize(xs[-1])})
    finally:
        torch.randn_like = raw_randn_like
        torch.set_default_dtype(torch.float32)
    save("reppo_reference.npz", out)


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("the reference checkout is needed to regenerate this fixture (%s)" % REF)
    make_reppo()
