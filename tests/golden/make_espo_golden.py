"""ESPO golden vectors produced by EXECUTING the reference's own code (rl_x/algorithms/espo/pytorch):

    python tests/golden/make_espo_golden.py          # needs the reference checkout; writes tests/golden/espo_reference.npz

The modules `Policy` (policy.py) and `Critic` (critic.py) are loaded by file path, and the closures `policy_loss_fn`, `critic_loss_fn`
and `calculate_gae_advantages_and_returns` of `ESPO.train` (espo.py:112-158) are compiled from the reference file's AST and run
against a stand-in `self` (the helpers of make_reference_golden.py), in float64 on float32-representable inputs, with the two Adam
optimisers built as the reference builds them (espo.py:87-88; fused=False on the CPU).  Only the five-line epoch loop with its
`break` (espo.py:240-278) is restated here.  Parameters come from tests/espo_twin.py's make_params (numpy, seeded); the minibatch
rows are the draws of np.random.default_rng(seed).choice(B, mb, replace=False), stored.  The file holds inputs and outputs only
(rollout arrays, indices, scalars, per-epoch metrics, epochs_run, seeded samples of the updated networks and their Adam moments,
get_logprob_entropy / get_deterministic_action outputs), plus a `source` field.

The generator asserts its own conditions: at every executed epoch ratio_delta is at least 1e-3 (relative) away from
max_ratio_delta; in median cases with an even minibatch the two middle values differ by at least 1e-3 relative; each stop lands on
the epoch its case names.

Cases (obs 8, act 3, hidden 64, B = 12 x 8 = 96 rows, 6 epochs, learning rate 2e-3 unless stated):
  0 mb 16, the threshold is never reached;                          1 mean operator, stop after epoch 3;
  2 median operator, mb 16 (even), stop after epoch 2;             3 median operator, mb 15 (odd), stop after epoch 3;
  4 entropy_coef 0.01 with max_grad_norm 1e-3: both clips act;     5 policy / critic index sets of different widths (6 and 10 of 12);
  6 obs 10, act 5, hidden 128, mb 13, stop after epoch 0;          7 stop after the last epoch."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_reference_golden import REF, _sampled, load_by_path, save, train_closures  # noqa: E402

import espo_twin as tw  # noqa: E402

# (obs, act, hidden, T, N, mb, epochs, param seed, stop epoch (None: never), overrides)
CASES = (
    (8, 3, 64, 12, 8, 16, 6, 51, None, dict(max_ratio_delta=0.25, learning_rate=3e-4)),
    (8, 3, 64, 12, 8, 16, 6, 52, 3, dict(max_ratio_delta=0.105)),
    (8, 3, 64, 12, 8, 16, 6, 53, 2, dict(max_ratio_delta=0.06, delta_calc_operator="median")),
    (8, 3, 64, 12, 8, 15, 6, 54, 3, dict(max_ratio_delta=0.0965, delta_calc_operator="median")),
    (8, 3, 64, 12, 8, 16, 6, 55, None, dict( entropy_coef=0.01, max_grad_norm=1e-3)),
    (12, 2, 64, 12, 8, 16, 6, 56, None, dict(pidx=(0, 2, 3, 5, 8, 11), cidx=(1, 2, 3, 4, 5, 6, 7, 9, 10, 11))),
    (10, 5, 128, 13, 8, 13, 6, 57, 0, dict(max_ratio_delta=0.02)),
    (8, 3, 64, 12, 8, 16, 6, 58, 5, dict(max_ratio_delta=0.15)),
)
CASE_KEYS = ("max_ratio_delta", "delta_calc_operator", "entropy_coef", "critic_coef", "max_grad_norm", "learning_rate", "gamma", "gae_lambda")
N_SAMPLED = 300


def policy_parts(P):
    return [P.policy_mean[0], P.policy_mean[2], P.policy_mean[4]], (P.policy_logstd,)


def critic_parts(C):
    return [C.critic[0], C.critic[2], C.critic[4]], ()


def flat(parts, f):
    """modules -> the flat layout of include/rlx_hip.h (arch A); f maps a parameter to the tensor to store"""
    lins, extra = parts
    out = []
    for lin in lins:
        out += [f(lin.weight).T.reshape(-1), f(lin.bias).reshape(-1)]
    out += [f(e).reshape(-1) for e in extra]
    return torch.cat([p.detach().to(torch.float64).reshape(-1) for p in out]).numpy().copy()


def load(parts, vec):
    lins, extra = parts
    t = torch.from_numpy(np.asarray(vec, np.float64))
    off = 0
    with torch.no_grad():
        for lin in lins:
            i, o = lin.in_features, lin.out_features
            lin.weight.copy_(t[off:off + i * o].reshape(i, o).T)
            off += i * o
            lin.bias.copy_(t[off:off + o])
            off += o
        for e in extra:
            e.copy_(t[off:off + e.numel()].reshape(e.shape))
            off += e.numel()
    assert off == t.numel(), (off, t.numel())


def adam_flat(opt, parts, key):
    return flat(parts, lambda prm: opt.state[prm][key] if prm in opt.state else torch.zeros_like(prm))


def make_espo(probe=False):
    import torch.nn as nn
    sys.path.insert(0, REF)
    pol = load_by_path("rl_x/algorithms/espo/pytorch/policy.py", "ref_espo_policy")
    cri = load_by_path("rl_x/algorithms/espo/pytorch/critic.py", "ref_espo_critic")
    dtype = torch.float64
    torch.set_default_dtype(dtype)
    sp = types.SimpleNamespace
    out = {"source": "reference:rl_x/algorithms/espo/pytorch (executed)", "n_cases": len(CASES)}
    try:
        for case, (O, A, H, T, N, mb, E, seed, stop, over) in enumerate(CASES):
            k = "c%d_" % case
            hp = dict(tw.HP, learning_rate=2e-3)
            hp.update({n: over[n] for n in CASE_KEYS if n in over})
            B = T * N
            g = torch.Generator().manual_seed(900 + case)
            r32 = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64).to(torch.float32).to(dtype)
            f32 = lambda x: x.to(torch.float32).to(dtype)
            pidx = np.asarray(over.get("pidx", range(O)), np.int64)
            cidx = np.asarray(over.get("cidx", range(O)), np.int64)
            low = np.linspace(-1.0, -2.0, A).astype(np.float32)
            high = np.linspace(1.0, 3.0, A).astype(np.float32)
            env = sp(single_action_space=sp(low=low, high=high, shape=(A,)), single_observation_space=sp(shape=(O,)))
            P = pol.Policy(env, 1.0, True, H, "cpu", pidx).to(dtype)
            C = cri.Critic(env, H, "cpu", cidx).to(dtype)
            p0, c0 = tw.make_params(seed, len(pidx), len(cidx), A, H)
            load(policy_parts(P), p0)
            load(critic_parts(C), c0)
            op = sp(mean=torch.mean, median=torch.median)
            me = sp(policy=P, critic=C, bf16_mixed_precision_training=False, delta_calc_operator=getattr(op, hp["delta_calc_operator"]),
                    entropy_coef=hp["entropy_coef"], critic_coef=hp["critic_coef"], max_grad_norm=hp["max_grad_norm"])
            me.policy_optimizer = torch.optim.Adam(P.parameters(), lr=hp["learning_rate"], fused=False)       # espo.py:87-88
            me.critic_optimizer = torch.optim.Adam(C.parameters(), lr=hp["learning_rate"], fused=False)
            ns = {"torch": torch, "nn": nn, "np": np, "self": me, "autocast": torch.autocast}
            policy_loss_fn, critic_loss_fn, gae = train_closures(
                "rl_x/algorithms/espo/pytorch/espo.py", ["policy_loss_fn", "critic_loss_fn", "calculate_gae_advantages_and_returns"], ns)
            # --- the rollout: states, actions around the policy's mean, old log-probs a little off the policy's own, GAE
            states = r32(T, N, O)
            rewards = r32(T, N)
            terminations = (torch.rand(T, N, generator=g) < 0.1).to(dtype)
            with torch.no_grad():
                values = f32(C.get_value(states).squeeze(-1) + 0.3 * r32(T, N))
                next_values = f32(C.get_value(f32(states + 0.1 * r32(T, N, O))).squeeze(-1))
                flat_states = states.reshape(B, O)
                mean = P.policy_mean(flat_states[:, pidx])
                actions = f32(mean + torch.exp(P.policy_logstd) * r32(B, A))
                lp0, ent0 = P.get_logprob_entropy(flat_states, actions)
                det0 = P.get_deterministic_action(flat_states)
                log_probs = f32(lp0 + 0.05 * r32(B))
                adv, ret = gae(rewards, terminations, values, next_values, hp["gamma"], hp["gae_lambda"])
            out.update({k + "gae_advantages": adv, k + "gae_returns": ret})
            advantages, returns = f32(adv.reshape(B)), f32(ret.reshape(B))
            idx = tw.draw_indices(np.random.default_rng(seed), B, mb, E)
            out.update({k + "obs_dim": O, k + "act_dim": A, k + "hidden": H, k + "T": T, k + "N": N, k + "mb": mb, k + "max_epochs": E,
                        k + "param_seed": seed, k + "pidx": pidx, k + "cidx": cidx, k + "low": low, k + "high": high, k + "states": states,
                        k + "rewards": rewards, k + "terminations": terminations, k + "values": values, k + "next_values": next_values,
                        k + "actions": actions, k + "log_probs": log_probs, k + "advantages": advantages, k + "returns": returns,
                        k + "idx": idx, k + "logprob0": lp0, k + "entropy0": ent0, k + "det_action0": det0,
                        k + "stop_epoch": -1 if stop is None else stop})
            out.update({k + n: hp[n] for n in CASE_KEYS})
            # --- the epoch loop (espo.py:240-278)
            rows = []
            for epoch in range(E):
                mbi = torch.from_numpy(idx[epoch].astype(np.int64))
                dev = None
                if hp["delta_calc_operator"] == "median" and mb % 2 == 0:      # the two middle values, before the step moves the policy
                    with torch.no_grad():
                        lp, _ = P.get_logprob_entropy(flat_states[mbi], actions[mbi])
                        dev = torch.sort(torch.abs(torch.exp(lp - log_probs[mbi]) - 1))[0]
                ratio_delta, pg_loss, entropy_loss, approx_kl_div, policy_grad_norm = policy_loss_fn(
                    flat_states[mbi], actions[mbi], log_probs[mbi], advantages[mbi])
                critic_loss, critic_grad_norm = critic_loss_fn(flat_states[mbi], returns[mbi])
                rows.append([float(x.detach()) for x in (pg_loss, critic_loss, entropy_loss, ratio_delta, approx_kl_div, policy_grad_norm,
                                                critic_grad_norm)])
                rd, thr = float(ratio_delta), hp["max_ratio_delta"]
                if probe:
                    print(case, epoch, "ratio_delta %.6f" % rd, "" if dev is None else "middle %.6f %.6f" % (dev[mb // 2 - 1], dev[mb // 2]))
                else:
                    assert abs(rd - thr) >= 1e-3 * abs(thr), (case, epoch, rd, thr)
                    if dev is not None:
                        lo, hi = float(dev[mb // 2 - 1]), float(dev[mb // 2])
                        assert rd == lo and hi - lo >= 1e-3 * hi, (case, epoch, lo, hi, rd)
                if ratio_delta > thr and not probe:
                    break
            if not probe:
                assert len(rows) == (E if stop is None else stop + 1), (case, len(rows), stop)
                if stop is not None:
                    assert rows[-1][3] > hp["max_ratio_delta"]
            out[k + "metrics"] = np.array(rows)
            out[k + "epochs_run"] = len(rows)
            for name, parts, opt, sd in (("p", policy_parts(P), me.policy_optimizer, 500), ("c", critic_parts(C), me.critic_optimizer, 600)):
                for n_, vec, sd_ in ((name + "_after", flat(parts, lambda t: t), sd + case),
                                     (name + "m_after", adam_flat(opt, parts, "exp_avg"), sd + 10 + case),
                                     (name + "v_after", adam_flat(opt, parts, "exp_avg_sq"), sd + 20 + case)):
                    out.update(_sampled(k + n_, vec, sd_, n=N_SAMPLED))
    finally:
        torch.set_default_dtype(torch.float32)
    if not probe:
        save("espo_reference.npz", out)


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("the reference checkout is needed to regenerate this fixture (%s)" % REF)
    make_espo(probe="--probe" in sys.argv)
