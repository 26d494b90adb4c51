"""MPO golden vectors produced by EXECUTING the reference's own code (rl_x/algorithms/mpo/pytorch):

    python tests/golden/make_mpo_golden.py          # needs the reference checkout; writes tests/golden/mpo_reference.npz

The modules `Policy` (policy.py), `QNetwork` (q_network.py) and `DualVariables` (dual_variables.py) are loaded by file path, and the
closure `update` of `MPO.train` (mpo.py:124-267) is compiled from the reference file's AST and run against a stand-in `self` (the
helpers of make_reference_golden.py), in float64 on float32-representable inputs, with the three Adam optimisers built as the
reference builds them (mpo.py:101-103; fused=False on the CPU).  torch.randn is replaced by seeded, stored N(0, 1) draws rounded to
float32 (the critic step's [S, B, A], then the actor step's [S, 2B, A]), and so is torch.randn_like for the acting outputs
(Policy.get_action / sample_action / get_deterministic_action).  A float64 module would compute softplus(0) in float64: the policies'
`softplus0` is set to the float32 value the reference computes.  Parameters come from tests/mpo_twin.py's make_params (numpy,
seeded).  The file holds inputs and outputs only (batch, noise, scalars, metrics, the duals and their Adam moments, seeded samples of
the updated networks and their Adam moments, acting outputs), plus a `source` field.

Cases (each batch has terminations, truncations and effective n-steps 1..4):
  0 near the defaults: v +-1600, 51 atoms, penalty on;            1 v +-10 with targets past both edges of the support;
  2 action_clipping = False;                                      3 policy_init_scale 3 (samples leave [-1, 1]), max_grad_norm
    small enough that all three clips act;                        4 duals at their edges: log_eta 25 (softplus' linear branch),
    log_alpha_stddev -17.99995 with target == online policy (the step pushes it below -18: the clamp acts);
  5 policy / critic observation index sets of different widths (6 and 10 of 12 columns);
  6 past the other cases' shapes: obs 10, act 5, hidden 128, 101 atoms (odd, past one wave), B 13, S 7, an asymmetric support
    [-20, 60] with rewards past both edges, and TWO consecutive `update` calls: the three Adam optimisers carry their state from
    the first into the second (step 2, non-zero moments), fresh noise per call, the same batch.  The second call's outputs are
    stored under c6_u2_* (the sampled networks at the first call's positions: values and norms only)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_reference_golden import REF, _sampled, load_by_path, save, train_closures  # noqa: E402

import mpo_twin as tw  # noqa: E402

# (obs, act, hidden, atoms, batch, S, param seed, target seed (None: target == online), overrides)
CASES = (
    (8, 3, 64, 51, 16, 6, 41, 81, {}),
    (8, 3, 64, 21, 16, 5, 42, 82, dict(v_min=-10.0, v_max=10.0, reward_scale=12.0)),
    (8, 3, 64, 51, 16, 6, 43, 83, dict(action_clipping=False)),
    (8, 3, 64, 51, 16, 6, 44, 84, dict(policy_init_scale=3.0, max_grad_norm=1e-3)),
    (8, 3, 64, 51, 16, 6, 45, None, dict(init_log_eta=25.0, init_log_alpha_stddev=-17.99995)),
    (12, 2, 64, 51, 12, 4, 46, 86, dict(pidx=(0, 2, 3, 5, 8, 11), cidx=(1, 2, 3, 4, 5, 6, 7, 9, 10, 11))),
    (10, 5, 128, 101, 13, 7, 47, 87, dict(v_min=-20.0, v_max=60.0, reward_scale=20.0, reward_edges=(75.0, -35.0, 60.5, -20.5),
                                          n_updates=2)),
)
# the settings a case may override (every case stores all of them)
CASE_KEYS = ("v_min", "v_max", "action_clipping", "policy_init_scale", "max_grad_norm", "init_log_eta", "init_log_alpha_stddev")


def policy_modules(P):
    return [P.torso[0], P.torso[3], P.torso[5]], P.torso[1], (P.mean, P.std)


def critic_modules(Q):
    return [Q.critic[0], Q.critic[3], Q.critic[5]], Q.critic[1], (Q.critic[7],)


def flat(mods, f):
    """modules -> the flat layout of include/rlx_hip.h (rlx_mpo_desc); f maps a parameter to the tensor to store"""
    lins, ln, heads = mods
    parts = [f(lins[0].weight).T.reshape(-1), f(lins[0].bias), f(ln.weight), f(ln.bias)]
    for lin in lins[1:]:
        parts += [f(lin.weight).T.reshape(-1), f(lin.bias)]
    parts += [torch.cat([f(h.weight).T for h in heads], dim=1).reshape(-1), torch.cat([f(h.bias) for h in heads])]
    return torch.cat([p.detach().to(torch.float64).reshape(-1) for p in parts]).numpy().copy()


def load(mods, vec):
    lins, ln, heads = mods
    t = torch.from_numpy(np.asarray(vec, np.float64))
    off = 0

    def take(n):
        nonlocal off
        off += n
        return t[off - n:off]
    with torch.no_grad():
        i, o = lins[0].in_features, lins[0].out_features
        lins[0].weight.copy_(take(i * o).reshape(i, o).T)
        lins[0].bias.copy_(take(o))
        ln.weight.copy_(take(o))
        ln.bias.copy_(take(o))
        for lin in lins[1:]:
            i, o = lin.in_features, lin.out_features
            lin.weight.copy_(take(i * o).reshape(i, o).T)
            lin.bias.copy_(take(o))
        H, n = heads[0].in_features, sum(h.out_features for h in heads)
        W, b = take(H * n).reshape(H, n), take(n)
        c = 0
        for h in heads:
            h.weight.copy_(W[:, c:c + h.out_features].T)
            h.bias.copy_(b[c:c + h.out_features])
            c += h.out_features
    assert off == t.numel(), (off, t.numel())


def adam_flat(opt, mods, key):
    return flat(mods, lambda prm: opt.state[prm][key] if prm in opt.state else torch.zeros_like(prm))


def make_mpo():
    import torch.nn.functional as F
    sys.path.insert(0, REF)
    pol = load_by_path("rl_x/algorithms/mpo/pytorch/policy.py", "ref_mpo_policy")
    qn = load_by_path("rl_x/algorithms/mpo/pytorch/q_network.py", "ref_mpo_q")
    dv = load_by_path("rl_x/algorithms/mpo/pytorch/dual_variables.py", "ref_mpo_duals")
    dtype = torch.float64
    torch.set_default_dtype(dtype)
    out = {"source": "reference:rl_x/algorithms/mpo/pytorch (executed)", "n_cases": len(CASES)}
    raw_randn, raw_randn_like = torch.randn, torch.randn_like
    sp = types.SimpleNamespace
    sp0 = float(torch.nn.functional.softplus(torch.zeros(1, dtype=torch.float32)).item())
    try:
        for case, (O, A, H, NA, B, S, seed, tseed, over) in enumerate(CASES):
            k = "c%d_" % case
            hp = dict(tw.HP, action_sampling_number=S, **{n: over[n] for n in CASE_KEYS if n in over})
            g = torch.Generator().manual_seed(700 + case)
            r32 = lambda *sh: raw_randn(*sh, generator=g, dtype=torch.float64).to(torch.float32).to(dtype)
            pidx = np.asarray(over.get("pidx", range(O)), np.int64)
            cidx = np.asarray(over.get("cidx", range(O)), np.int64)
            low = np.linspace(-1.0, -2.0, A).astype(np.float32)
            high = np.linspace(1.0, 3.0, A).astype(np.float32)
            env = sp(single_action_space=sp(low=low, high=high, shape=(A,)), single_observation_space=sp(shape=(O,)))
            mk_pol = lambda: pol.Policy(env, hp["policy_init_scale"], hp["policy_min_scale"], hp["action_clipping"], hp["action_rescaling"], H,
                                        "cpu", pidx).to(dtype)
            mk_q = lambda: qn.QNetwork(env, NA, hp["action_clipping"], H, "cpu", cidx).to(dtype)
            P, TP, Q, TQ = mk_pol(), mk_pol(), mk_q(), mk_q()
            for m in (P, TP):
                m.softplus0 = sp0
            p, q = tw.make_params(seed, len(pidx), len(cidx), A, H, NA)
            tp, tq = (p, q) if tseed is None else tw.make_params(tseed, len(pidx), len(cidx), A, H, NA)
            load(policy_modules(P), p)
            load(policy_modules(TP), tp)
            load(critic_modules(Q), q)
            load(critic_modules(TQ), tq)
            cfg = sp(algorithm=sp(**{n: hp[n] for n in ("init_log_eta", "init_log_alpha_mean", "init_log_alpha_stddev",
                                                        "init_log_penalty_temperature")}))
            duals = dv.DualVariables(cfg, A, "cpu")
            d0 = tw.init_duals(A, hp)
            with torch.no_grad():
                duals.log_eta.copy_(torch.tensor(d0[:1]))
                duals.log_alpha_mean.copy_(torch.tensor(d0[1:1 + A]))
                duals.log_alpha_stddev.copy_(torch.tensor(d0[1 + A:1 + 2 * A]))
                duals.log_penalty_temperature.copy_(torch.tensor(d0[1 + 2 * A:]))
            states, next_states = r32(B, O), r32(B, O)
            actions = (r32(B, A) * 0.8).to(torch.float32).to(dtype)
            rewards = (r32(B) * over.get("reward_scale", 2.0)).to(torch.float32).to(dtype)
            dones = (torch.rand(B, generator=g) < 0.25).to(dtype)
            truncs = (torch.rand(B, generator=g) < 0.5).to(dtype) * dones       # a truncation is also a done (replay_buffer.py)
            nsteps = torch.randint(1, 5, (B,), generator=g).to(dtype)
            dones[:2], truncs[:2], nsteps[:4] = torch.tensor([1.0, 1.0]), torch.tensor([0.0, 1.0]), torch.tensor([1.0, 2.0, 3.0, 4.0])
            if "reward_edges" in over:          # rows 4.. (not done): targets past both edges of the support
                e = over["reward_edges"]
                rewards[4:4 + len(e)] = torch.tensor(e)
                dones[4:4 + len(e)] = 0.0
                truncs[4:4 + len(e)] = 0.0
            eps_c, eps_a, eps_act = r32(S, B, A), r32(S, 2 * B, A), r32(B, A)
            queue = []

            def randn(*shape, **kw):
                e = queue.pop(0)
                sh = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
                assert tuple(e.shape) == sh, (e.shape, sh)
                return e.clone()

            def randn_like(x, **kw):
                e = queue.pop(0)
                assert tuple(e.shape) == tuple(x.shape), (e.shape, x.shape)
                return e.to(x.dtype)
            torch.randn, torch.randn_like = randn, randn_like
            me = sp(actor=P, target_actor=TP, critic=sp(q=Q, q_target=TQ), duals=duals, device="cpu", bf16_mixed_precision_training=False,
                    action_sampling_number=S, nr_atoms=NA, gamma=hp["gamma"], v_min=hp["v_min"], v_max=hp["v_max"],
                    max_grad_norm=hp["max_grad_norm"], float_epsilon=hp["float_epsilon"], action_clipping=hp["action_clipping"],
                    epsilon_non_parametric=hp["epsilon_non_parametric"], epsilon_parametric_mu=hp["epsilon_parametric_mu"],
                    epsilon_parametric_sigma=hp["epsilon_parametric_sigma"], epsilon_penalty=hp["epsilon_penalty"],
                    min_log_temperature=hp["min_log_temperature"], min_log_alpha=hp["min_log_alpha"],
                    q_support=torch.linspace(hp["v_min"], hp["v_max"], NA),
                    log_num_actions=torch.log(torch.tensor(S, dtype=torch.float32)),
                    log_2pi=torch.log(torch.tensor(2.0 * np.pi, dtype=torch.float32)))      # mpo.py:113-115
            me.actor_optimizer = torch.optim.Adam(P.parameters(), lr=hp["agent_learning_rate"], fused=False)
            me.critic_optimizer = torch.optim.Adam(Q.parameters(), lr=hp["agent_learning_rate"], fused=False)
            me.dual_optimizer = torch.optim.Adam(duals.parameters(), lr=hp["dual_learning_rate"], fused=False)
            ns = {"torch": torch, "F": F, "np": np, "self": me, "autocast": torch.autocast}
            (update,) = train_closures("rl_x/algorithms/mpo/pytorch/mpo.py", ["update"], ns)
            out.update({k + "obs_dim": O, k + "act_dim": A, k + "hidden": H, k + "nr_atoms": NA, k + "batch": B, k + "S": S,
                        k + "param_seed": seed, k + "target_seed": -1 if tseed is None else tseed, k + "pidx": pidx, k + "cidx": cidx,
                        k + "low": low, k + "high": high, k + "duals0": d0, k + "states": states, k + "next_states": next_states,
                        k + "actions": actions, k + "rewards": rewards, k + "dones": dones, k + "truncs": truncs, k + "nsteps": nsteps,
                        k + "eps_c": eps_c, k + "eps_a": eps_a, k + "eps_act": eps_act})
            out.update({k + n: hp[n] for n in CASE_KEYS})
            # --- acting (policy.py:71-97) on the states
            with torch.no_grad():
                mean, std = P.get_action(states)
                queue.append(eps_act)
                a_s, pa_s = P.sample_action(states)
                pa_d = P.get_deterministic_action(states)
            out.update({k + "act_mean": mean, k + "act_std": std, k + "act_sample": a_s, k + "act_sample_proc": pa_s, k + "act_det_proc": pa_d})
            # --- one update (mpo.py:124-267); a second one with fresh noise when the case asks for it
            for call in range(over.get("n_updates", 1)):
                u = k if call == 0 else k + "u2_"
                if call == 0:
                    ec, ea = eps_c, eps_a
                else:
                    ec, ea = r32(S, B, A), r32(S, 2 * B, A)
                    out.update({u + "eps_c": ec, u + "eps_a": ea})
                queue.extend([ec, ea])
                met = update(states, next_states, actions, rewards, dones, truncs, nsteps)
                assert not queue
                # the closure returns them in the order of mpo.py:249-267; stored in the order of the logged dict (mpo.py:389-407)
                met = [float(x.detach()) for x in met]
                out[u + "metrics"] = np.array([met[i] for i in (0, 1, 2, 8, 9, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 15, 16)])
                pm_, qm_ = policy_modules(P), critic_modules(Q)
                for name, mods, opt, sd in (("p", pm_, me.actor_optimizer, 500), ("q", qm_, me.critic_optimizer, 600)):
                    for n_, vec, sd_ in ((name + "_after", flat(mods, lambda t: t), sd + case),
                                         (name + "m_after", adam_flat(opt, mods, "exp_avg"), sd + 10 + case),
                                         (name + "v_after", adam_flat(opt, mods, "exp_avg_sq"), sd + 20 + case)):
                        smp = _sampled(u + n_, vec, sd_)
                        if call:        # the same positions as the first call's: the indices are stored once
                            assert np.array_equal(smp.pop(u + n_ + "_idx"), out[k + n_ + "_idx"])
                        out.update(smp)
                dl = [duals.log_eta, duals.log_alpha_mean, duals.log_alpha_stddev, duals.log_penalty_temperature]
                st = me.dual_optimizer.state
                out[u + "duals_after"] = torch.cat([x.detach().reshape(-1) for x in dl]).numpy()
                for key in ("exp_avg", "exp_avg_sq"):
                    out[u + "duals_" + key] = torch.cat([(st[x][key] if x in st else torch.zeros_like(x)).reshape(-1) for x in dl]).numpy()
            torch.randn, torch.randn_like = raw_randn, raw_randn_like
    finally:
        torch.randn, torch.randn_like = raw_randn, raw_randn_like
        torch.set_default_dtype(torch.float32)
    save("mpo_reference.npz", out)


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("the reference checkout is needed to regenerate this fixture (%s)" % REF)
    make_mpo()
