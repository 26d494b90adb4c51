"""FastTD3 golden vectors produced by EXECUTING the reference's own code (rl_x/algorithms/fasttd3/pytorch):

    python tests/golden/make_fasttd3_golden.py          # needs the reference checkout; writes tests/golden/fasttd3_reference.npz

The modules `Policy` (policy.py) and `QNetwork` (q_network.py) are loaded by file path, and the closures `critic_loss_fn` /
`policy_loss_fn` of `FastTD3.train` (fasttd3.py:104-225) are compiled from the reference file's AST and run against a stand-in
`self` (the helpers of make_reference_golden.py), in float64 on float32-representable inputs, with AdamW optimisers built as the
reference builds them (fasttd3.py:88-89, default betas; fused=False on the CPU).  Parameters come from tests/fasttd3_twin.py's
make_params (numpy, seeded): a test regenerates them.  The N(0, 1) draws of torch.randn_like (exploration noise in get_action,
smoothing noise in critic_loss_fn) come from a seeded generator, rounded to float32, and are stored.  The file holds inputs and
outputs only (batch, noise, scalars, norms + seeded samples of gradients and updated parameters), plus a `source` field.

Cases: 0 clipped double Q off; 1 clipped double Q on (the default) with action_clipping_and_rescaling; 2 clipped double Q on
with gradient clipping active (max_grad_norm below both gradient norms)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_reference_golden import REF, _sampled, load_by_path, save, train_closures  # noqa: E402

import fasttd3_twin  # noqa: E402

CASES = (  # (obs, act, nr_atoms, batch, clipped, param seed, max_grad_norm, action clipping and rescaling)
    (9, 3, 21, 48, False, 21, -1.0, False),
    (7, 2, 101, 32, True, 22, -1.0, True),
    (9, 3, 21, 48, True, 23, 0.05, False),
)


def _load_relu(seq, flat, in_dim, hidden, out_dim, dtype):
    """flat layout -> the Linear layers of the reference's nn.Sequential (ReLU / Tanh in between)."""
    lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
    assert len(lins) == len(hidden) + 1
    off, d = 0, in_dim
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    with torch.no_grad():
        for lin, h in zip(lins, list(hidden) + [out_dim]):
            lin.weight.copy_(t(flat[off:off + d * h].reshape(d, h).T)); off += d * h
            lin.bias.copy_(t(flat[off:off + h])); off += h
            d = h
    assert off == flat.size, (off, flat.size)


def _flat_relu(seq, grads=False):
    f = (lambda p: p.grad) if grads else (lambda p: p.detach())
    parts = []
    for lin in [m for m in seq if isinstance(m, torch.nn.Linear)]:
        parts += [f(lin.weight).T.contiguous().reshape(-1), f(lin.bias).reshape(-1)]
    return torch.cat(parts).to(torch.float64).numpy().copy()


def make_fasttd3():
    import torch.nn.functional as F
    sys.path.insert(0, REF)
    pol_mod = load_by_path("rl_x/algorithms/fasttd3/pytorch/policy.py", "ref_ftd3_policy")
    q_mod = load_by_path("rl_x/algorithms/fasttd3/pytorch/q_network.py", "ref_ftd3_q")
    dtype = torch.float64
    torch.set_default_dtype(dtype)
    out = {"source": "reference:rl_x/algorithms/fasttd3/pytorch (executed)", "n_cases": len(CASES)}
    raw_randn_like = torch.randn_like
    for case, (O, A, NA, B, clipped, seed, mgn, clip_act) in enumerate(CASES):
        sp = types.SimpleNamespace
        low, high = np.linspace(-1.0, -0.5, A).astype(np.float32), np.linspace(1.0, 2.0, A).astype(np.float32)
        env = sp(single_action_space=sp(low=low, high=high, shape=(A,)), single_observation_space=sp(shape=(O,)))
        hp = dict(gamma=0.97, tau=0.1, v_min=-10.0, v_max=10.0, learning_rate=3e-4, weight_decay=0.1, smoothing_epsilon=0.2,
                  smoothing_clip_value=0.3)
        policy = pol_mod.Policy(env, clip_act, "cpu", np.arange(O)).to(dtype)
        qs = [q_mod.QNetwork(env, NA, "cpu", np.arange(O)).to(dtype) for _ in range(4)]
        pflat, qflat = fasttd3_twin.make_params(seed, O, A, NA)
        _load_relu(policy.policy, pflat, O, fasttd3_twin.POLICY_HIDDEN, A, dtype)
        for q, fl in zip(qs, qflat):
            _load_relu(q.critic, fl, O + A, fasttd3_twin.CRITIC_HIDDEN, NA, dtype)
        critic = sp(q1=qs[0], q2=qs[1], q1_target=qs[2], q2_target=qs[3])
        me = sp(policy=policy, critic=critic, gamma=hp["gamma"], v_min=hp["v_min"], v_max=hp["v_max"], nr_atoms=NA,
                smoothing_epsilon=hp["smoothing_epsilon"], smoothing_clip_value=hp["smoothing_clip_value"],
                clipped_double_q_learning=clipped, bf16_mixed_precision_training=False, max_grad_norm=mgn, device=torch.device("cpu"),
                q_support=torch.linspace(hp["v_min"], hp["v_max"], NA))
        kw = dict(lr=hp["learning_rate"], weight_decay=hp["weight_decay"], fused=False)
        me.policy_optimizer = torch.optim.AdamW(policy.parameters(), **kw)
        me.q_optimizer = torch.optim.AdamW(list(qs[0].parameters()) + list(qs[1].parameters()), **kw)
        ns = {"torch": torch, "F": F, "self": me, "autocast": torch.autocast}
        policy_loss_fn, critic_fn = train_closures("rl_x/algorithms/fasttd3/pytorch/fasttd3.py", ["policy_loss_fn", "critic_loss_fn"], ns)
        g = torch.Generator().manual_seed(170 + case)
        r32 = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64).to(torch.float32).to(dtype)
        s, s2 = r32(B, O), r32(B, O)
        a = torch.clamp(r32(B, A) * 0.6, -1.0, 1.0).to(torch.float32).to(dtype)
        rew = (r32(B) * 3.0).to(torch.float32).to(dtype)
        done = (torch.rand(B, generator=g) < 0.3).to(dtype)
        trunc = (torch.rand(B, generator=g) < 0.5).to(dtype) * done
        nst = torch.randint(1, 4, (B,), generator=g).to(dtype)
        scales = (torch.rand(B, 1, generator=g, dtype=torch.float64) * 0.4 + 0.001).to(torch.float32).to(dtype)
        noise = []

        def randn_like(x, **k):
            e = torch.randn(x.shape, generator=g, dtype=torch.float64).to(torch.float32).to(x.dtype)   # float32-representable
            noise.append(e.clone())
            return e
        torch.randn_like = randn_like
        try:
            k = "c%d_" % case
            out.update({k + "obs_dim": O, k + "act_dim": A, k + "nr_atoms": NA, k + "batch": B, k + "clipped": int(clipped),
                        k + "param_seed": seed, k + "max_grad_norm": mgn, k + "clip_and_rescale": int(clip_act), k + "low": low,
                        k + "high": high, k + "states": s, k + "next_states": s2, k + "actions": a, k + "rewards": rew, k + "dones": done,
                        k + "truncations": trunc, k + "n_steps": nst, k + "noise_scales": scales[:, 0]})
            out.update({k + n: v for n, v in hp.items()})
            # --- acting (policy.py:57-66): deterministic, then with the per-env noise scales
            with torch.no_grad():
                out[k + "deterministic_action"] = policy.get_action(s)[0]
                action, processed = policy.get_action(s, scales)
                out.update({k + "act_noise": noise[-1], k + "action": action, k + "processed_action": processed,
                            k + "q1_logits": qs[0](s, a), k + "q2_logits": qs[1](s, a)})
            # --- critic step (fasttd3.py:140-225)
            q_loss, q_min, q_max, c_gn = critic_fn(s, s2, a, rew, done, trunc, nst)
            out.update({k + "noise_next": noise[-1], k + "q_loss": q_loss.detach(), k + "q_min": q_min.detach(), k + "q_max": q_max.detach(),
                        k + "critic_grad_norm": torch.as_tensor(c_gn).detach()})
            gq = np.concatenate([_flat_relu(q.critic, grads=True) for q in qs[:2]])
            qa = np.concatenate([_flat_relu(q.critic) for q in qs[:2]])
            out.update(_sampled(k + "gcritic", gq, 100 + case))
            out.update(_sampled(k + "qparams_after", qa, 200 + case))
            # --- Polyak update of the targets (fasttd3.py:316-320), after every critic step
            with torch.no_grad():
                for qo, qt in ((qs[0], qs[2]), (qs[1], qs[3])):
                    for param, target_param in zip(qo.parameters(), qt.parameters()):
                        target_param.data.mul_(1.0 - hp["tau"]).add_(param.data, alpha=hp["tau"])
            ta = np.concatenate([_flat_relu(q.critic) for q in qs[2:]])
            out.update(_sampled(k + "qtarget_after", ta, 300 + case))
            # --- policy step on the updated critics (fasttd3.py:105-136, :324)
            p_loss, p_gn = policy_loss_fn(s)
            out.update({k + "policy_loss": p_loss.detach(), k + "policy_grad_norm": torch.as_tensor(p_gn).detach()})
            out.update(_sampled(k + "gpolicy", _flat_relu(policy.policy, grads=True), 400 + case))
            out.update(_sampled(k + "pparams_after", _flat_relu(policy.policy), 500 + case))
        finally:
            torch.randn_like = raw_randn_like
    torch.set_default_dtype(torch.float32)
    save("fasttd3_reference.npz", out)


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("the reference checkout is needed to regenerate this fixture (%s)" % REF)
    make_fasttd3()
