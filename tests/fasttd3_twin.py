"""CPU twin (float64) of FastTD3's networks and update steps -- test infrastructure for tests/test_fasttd3_*.py and
tests/test_gpu_fasttd3.py.

Follows rl_x/algorithms/fasttd3/pytorch:
    policy.py:38-47      Linear(O,512)-ReLU, Linear(512,256)-ReLU, Linear(256,128)-ReLU, Linear(128,A)-Tanh
    policy.py:57-66      get_action: a = policy(x) + randn * noise_scales (per env); processed = a, or with
                         action_clipping_and_rescaling low + 0.5 (clamp(a, -1, 1) + 1)(high - low)
    q_network.py:28-39   Linear(Oc + A,1024)-ReLU, Linear(1024,512)-ReLU, Linear(512,256)-ReLU, Linear(256, nr_atoms) on [obs | action]
    fasttd3.py:140-225   critic_loss_fn: next action clamp(policy(s') + clamp(eps * smoothing_epsilon, +-clip), -1, 1) (no gradient,
                         no target policy), categorical projection of the n-step target WITHOUT an entropy term (oracle/c51.py with
                         alpha = 0), clipped double Q, q_loss = q1_loss + q2_loss, one AdamW over both critics
    fasttd3.py:316-320   Polyak after every critic step
    fasttd3.py:105-136   policy_loss_fn: loss = -mean(min(q1, q2)) (or the mean of the two) of the critics' expected values
Optimiser and Polyak helpers: oracle/fastsac.py (torch.optim.AdamW, clip_grad_norm_).  Flat layout: rlx_mlp_desc with
ln_first = 0, has_logstd = 0 -- per layer W[in, out] row-major, b[out]; then the head.

Pinned by tests/golden/fasttd3_reference.npz: outputs of the reference's own modules and closures executed in float64
(tests/golden/make_fasttd3_golden.py), checked in tests/test_fasttd3_twin.py."""
import numpy as np
import torch

from oracle import c51
from oracle.fastsac import adamw, clip_grad_norm, polyak

POLICY_HIDDEN = (512, 256, 128)
CRITIC_HIDDEN = (1024, 512, 256)


def param_count(in_dim, hidden, out_dim):
    n, d = 0, in_dim
    for h in list(hidden) + [out_dim]:
        n += d * h + h
        d = h
    return n


def make_params(seed, obs_dim, act_dim, nr_atoms, critic_obs_dim=None, policy_hidden=POLICY_HIDDEN, critic_hidden=CRITIC_HIDDEN):
    """Deterministic test parameters in the flat layout: (policy, [q1, q2, q1_target, q2_target]) float32 arrays drawn from numpy's
    PCG64 -- the fixture generator loads exactly these into the reference's modules, a test rebuilds them from the seed.  The
    targets differ from the online critics (a Polyak-averaged state, as after some training)."""
    rng = np.random.default_rng(seed)
    oc = obs_dim if critic_obs_dim is None else critic_obs_dim

    def net(in_dim, hidden, out_dim, head_scale):
        parts, d = [], in_dim
        for h in hidden:
            parts += [rng.standard_normal((d, h)) * np.sqrt(2.0 / d), 0.1 * rng.standard_normal(h)]
            d = h
        parts += [head_scale * rng.standard_normal((d, out_dim)) / np.sqrt(d), 0.1 * rng.standard_normal(out_dim)]
        return np.concatenate([x.reshape(-1) for x in parts]).astype(np.float32)
    policy = net(obs_dim, policy_hidden, act_dim, 0.5)
    critics = [net(oc + act_dim, critic_hidden, nr_atoms, 1.0) for _ in range(4)]
    return policy, critics


def forward(flat, in_dim, hidden, out_dim, x, keep=None):
    """flat, x: torch tensors.  -> head output [M, out_dim] of the ReLU network.  keep (a list) receives (input rows, pre-activation)
    of every hidden layer; a pre-activation that takes part in a backward keeps its gradient (.grad after it)."""
    off, d, h = 0, in_dim, x
    for li, width in enumerate(list(hidden) + [out_dim]):
        W = flat[off:off + d * width].reshape(d, width); off += d * width
        b = flat[off:off + width]; off += width
        x_in = h
        h = h @ W + b
        if li < len(hidden):
            if keep is not None:
                if h.requires_grad:
                    h.retain_grad()
                keep.append((x_in, h))
            h = torch.relu(h)
        d = width
    return h


def _t(a, dtype=np.float64):
    return torch.tensor(np.asarray(a, dtype=dtype))


def policy_action(pflat, obs_dim, act_dim, obs, hidden=POLICY_HIDDEN, keep=None):
    return torch.tanh(forward(pflat, obs_dim, hidden, act_dim, obs, keep))


def critic_logits(qflat, obs_dim, act_dim, nr_atoms, obs, act, hidden=CRITIC_HIDDEN, keep=None):
    return forward(qflat, obs_dim + act_dim, hidden, nr_atoms, torch.cat([obs, act], dim=1), keep)


def act(pflat, obs_dim, act_dim, obs, eps, noise_scales, low=None, high=None, hidden=POLICY_HIDDEN):
    """Policy.get_action with the given N(0, 1) draws eps [N, A] (noise_scales None: deterministic).  -> (action, processed)"""
    a = policy_action(_t(pflat), obs_dim, act_dim, _t(obs), hidden).numpy()
    if noise_scales is not None:
        a = a + np.asarray(eps, np.float64) * np.asarray(noise_scales, np.float64).reshape(-1, 1)
    if low is None:
        return a, a
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    return a, low + 0.5 * (np.clip(a, -1.0, 1.0) + 1.0) * (high - low)


def critic_step(pflat, q1, q2, t1, t2, obs_dim, act_dim, nr_atoms, batch, noise_next, hp, clipped, critic_batch=None,
                policy_hidden=POLICY_HIDDEN, critic_hidden=CRITIC_HIDDEN, dtype=np.float64, trace=None):
    """batch = (states, next_states, actions, rewards, dones, truncations, n_steps) with the POLICY's observation columns;
    critic_batch = (critic states, critic next states) or None (the same columns).  obs_dim: the critic's observation width.
    dtype: the precision the whole step is evaluated in (np.float32: what float32 alone costs).  trace (a list): receives
    forward's `keep` records of every network pass, in call order.
    -> dict(q_loss, q_min, q_max, g_q1, g_q2, next_actions)"""
    _t = lambda x: torch.tensor(np.asarray(x, dtype=dtype))
    s, s2, a, rew, done, trunc, nst = (_t(x) for x in batch)
    cs, cs2 = (s, s2) if critic_batch is None else (_t(critic_batch[0]), _t(critic_batch[1]))
    with torch.no_grad():
        pin = s2.shape[1]
        noise = torch.clamp(_t(noise_next) * hp["smoothing_epsilon"], -hp["smoothing_clip_value"], hp["smoothing_clip_value"])
        a2 = torch.clamp(policy_action(_t(pflat), pin, act_dim, s2, policy_hidden, trace) + noise, -1.0, 1.0)
        nl1 = critic_logits(_t(t1), obs_dim, act_dim, nr_atoms, cs2, a2, critic_hidden, trace).numpy()
        nl2 = critic_logits(_t(t2), obs_dim, act_dim, nr_atoms, cs2, a2, critic_hidden, trace).numpy()
    zero = np.zeros(rew.shape[0], dtype)
    args = (rew.numpy(), done.numpy(), trunc.numpy(), nst.numpy(), zero, 0.0, hp["gamma"], hp["v_min"], hp["v_max"])
    p1, v1 = c51.project(nl1, *args)
    p2, v2 = c51.project(nl2, *args)
    if clipped:
        tgt1 = tgt2 = np.where((v1 < v2)[:, None], p1, p2)
    else:
        tgt1, tgt2 = p1, p2
    Q1, Q2 = _t(q1).requires_grad_(True), _t(q2).requires_grad_(True)
    l1 = critic_logits(Q1, obs_dim, act_dim, nr_atoms, cs, a, critic_hidden, trace)
    l2 = critic_logits(Q2, obs_dim, act_dim, nr_atoms, cs, a, critic_hidden, trace)
    loss = -(_t(tgt1) * torch.log_softmax(l1, dim=1)).sum(dim=1).mean() - (_t(tgt2) * torch.log_softmax(l2, dim=1)).sum(dim=1).mean()
    loss.backward()
    return dict(q_loss=float(loss.detach()), q_min=float(v1.min()), q_max=float(v1.max()), g_q1=Q1.grad.numpy(), g_q2=Q2.grad.numpy(),
                next_actions=a2.numpy(), q1_logits=l1.detach().numpy(), q2_logits=l2.detach().numpy(), target1=tgt1, target2=tgt2,
                p1=p1, p2=p2, v1=v1, v2=v2)


def policy_step(pflat, q1, q2, obs_dim, act_dim, nr_atoms, states, hp, clipped, critic_states=None, policy_hidden=POLICY_HIDDEN,
                critic_hidden=CRITIC_HIDDEN, dtype=np.float64, trace=None):
    """dtype, trace: as in critic_step (the atoms z stay float64).  -> dict(policy_loss, g_policy, q_value, actions)"""
    _t = lambda x: torch.tensor(np.asarray(x, dtype=dtype))
    s = _t(states)
    cs = s if critic_states is None else _t(critic_states)
    P = _t(pflat).requires_grad_(True)
    a = policy_action(P, s.shape[1], act_dim, s, policy_hidden, trace)
    z = torch.linspace(hp["v_min"], hp["v_max"], nr_atoms, dtype=torch.float64)
    v1 = (torch.softmax(critic_logits(_t(q1), obs_dim, act_dim, nr_atoms, cs, a, critic_hidden, trace), dim=1) * z).sum(dim=1)
    v2 = (torch.softmax(critic_logits(_t(q2), obs_dim, act_dim, nr_atoms, cs, a, critic_hidden, trace), dim=1) * z).sum(dim=1)
    q = torch.minimum(v1, v2) if clipped else (v1 + v2) / 2.0
    loss = -q.mean()
    loss.backward()
    return dict(policy_loss=float(loss.detach()), g_policy=P.grad.numpy(), q_value=q.detach().numpy(), actions=a.detach().numpy())


def critic_update(pflat, qparams, qm, qv, qtarget, step, obs_dim, act_dim, nr_atoms, batch, noise_next, hp, clipped, critic_batch=None,
                  **kw):
    """critic_step + clip_grad_norm_ + AdamW over both critics (flat [q1 | q2]) + Polyak.  step: 1-based optimizer step.
    -> (qparams, qm, qv, qtarget, metrics [q_loss, q_min, q_max, critic_grad_norm], critic_step dict)"""
    nq = qparams.size // 2
    q1, q2, t1, t2 = qparams[:nq], qparams[nq:], qtarget[:nq], qtarget[nq:]
    r = critic_step(pflat, q1, q2, t1, t2, obs_dim, act_dim, nr_atoms, batch, noise_next, hp, clipped, critic_batch, **kw)
    g, norm = clip_grad_norm(np.concatenate([r["g_q1"], r["g_q2"]]), hp["max_grad_norm"])
    qp, qm, qv = adamw(np.asarray(qparams, np.float64), g, qm, qv, step, hp["learning_rate"], hp["weight_decay"], 0.9, 0.999)
    qt = polyak(np.asarray(qtarget, np.float64), qp, hp["tau"])
    return qp, qm, qv, qt, np.array([r["q_loss"], r["q_min"], r["q_max"], norm]), r


def policy_update(pflat, pm, pv, step, qparams, obs_dim, act_dim, nr_atoms, states, hp, clipped, critic_states=None, **kw):
    """policy_step + clip_grad_norm_ + AdamW.  -> (pparams, pm, pv, metrics [policy_loss, policy_grad_norm], policy_step dict)"""
    nq = qparams.size // 2
    r = policy_step(pflat, qparams[:nq], qparams[nq:], obs_dim, act_dim, nr_atoms, states, hp, clipped, critic_states, **kw)
    g, norm = clip_grad_norm(r["g_policy"], hp["max_grad_norm"])
    pp, pm, pv = adamw(np.asarray(pflat, np.float64), g, pm, pv, step, hp["learning_rate"], hp["weight_decay"], 0.9, 0.999)
    return pp, pm, pv, np.array([r["policy_loss"], norm]), r
