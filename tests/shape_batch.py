"""What the FastSAC and FastTD3 shape cases (fastsac_cases.py, fasttd3_cases.py) draw the same way: the observation columns of the
policy and of the critics, and a replay batch of float32-representable values with terminations, truncations and n-steps 1..4."""
import numpy as np


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def index_sets(rng, O, Op, Oc):
    """(policy columns sorted, critic columns in drawn order) of an O-wide observation; None: all of them"""
    pidx = None if Op is None else np.sort(rng.choice(O, Op, replace=False))
    cidx = None if Oc is None else rng.choice(O, Oc, replace=False)
    return pidx, cidx


def draw_batch(rng, B, O, A, h, action, pidx, cidx):
    """-> (batch with the POLICY's columns [states, next_states, actions, rewards, dones, truncations, n_steps], the critics'
    (states, next_states) or None when both see every column).  action(raw standard normal [B, A]) -> the stored actions;
    a fifth of the rows are done, half of those truncated; the first rows carry n-steps 1, 2, 3, 4; rewards within max|v| / 4"""
    s, s2 = f32(rng.standard_normal((B, O))), f32(rng.standard_normal((B, O)))
    a = f32(action(rng.standard_normal((B, A))))
    dones = (rng.random(B) < 0.2).astype(np.float64)
    truncs = dones * (rng.random(B) < 0.5)
    nsteps = rng.integers(1, 5, B).astype(np.float64)
    nsteps[:4] = [1.0, 2.0, 3.0, 4.0][:B]
    rewards = f32(rng.standard_normal(B) * min(3.0, max(abs(h["v_min"]), abs(h["v_max"])) / 4))
    cols = lambda x, idx: x if idx is None else np.ascontiguousarray(x[:, idx])
    batch = [cols(s, pidx), cols(s2, pidx), a, rewards, dones, truncs, nsteps]
    cbatch = (cols(s, cidx), cols(s2, cidx)) if pidx is not None or cidx is not None else None
    return batch, cbatch
