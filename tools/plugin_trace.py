#!/usr/bin/env python
"""Bit-for-bit trace of the five plugins on the net_pass layer (fastsac.hip, fasttd3.hip, mpo.hip, fastmpo.hip, reppo.hip) through
their public surface only, so that one file runs on two commits and the results can be compared.  One MI355X, small shapes.

    python tools/plugin_trace.py record DIR [CASE PREFIX ...]   # DIR/trace.json and one <case>.model per plugin
    python tools/plugin_trace.py compare DIR_A DIR_B            # == on everything recorded; wall times side by side; exit 1 on a difference
    python tools/plugin_trace.py load DIR          # load every <case>.model of DIR with THIS tree's plugin, compare _STATE with DIR's trace

An array is recorded as (dtype, shape, SHA-256 of its bytes, float64 sum): equal digests are equal bits, which is what np.array_equal
asks and a little more (it tells -0 from 0), and the parameter vectors of twelve cases stay out of the files; arrays of up to 64 elements
are kept as lists too, so a difference in a key or a counter can be read.

Per case: `_STATE` and `key` after construction; after train(): `_STATE`, `key`, the counters, the ring / pos / size or the b_*
buffers, the normaliser statistics; every sink.write as (step, keys in order, values) without the `time/` keys; the checkpoint's
(key, dtype, shape) list; the returns of test(2) on the loaded checkpoint.  Then train()'s wall time on three fresh models (the
recorded run is the warm-up): median, min, max.  Evaluation, saving and learning-rate annealing are on in every case."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-x_amd"))

import numpy as np  # noqa: E402

ENV = dict(nr_envs=32, obs_dim=24, act_dim=4, horizon=12)
STEPS = 12                                                   # vector steps of the off-policy cases
COLUMNS = (np.arange(0, 10), np.arange(6, 24))               # policy / critic observation index sets
TWO_PHASE = dict(batch_size=64, buffer_size_per_env=8, learning_starts=3, nr_atoms=51, nr_critic_updates_per_policy_update=2,
                 nr_policy_updates_per_step=2, total_timesteps=32 * STEPS, logging_frequency=32 * 4, evaluation_frequency=32 * 8,
                 save_frequency=32 * 4, anneal_learning_rate=True)
MPO = dict(batch_size=64, buffer_size=32 * 8, learning_starts=32 * 3, n_steps=2, optimize_every_n_steps=2, target_network_update_period=3,
           actor_update_period=4, action_sampling_number=5, nr_hidden_units=64, total_timesteps=32 * STEPS, logging_frequency=32 * 4,
           evaluation_frequency=32 * 8, anneal_agent_learning_rate=True, anneal_dual_learning_rate=True)
FASTMPO = dict(batch_size=64, buffer_size_per_env=8, learning_starts=3, n_steps=1, total_timesteps=32 * STEPS, logging_frequency=32 * 4,
               evaluation_and_save_frequency=32 * 4, evaluation_active=True, nr_policy_updates_per_step=2,
               nr_critic_updates_per_policy_update=2, anneal_critic_learning_rate=True, anneal_policy_learning_rate=True,
               anneal_dual_learning_rate=True)
REPPO = dict(nr_steps=4, nr_epochs=2, nr_minibatches=2, policy_hidden_dim=64, critic_hidden_dim=64, nr_bins=51, nr_kl_samples=4,
             total_timesteps=3 * 32 * 4, evaluation_frequency=32 * 4, evaluation_episodes=4, anneal_learning_rate=True)
# name -> (algorithm, environment, algorithm flags, index sets?, checkpoint file)
CASES = {}
for _alg in ("fastsac.hip", "fasttd3.hip"):
    for _n, _cols in ((1, False), (3, False), (1, True)):
        CASES[f"{_alg}-n{_n}" + ("-columns" if _cols else "")] = (_alg, "synthetic.random_obs", dict(TWO_PHASE, n_steps=_n), _cols, "latest.model")
CASES["mpo.hip-torch"] = ("mpo.hip", "synthetic.random_obs", MPO, False, "best.model")
CASES["mpo.hip-numpy"] = ("mpo.hip", "synthetic.numpy_obs", MPO, False, "best.model")
CASES["fastmpo.hip-dual"] = ("fastmpo.hip", "synthetic.random_obs", FASTMPO, False, "latest.model")
CASES["fastmpo.hip-single"] = ("fastmpo.hip", "synthetic.random_obs",
                               dict(FASTMPO, dual_critic=False, critic_network_type="mpo", policy_network_type="fasttd3", action_clipping=True,
                                    action_rescaling="normal", n_steps=3, collect_data_with_online_policy=True), False, "latest.model")
CASES["reppo.hip"] = ("reppo.hip", "synthetic.random_obs", REPPO, False, "best.model")
CASES["reppo.hip-columns"] = ("reppo.hip", "synthetic.random_obs", REPPO, True, "best.model")
KEEP_MODEL = ("fastsac.hip-n1-columns", "fasttd3.hip-n1-columns", "mpo.hip-numpy", "fastmpo.hip-single", "reppo.hip-columns")
COUNTERS = ("critic_count", "policy_count", "nr_updates", "opt_counts", "opt_count", "nr_iterations_done", "pos", "size")


def make(case, run_path):
    """(model class, config, train env, eval env) of a case, every one fresh"""
    import importlib
    from rlx_amd.runner.config_dict import ConfigDict
    from rlx_amd.runner.default_config import get_config as runner_cfg
    from rlx_amd.algorithms.algorithm_manager import get_algorithm_config, get_algorithm_model_class
    from rlx_amd.environments.environment_manager import get_environment_config, get_environment_create_train_and_eval_env
    alg, env_name, flags, columns, _ = CASES[case]
    importlib.import_module("rlx_amd.algorithms." + alg)
    importlib.import_module("rlx_amd.environments." + env_name)
    config = ConfigDict()
    config.runner = runner_cfg("train")
    config.runner.save_model = True
    config.algorithm = get_algorithm_config(alg)
    config.environment = get_environment_config(env_name)
    for k, v in ENV.items():
        config.environment[k] = v
    for k, v in flags.items():
        config.algorithm[k] = v
    env, eval_env = get_environment_create_train_and_eval_env(env_name)(config)
    if columns:
        env.policy_observation_indices, env.critic_observation_indices = COLUMNS
    if alg in ("fastsac.hip", "fasttd3.hip", "reppo.hip"):
        eval_env = env                                       # as their end-to-end tests run them: snapshot / restore on the training env
    return get_algorithm_model_class(alg), config, env, eval_env


def _host(x):
    a = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x))
    rec = [str(a.dtype), list(a.shape), hashlib.sha256(a.tobytes()).hexdigest(), float(a.astype(np.float64).sum())]
    return rec + [a.reshape(-1).tolist()] if a.size <= 64 else rec


def _state(m, arrays, prefix):
    for k in m._STATE + tuple(k for k in ("norm_mean", "norm_var", "norm_std", "norm_count") if hasattr(m, k)) + ("key",):
        arrays[prefix + k] = _host(getattr(m, k))


def record_case(case, out, arrays, lists):
    import tempfile
    run_path = tempfile.mkdtemp(prefix="plugin_trace_")
    cls, config, env, eval_env = make(case, run_path)
    m = cls(config, env, eval_env, run_path, None)
    _state(m, arrays, case + "/init/")
    writes, real_write = [], m.sink.write

    def write(step, scalars):
        kept = [(k, float(v)) for k, v in scalars.items() if not k.startswith("time/")]
        writes.append([int(step), [k for k, _ in kept], [v for _, v in kept]])
        real_write(step, scalars)
    m.sink.write = write
    t0 = time.perf_counter()
    m.train()
    first = time.perf_counter() - t0
    _state(m, arrays, case + "/trained/")
    lists[case + "/counters"] = {k: np.asarray(getattr(m, k)).tolist() for k in COUNTERS if hasattr(m, k)}
    for i, x in enumerate(getattr(m, "ring", ())):
        arrays[f"{case}/trained/ring{i}"] = _host(x)
    for k, v in sorted(vars(m).items()):
        if k.startswith("b_") and hasattr(v, "detach"):
            arrays[f"{case}/trained/{k}"] = _host(v)
    lists[case + "/writes"] = writes
    m.save()
    path = os.path.join(m.save_path, CASES[case][4])
    ckpt = np.load(path, allow_pickle=False)
    lists[case + "/checkpoint"] = [[k, str(ckpt[k].dtype), list(ckpt[k].shape)] for k in ckpt.files]
    if case in KEEP_MODEL:
        with open(path, "rb") as src, open(os.path.join(out, case + ".model"), "wb") as dst:
            dst.write(src.read())
    config.runner.load_model = path
    m2 = cls.load(config, env, eval_env, run_path, None, [])
    _state(m2, arrays, case + "/loaded/")
    lists[case + "/test"] = [float(x) for x in m2.test(2)]
    times = []
    for _ in range(3):
        cls, config, env, eval_env = make(case, run_path)
        m = cls(config, env, eval_env, run_path, None)
        t0 = time.perf_counter()
        m.train()
        times.append(time.perf_counter() - t0)
    lists[case + "/seconds"] = dict(first=first, median=float(np.median(times)), min=min(times), max=max(times))
    print(case, "train() s: median %.4f min %.4f max %.4f (first %.4f)" % (np.median(times), min(times), max(times), first), flush=True)


def record(out, only):
    os.makedirs(out, exist_ok=True)
    arrays, lists = {}, {}
    for case in CASES:
        if not only or any(case.startswith(o) for o in only):
            record_case(case, out, arrays, lists)
    with open(os.path.join(out, "trace.json"), "w") as f:
        json.dump(dict(arrays=arrays, lists=lists), f, indent=1)


def _same(a, b):
    """== on nested lists / dicts with NaN equal to NaN (an evaluation without a finished episode reports NaN)"""
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (a != a and b != b)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    return a == b


def compare(dir_a, dir_b):
    ta, tb = (json.load(open(os.path.join(d, "trace.json"))) for d in (dir_a, dir_b))
    a, b, la, lb = ta["arrays"], tb["arrays"], ta["lists"], tb["lists"]
    bad = sorted(set(a) ^ set(b)) + sorted(set(la) ^ set(lb))
    bad += [k for k in a if k in b and not _same(a[k], b[k])]
    bad += [k for k in la if k in lb and not k.endswith("/seconds") and not _same(la[k], lb[k])]
    print(f"{len(a)} arrays, {sum(not k.endswith('/seconds') for k in la)} lists compared; different: {bad if bad else 'none'}")
    slower = []
    for k in la:
        if k.endswith("/seconds") and k in lb:
            sa, sb = la[k], lb[k]
            over = sb["median"] - sa["median"] > sa["max"] - sa["min"]
            slower += [k] if over else []
            print("%-28s A median %.4f (spread %.4f)   B median %.4f (spread %.4f)%s" % (
                k[:-8], sa["median"], sa["max"] - sa["min"], sb["median"], sb["max"] - sb["min"], "   B SLOWER THAN A's SPREAD ALLOWS" if over else ""))
    print("B's median above A's by more than A's spread:", slower if slower else "none")
    return 1 if bad else 0


def load(src):
    ref = json.load(open(os.path.join(src, "trace.json")))["arrays"]
    bad = []
    for case in CASES:
        path = os.path.join(src, case + ".model")
        if not os.path.exists(path):
            continue
        cls, config, env, eval_env = make(case, "/tmp/plugin_trace_load")
        config.runner.save_model = False
        config.runner.load_model = path
        m = cls.load(config, env, eval_env, "/tmp/plugin_trace_load", None, [])
        got = {}
        _state(m, got, case + "/trained/")
        bad += [k for k, v in got.items() if not _same(v, ref[k])]
        print(case, "loaded:", len(got), "arrays", flush=True)
    print("different from the recorded state:", bad if bad else "none")
    return 1 if bad else 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "record" and len(sys.argv) >= 3:
        record(sys.argv[2], sys.argv[3:])
    elif mode == "compare" and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif mode == "load" and len(sys.argv) == 3:
        sys.exit(load(sys.argv[2]))
    else:
        sys.exit(__doc__)
