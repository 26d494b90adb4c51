"""CPU: `python bench.py --gpus N` (N > 1, no WORLD_SIZE) turns itself into the launcher the driver would otherwise be --
torch.distributed.run with one rank per GPU on 127.0.0.1 -- instead of exiting.  The ranks themselves
need a GPU (tests/test_gpu_multiprocess.py::test_bench_self_launches_two_ranks); here the command line is checked."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_without_torchrun_builds_the_launch_command():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["RLX_BENCH_DRY_LAUNCH"] = "1"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "8", "--steps", "3", "--warmup", "1"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["launch"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-7:] == [os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1"]


def test_world_size_mismatch_is_an_error():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "4"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_zero_timed_steps_is_an_error():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "0"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("rlx_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float_arrays_of_the_bench_shape(tmp_path):
    """--dump-outputs at the bench's own shapes (host tensors stand in for the device ones): float32 / float64 only, the
    (T, N) rollout arrays whole, the (T, N, width) ones at a sorted env sample that is the same on every call, under 64 MB."""
    import numpy as np
    import torch
    bench = _bench_module()
    T, N, O, A, P, C = bench.NR_STEPS, bench.ENVS_PER_GPU, 17, 6, 176_000, 170_000
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g)
    batch = type("Batch", (), {})()
    for name in ("rewards", "terminations", "values", "next_values", "log_probs", "advantages", "returns"):
        setattr(batch, name, rnd(T, N))
    batch.states, batch.next_states, batch.actions = rnd(T, N, O), rnd(T, N, O), rnd(T, N, A)
    model = type("Model", (), {})()
    model.pparams, model.cparams, model.key, model.last_host_metrics = rnd(P), rnd(C), np.array([3, 7], np.uint32), [0.5] * 12
    state, metrics = rnd(N, O), rnd(160, 10)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, batch, state, metrics)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and all(f.endswith(".npy") for f in files)
    arrays = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    cols = arrays["sample_env_index"].astype(np.int64)
    assert len(cols) == bench.DUMP_SAMPLE_ENVS and np.all(np.diff(cols) > 0) and cols[-1] < N
    assert np.array_equal(arrays["batch_states_sample"], batch.states.numpy()[:, cols])
    assert np.array_equal(arrays["batch_advantages"], batch.advantages.numpy())
    assert np.array_equal(arrays["next_obs"], state.numpy()) and np.array_equal(arrays["update_metrics"], metrics.numpy())
    assert np.array_equal(arrays["policy_params"], model.pparams.numpy()) and list(arrays["prng_key"]) == [3.0, 7.0]
    for f in files:
        assert np.array_equal(arrays[f[:-4]], np.load(tmp_path / "b" / f))
