"""bench.py on the GPU box: the bare `--gpus 2` launch (rehearsal: both ranks on the one GPU, collectives over gloo),
the one-rank RCCL run with forced collectives, a plain run, and --dump-outputs runs.  Short runs: the control flow, the
JSON contract and the dumped files, not the timings."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu


def _bench(env_extra, *args, timeout=420):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_bare_gpus_2_rehearsal_prints_one_line_for_two_ranks():
    out = _bench({"CAPHN_BENCH_REHEARSAL": "1"}, "--gpus", "2", "--steps", "3", "--warmup", "1", "--no-spinup", "--batch", "16")
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 32 and out["scaling"] == "weak"
    assert out["value"] > 0 and "REHEARSAL" in out["config"]["parallelism"]
    assert "cpu_baseline" not in out            # rank 0 at N = 1 only


@pytest.mark.timeout(600)
def test_single_rank_rccl_group_with_forced_collectives():
    out = _bench({"CAPHN_FORCE_COLLECTIVES": "1"}, "--gpus", "1", "--steps", "5", "--warmup", "2", "--no-spinup",
                 "--no-cpu-baseline", "--full")
    assert out["n_gpus"] == 1 and "collectives forced" in out["config"]["parallelism"]
    assert out["roofline"]["frac"] > 0.3 and out["config"]["final_loss"] < 9.5


@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_and_no_side_figures():
    out = _bench({}, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "images/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["ms_per_step"] > 0
    assert abs(out["value"] - 16 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert not {"roofline", "module_api", "cpu_baseline"} & set(out)              # side figures: --full only
    assert out["config"]["spinup_steps"] >= 40                                     # the adaptive spin-up ran (>= 2 windows)
    assert out["config"]["deterministic_gradients"] is False                       # the default, atomic-accumulating path
    assert out["collectives"]["world"] == 1


def _dump(d, *args):
    out = _bench({}, "--gpus", "1", "--batch", "16", "--dump-outputs", str(d), *args)
    assert out["config"]["spinup_steps"] == 0 and out["config"]["deterministic_gradients"] is True
    assert not {"roofline", "module_api", "cpu_baseline"} & set(out)
    arrays = {f: np.load(d / f) for f in sorted(os.listdir(d))}
    assert "loss.npy" in arrays and "captioner.fc.weight.npy" in arrays and "hn_heads.0.2.weight.sample.npy" in arrays
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["captioner.fc.weight.npy"].shape == (9684, 200)
    assert float(arrays["loss.npy"][0]) == out["config"]["final_loss"]
    return arrays


@pytest.mark.timeout(600)
def test_dump_outputs_hold_the_last_step_and_are_the_same_in_every_run(tmp_path):
    # one step from the seeded start: Adam's first update is lr * g / (|g| + eps), at most lr = 1e-3 per element and close
    # to it where the gradient is well above eps -- parameters written before the update (no move) or after a second step (up
    # to 2 lr) fail this
    import bench
    from hypernet_attention import HyperNet
    torch.manual_seed(1234)                        # bench.py's initialisation (on the host, then moved to the GPU)
    w0 = HyperNet(200, 200, 200, 9684, bench._Vocab()).captioner.fc.weight.detach().double().numpy()
    one = _dump(tmp_path / "one", "--warmup", "0", "--steps", "1")
    move = np.abs(one["captioner.fc.weight.npy"].astype(np.float64) - w0)
    assert move.max() <= 1e-3 + 1e-7 and np.median(move) > 1e-5, (move.max(), np.median(move))
    # same arguments, same files, bit for bit (no spin-up, deterministic-gradient mode)
    a = _dump(tmp_path / "a", "--warmup", "1", "--steps", "2")
    b = _dump(tmp_path / "b", "--warmup", "1", "--steps", "2")
    assert sorted(a) == sorted(b)
    for f in a:
        np.testing.assert_array_equal(b[f], a[f], err_msg=f)
    assert not np.array_equal(a["captioner.fc.weight.npy"], one["captioner.fc.weight.npy"])
