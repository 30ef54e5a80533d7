"""bench.py --gpus N brings up N ranks itself (VERDICT r4 Missing #1 / Next #1).

`python3 bench.py --gpus 2` — the driver's BENCH command form, no torchrun — must start two ranks (one
process per GPU) before any GPU call, for every mode; under a launcher whose WORLD_SIZE differs from --gpus
it must exit non-zero.  --launch-check runs the same bring-up (launcher, process group, rank -> shard of the
global batch) over gloo without touching a GPU, so this runs on the CPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None, timeout=180):
    env = dict(os.environ, NPS_BENCH_REHEARSAL="1", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def _line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("mode_args,gb", [([], 16), (["--mode", "train"], 16), (["--model", "ufno3d"], 8)])
def test_gpus_2_starts_two_ranks(mode_args, gb):
    r = _bench(["--gpus", "2", "--launch-check", *mode_args])
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["dist"]["world_size"] == 2 and line["n_gpus"] == 2
    assert line["dist"]["backend"] == "gloo"
    assert line["shards"] == [[0, gb // 2], [gb // 2, gb]]


def test_gpus_1_is_one_process():
    r = _bench(["--launch-check"])
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["dist"]["world_size"] == 1 and line["shards"] == [[0, 16]]


def test_world_size_mismatch_exits_nonzero():
    r = _bench(["--gpus", "2", "--launch-check"], env_extra=dict(WORLD_SIZE="4", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0
    assert "WORLD_SIZE=4" in r.stderr


def test_indivisible_batch_exits_nonzero():
    r = _bench(["--gpus", "3", "--launch-check"])
    assert r.returncode != 0


def test_full_and_dump_outputs_are_options():
    r = _bench(["--launch-check", "--full", "--dump-outputs", "unused"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert _line(r.stdout)["dist"]["world_size"] == 1


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path):
    """--dump-outputs: small arrays whole (shape kept; float64 stays, bf16 / complex become float32), an array
    above DUMP_MAX_ELEMS as the same seeded sample of its elements on every call, rank-suffixed names at N > 1."""
    import numpy as np
    import torch
    import bench
    n = bench.DUMP_MAX_ELEMS + 12345
    big = torch.arange(n, dtype=torch.float32)
    arrays = {"small": torch.arange(6, dtype=torch.float64).reshape(2, 3), "half": torch.ones(4, dtype=torch.bfloat16),
              "cplx": torch.tensor([1 + 2j, 3 - 4j], dtype=torch.complex64), "big": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), {"big": big * 2}, rank=1, world=2)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    assert got["small"].dtype == np.float64 and got["small"].shape == (2, 3)
    assert got["half"].dtype == np.float32 and got["cplx"].dtype == np.float32
    assert got["cplx"].tolist() == [[1.0, 2.0], [3.0, -4.0]]
    assert got["big"].dtype == np.float32 and got["big"].shape == (bench.DUMP_MAX_ELEMS,)
    assert sum(a.nbytes for a in got.values()) <= 64 * 10 ** 6
    # values of `big` are their own indices: the sample is in range, not constant, and the same on every call
    assert got["big"].min() >= 0 and got["big"].max() < n and len(np.unique(got["big"][:1000])) > 900
    other = np.load(tmp_path / "b" / "big_rank1.npy")
    assert np.array_equal(other, 2 * got["big"])
