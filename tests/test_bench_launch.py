"""bench.py launch contract: ``--gpus N`` outside a launcher re-launches N ranks under
torch.distributed.run (before any device call) and rank 0 prints ONE JSON line with
``n_gpus == N`` and the whole-job throughput; inside a launcher ``WORLD_SIZE`` must equal
``--gpus``.  Runs on the CPU (gloo, fp32, tiny batch / image) — the reference harness is
``DL/models/utils/DistriOptimizerPerf.scala:32-146``."""
import json
import os
import subprocess
import sys

import pytest

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.join(_REPO, "bench.py"), "--device", "cpu", "--batch", "2", "--image-size", "64",
           "--steps", "2", "--warmup", "1", "--phase-steps", "1"] + extra
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=_REPO)


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("n", [1, 2])
def test_bench_gpus_flag_spawns_ranks(n):
    r = _run(["--gpus", str(n), "--full"])  # the per-phase timers are a --full measurement
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout  # rank 0 only
    j = lines[0]
    assert j["n_gpus"] == n
    assert j["config"]["global_batch"] == 2 * n
    assert j["config"]["parallelism"] == f"dp{n}"
    assert j["config"]["driver"] == ("DistriOptimizer" if n > 1 else "LocalOptimizer")
    assert j["steps"] == 2 and j["warmup"] == 1
    assert j["value"] > 0 and j["ms_per_step"] > 0
    # value is the whole-job aggregate: global batch × steps / elapsed
    assert abs(j["value"] - 2 * n * 1e3 / j["ms_per_step"]) / j["value"] < 0.02
    ph = j["phase_ms_max_over_ranks"]
    assert "forward" in ph and "backward" in ph and "compute weight" in ph
    if n > 1:
        assert "aggregate gradient" in ph


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """Without ``--full`` only the headline is measured (no phase timers, no fp32 record), and
    ``--dump-outputs`` writes the last timed step's loss as float32."""
    import numpy as np
    d = tmp_path / "out"
    r = _run(["--gpus", "1", "--dump-outputs", str(d)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    (j,) = _json_lines(r.stdout)
    assert j["steps"] == 2 and j["value"] > 0 and j["ms_per_step"] > 0
    assert j["phase_ms_max_over_ranks"] == {} and j["fp32"] is None
    assert [f.name for f in d.iterdir()] == ["loss.npy"]
    loss = np.load(d / "loss.npy")
    assert loss.dtype == np.float32 and loss.shape == (1,) and np.isfinite(loss).all()
    assert abs(float(loss[0]) - j["final_loss"]) < 1e-6 * max(1.0, abs(j["final_loss"]))
    # the dumped step starts from the seeded initial state whatever ran before it: two more timed
    # steps in front (same batch parity) leave the file unchanged up to fp32 summation order
    d4 = tmp_path / "out4"
    r = _run(["--gpus", "1", "--steps", "4", "--dump-outputs", str(d4)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert _json_lines(r.stdout)[0]["steps"] == 4
    np.testing.assert_allclose(np.load(d4 / "loss.npy"), loss, rtol=1e-5, atol=0)


def test_bench_world_size_mismatch_rejected():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1 but --gpus 2" in (r.stdout + r.stderr)
