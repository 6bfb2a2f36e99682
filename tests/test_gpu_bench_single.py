"""The N = 1 bench as the driver runs it: a plain `bench.py --gpus 1 --steps K --warmup W`
prints one JSON line with the headline alone (no secondary measurement: those are --full's),
and --dump-outputs DIR writes what the last timed step computed — checked here bit for bit
against the CPU oracle's allreduce of the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

torch = pytest.importorskip("torch")
import bench  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

# --full's fields of the N = 1 line: a plain run measures none of them
FULL_ONLY = {"schedule_faithful", "cache_resident", "hierarchical_step_w1", "host_staged", "config1", "tilesum",
             "cpu_baseline"}


@pytest.fixture(scope="module")
def oracle_rows():
    """what the last timed step leaves in its bucket set, by the CPU oracle (same schedule, same
    per-add bf16 rounding), as float32 (64, 327680): the seeded set allreduced in place twice,
    by the last step of the untimed lead-in and by the last timed step"""
    buf = torch.empty((bench.RANKS, bench.ELEMS), dtype=torch.int16, device="cuda:0")
    bench.fill_reference_convention(buf, bench.LAST_SET_SEED)
    want = [r.copy() for r in buf.cpu().numpy().view(np.uint16)]
    for _ in range(2):
        oracle.allreduce("bo", oracle.SWING, bench.SIDE, want, bench.RANKS)
    want = torch.from_numpy(np.stack(want).view(np.int16)).view(torch.bfloat16).float().numpy()
    assert np.isfinite(want).all() and want.max() > 6400.0   # 64 x 64 values in [0, 100)
    return want


# 8: eager launches behind a spin kernel; 100: one replay of a captured HIP graph;
# GRAPH_MAX_STEPS + 1: replays of the chunk graph, then the graph with the rest
@pytest.mark.parametrize("steps", [8, 100, bench.GRAPH_MAX_STEPS + 1])
def test_plain_run_prints_the_headline_and_dumps_the_last_steps_outputs(tmp_path, oracle_rows, steps):
    out_dir = tmp_path / "outputs"
    # 4 rotating sets, no prewarm: the shortest run of the whole plain path
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--sets", "4", "--prewarm-ms", "0", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "GB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == 2
    assert d["timing"]["timed_steps"] == steps and d["full"] is False
    assert d["config"]["hip_graph"] is (steps >= 100)
    assert d["ms_per_step"] == pytest.approx(d["timing"]["ms_timed"] / steps, rel=1e-3)
    bytes_all = bench.RANKS * bench.ELEMS * 2
    assert d["value"] == pytest.approx(bytes_all / (d["ms_per_step"] * 1e-3) / 1e9, rel=1e-3)
    assert not FULL_ONLY & set(d)

    files = sorted(os.listdir(out_dir))
    assert files == ["allreduce_rank0.npy", "allreduce_ranks_sample.npy", "allreduce_sample_columns.npy"]
    arrays = {f: np.load(out_dir / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
    cols = arrays["allreduce_sample_columns.npy"].astype(np.int64)
    assert (cols == bench.dump_sample_columns()).all() and cols.shape == (bench.DUMP_SAMPLE_COLUMNS,)

    assert np.array_equal(arrays["allreduce_rank0.npy"], oracle_rows[0])
    assert np.array_equal(arrays["allreduce_ranks_sample.npy"], oracle_rows[:, cols])
