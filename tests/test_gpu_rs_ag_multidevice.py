"""allred_dist_reduce_scatter / allred_dist_all_gather over RCCL across 2, 4 and 8
REAL devices, one fresh child process per GPU (tests/gpu_rs_ag_child.py), bit-exact
against the oracle — the expectations of tests/test_rs_ag_host.py, which runs the
same half programs through the host twins on CPU.  Each case needs that many visible
GPUs and skips with that reason otherwise (RCCL refuses two ranks on one device)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NG = torch.cuda.device_count()   # counts devices without initialising HIP
GRIDS = {2: (2, 2), 4: (2, 4), 8: (4, 8)}
ALGOS = (0, 1, 2, 3)   # RecDub, Swing, 1D RecDub, 1D Swing
CHILD_TIMEOUT_S = 180


def elems(world):
    return 8 * GRIDS[world][1] * 3


def rank_inputs(world, algo, check):
    """(bf16 data for the reduce-scatter, arbitrary 16-bit patterns for the all-gather), one row per rank"""
    n = elems(world)
    rng = np.random.default_rng(1000 * world + 10 * algo + check)
    return (rng.integers(0x3F80, 0x42C8, (world, n)).astype(np.uint16),
            rng.integers(0, 0x10000, (world, n)).astype(np.uint16))


@pytest.mark.parametrize("world", [2, 4, 8])
def test_rccl_reduce_scatter_all_gather_across_gpus(world, tmp_path):
    if NG < world:
        pytest.skip(f"needs {world} GPUs, {NG} visible (RCCL: one rank per device)")
    uid = t.Comm.unique_id().hex()
    env = dict(os.environ)
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "gpu_rs_ag_child.py"), str(r), str(world), uid,
                               outs[r]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for r in range(world)]
    results = []
    try:
        for p in procs:   # each child has its own bound
            results.append(p.communicate(timeout=CHILD_TIMEOUT_S))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, (so, se)) in enumerate(zip(procs, results)):
        assert p.returncode == 0, (r, so, se[-3000:])
    side2d, total = GRIDS[world]
    n = elems(world)
    blk = n // total
    got = [np.load(o) for o in outs]
    for check in (0, 1):
        for algo in ALGOS:
            data, raw = rank_inputs(world, algo, check)
            want = [d.copy() for d in data]
            oracle.allreduce("bo", algo, 1 if algo >= 2 else side2d, want, total)
            for r in range(world):
                own = slice(r * blk, (r + 1) * blk)
                assert np.array_equal(got[r][f"rs_{check}_{algo}"][own], want[r][own]), ("rs", check, algo, r)
                assert np.array_equal(got[r][f"rsag_{check}_{algo}"], want[r]), ("rs+ag", check, algo, r)
                gathered = np.concatenate([raw[b][b * blk:(b + 1) * blk] for b in range(total)])
                assert np.array_equal(got[r][f"ag_{check}_{algo}"], gathered), ("ag", check, algo, r)
