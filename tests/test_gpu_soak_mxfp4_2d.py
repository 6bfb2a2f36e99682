"""k_ag_group_mxfp4_2d through the replay soak (tests/soak.py), as tests/test_gpu_soak_mx2d.py soaks
k_ag_group_mxfp8_2d: every instantiated rank count with ROWS true and false (RCEIL alternating), on one unequal
list of four matrices — strips inside one shard block, across two and four, and astride a block end — in the flat
layout at pipe_grid 5, under the three loads.  What it is there for: the rotation of the two LDS image sets across
strips of 4, 8 and 16 squares, and the strip's last barrier in front of the streaming stores.

One capture, soak.R replays back to back, two datasets alternating in the same buffers; every buffer — each
bucket's four row sets with skew and guard row, the flat shard buffer with its guard — compared whole."""
import pytest

import mx4_2d_ref as r2
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_shards_mxfp4_2d as m4  # noqa: E402
import test_gpu_soak_shards as shards_soak  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = ((32, 32), (96, 64), (64, 96), (128, 32))   # (cols, R) per bucket


def build(total, rceil, rows, plan):
    buckets = [m4.Bucket2d(total, cols, R, skew=i % 2 == 1, rows=rows) for i, (cols, R) in enumerate(SHAPES)]
    data = [[sc.finite_floats(100 * seed + i, (total * b.R, b.cols)) for i, b in enumerate(buckets)] for seed in sc.SEEDS]
    shards = m4.Shards(buckets, "flat")
    staged = [shards.expected([W.reshape(total, -1) for W in d]) for d in data]
    bufs = []
    for i, b in enumerate(buckets):
        want = [r2.expected(d[i], total, rceil) for d in data]
        for name, part, k in ([("rows", b.r, 0)] if rows else []) + [("t rows", b.c, 2)]:
            after = [part.after(w[k], w[k + 1]) for w in want]
            for j, kind in enumerate(("element", "scale")):
                bufs.append(soak.SoakBuf(f"bucket {i} {kind} {name}", part.buf[j], [part.host[j]] * 2, [a[j] for a in after]))
    bufs += shards_soak.shard_bufs("shard", shards, staged, staged)
    args = shards.args()
    case = soak.Case(bufs, lambda s: plan.all_gather_shards_mxfp4_2d(args, rceil=rceil, stream=s))
    case.keep = (buckets, shards)
    return case


@pytest.mark.parametrize("mode", soak.MODES)
@pytest.mark.parametrize("rows", [False, True], ids=["t-only", "rows"])
@pytest.mark.parametrize("total", sc.RANKS)
def test_mxfp4_2d_soaked(total, rows, mode):
    rceil = (total in (16, 64)) != rows
    plan = m4.plan_for(total)
    try:
        case = build(total, rceil, rows, plan)
        with t.tuned(pipe_grid=sc.GRID):
            _, trace, _ = soak.soak(case, soak.R, mode)
        assert trace.kernels == [m4.kernel(total, rceil, rows)] and trace.grids == [sc.GRID], (trace.kernels, trace.grids)
    finally:
        plan.close()
