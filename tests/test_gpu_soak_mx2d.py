"""k_ag_group_mxfp8_2d through the replay soak (tests/soak.py), as tests/test_gpu_soak_adamw_mx.py soaks
k_adamw_ag_mxfp8: every instantiated rank count and all four (RCEIL, ROWS) values (tests/mx2d_cases.py,
SOAK_CASES; tests/test_mx2d_table.py holds the table against the kernel file), on an unequal list of six
matrices, two of them of several row groups per shard block, in the flat layout at pipe_grid 5 — every
workgroup walks at least three work units, so the LDS image rotates — under `idle`, `uniform` and `uneven` load.

One capture, soak.R replays back to back, two datasets (soak_cases.finite_floats on two seeds) alternating in
the same buffers; every buffer — each bucket's four row sets with skew and guard row, the flat shard buffer with its
guard — restored before and compared whole after every replay, on the device."""
import numpy as np
import pytest

import mx2d_cases as mc
import mx2d_ref
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_shards_mxfp8_2d as m2  # noqa: E402
import test_gpu_soak_shards as shards_soak  # noqa: E402

pytestmark = pytest.mark.gpu
loads = pytest.mark.parametrize("mode", soak.MODES)


def build(c, plan):
    total, rceil, rows = c["total"], c["rceil"], c["rows"]
    buckets = [m2.Bucket2d(total, cols, R, skew=i % 2 == 1, rows=rows) for i, (cols, R) in enumerate(c["shapes"])]
    data = [[sc.finite_floats(100 * seed + i, (total * b.R, b.cols)) for i, b in enumerate(buckets)] for seed in sc.SEEDS]
    shards = m2.Shards(buckets, "flat")
    staged = [shards.expected([mx2d_ref.blocks(W, total) for W in d]) for d in data]
    bufs = []
    for i, b in enumerate(buckets):
        want = [mx2d_ref.expected_rows(d[i], total, rceil) + mx2d_ref.expected_t(d[i], rceil) for d in data]
        sets = ([("element rows", b.r, 0), ("scale rows", b.r, 1)] if rows else []) + [("t element rows", b.c, 2), ("t scale rows", b.c, 3)]
        for name, part, k in sets:
            after = [part.after(w[k - k % 2], w[k - k % 2 + 1])[k % 2] for w in want]
            bufs.append(soak.SoakBuf(f"bucket {i} {name}", part.buf[k % 2], [part.host[k % 2]] * 2, after))
    bufs += shards_soak.shard_bufs("shard", shards, staged, staged)
    args = shards.args()
    case = soak.Case(bufs, lambda s: plan.all_gather_shards_mxfp8_2d(args, rceil=rceil, stream=s))
    case.keep = (buckets, shards)
    return case


@loads
@pytest.mark.parametrize("c", mc.SOAK_CASES, ids=[mc.soak_case_id(c) for c in mc.SOAK_CASES])
def test_mxfp8_2d_soaked(c, mode):
    total = c["total"]
    plan = base.any_plan(t.SWING, sc.SIDE[total], total)
    try:
        case = build(c, plan)
        with t.tuned(pipe_grid=c["grid"]):
            _, trace, _ = soak.soak(case, soak.R, mode)
        assert trace.kernels == [mc.soak_kernel_name(total, c["rceil"], c["rows"])] * c["launches"], trace.kernels
        assert trace.grids == [mc.SOAK_GRID], trace.grids
    finally:
        plan.close()
