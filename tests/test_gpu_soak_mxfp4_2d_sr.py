"""k_ag_group_mxfp4_2d_sr through the replay soak (tests/soak.py) as tests/test_gpu_soak_mxfp4_2d.py soaks
k_ag_group_mxfp4_2d: the random words stand between a square's F store and its barrier, so this holds that the
rotation of F and of the two image sets still stands.  P = 8 and 64, rows given, RCEIL and the rotation fixed on; the
state's step unchanged between replays."""
import numpy as np
import pytest

import mx4_2d_ref as r2
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_shards_mxfp4_2d as m4  # noqa: E402
import test_gpu_shards_mxfp4_2d_sr as sr2  # noqa: E402
import test_gpu_soak_shards as shards_soak  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = ((32, 32), (96, 64), (128, 32))   # (cols, R) per bucket: strips of 4, 4 and 16 squares
STEP = 9


def build(total, plan):
    buckets = [m4.Bucket2d(total, cols, R, skew=i % 2 == 1) for i, (cols, R) in enumerate(SHAPES)]
    data = [[sc.finite_floats(100 * seed + i, (total * b.R, b.cols)) for i, b in enumerate(buckets)] for seed in sc.SEEDS]
    shards = m4.Shards(buckets, "flat")
    staged = [shards.expected([W.reshape(total, -1) for W in d]) for d in data]
    bufs = []
    for i, b in enumerate(buckets):
        want = [r2.expected(d[i], total, True)[:2] + t.mxfp4_sr_quantize(np.ascontiguousarray(d[i].T).reshape(-1), sr2.sr1.SEED, STEP, i,
                                                                         rceil=True, sign_mask=sr2.MASK) for d in data]
        for name, part, k in (("rows", b.r, 0), ("t rows", b.c, 2)):
            after = [part.after(w[k], w[k + 1]) for w in want]
            for j, kind in enumerate(("element", "scale")):
                bufs.append(soak.SoakBuf(f"bucket {i} {kind} {name}", part.buf[j], [part.host[j]] * 2, [a[j] for a in after]))
    bufs += shards_soak.shard_bufs("shard", shards, staged, staged)
    args, sr = shards.args(), sr2.state(STEP)
    case = soak.Case(bufs, lambda s: plan.all_gather_shards_mxfp4_2d_sr(args, sr.data_ptr(), sign_mask=sr2.MASK, rceil=True, stream=s))
    case.keep = (buckets, shards, sr)
    return case


@pytest.mark.parametrize("mode", soak.MODES)
@pytest.mark.parametrize("total", [8, 64])
def test_mxfp4_2d_sr_soaked(total, mode):
    plan = m4.plan_for(total)
    try:
        case = build(total, plan)
        with t.tuned(pipe_grid=sc.GRID):
            _, trace, _ = soak.soak(case, soak.R, mode)
        assert trace.kernels == [sr2.kernel(total, True, True, sr2.MASK)] and trace.grids == [sc.GRID], (trace.kernels, trace.grids)
    finally:
        plan.close()
