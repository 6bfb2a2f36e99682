"""k_adamw_ag_mxfp4_2d through the replay soak (tests/soak.py): every rank count of for_ranks<8, 64> with both ZERO values, ROWS
on, RCEIL alternating, on test_gpu_soak_adamw_mx2d's four matrices — 28 strips-by-column-groups at 8 ranks, so at pipe_grid 5
every workgroup takes at least five units across shard-block, strip and bucket ends — in the flat layout, two parameter groups,
under the three loads.  The planes are rewritten IN PLACE, so the restore before and the whole-buffer compare after each of soak.R
replays, on two alternating datasets, is the check that matters: a plane store racing a later load, an element updated twice or
a prefetched square that saw a p' differs."""
import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_adamw_mx2d as a2  # noqa: E402
import test_gpu_adamw_mx4_2d as a4  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_mxfp4_2d as m4  # noqa: E402
import test_gpu_soak_adamw_mx2d as s2  # noqa: E402
import test_gpu_soak_shards as shards_soak  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [{"total": p, "zero": zero, "rceil": (i + zero) % 2 == 1} for i, p in enumerate(sc.RANKS) for zero in (False, True)]


def build(c, plan):
    total, zero, rceil = c["total"], c["zero"], c["rceil"]
    lst = tuple((cols, R, "planes", g) for (cols, R), g in zip(s2.SHAPES, sc.GROUP_OF))
    buckets = a4.buckets_of(total, lst)
    data = [a2.make_data(total, lst, 100 * seed, sc.finite_planes) for seed in sc.SEEDS]
    planes = a4.Planes(buckets, "flat", data[0])
    nsq = adamw_cases.norm_sq(total)
    small = a4.SmallG(gc.hyper_array(2), nsq)
    want = [a4.expect(d, lst, total, nsq, zero, rceil) for d in data]
    bufs = []
    for i, b in enumerate(buckets):
        for part, k in ((b.r, 0), (b.c, 2)):   # outputs k, k + 1: an element buffer and a scale buffer
            after = [part.after(w[1][i][k], w[1][i][k + 1]) for w in want]
            bufs += [soak.SoakBuf(f"bucket {i} output {k + j}", part.buf[j], [part.host[j]] * 2, [a[j] for a in after]) for j in (0, 1)]
    for k in range(4):
        bufs += shards_soak.shard_bufs(one.NAMES[k], planes.s[k], [planes.s[k].expected([x[k] for x in d]) for d in data],
                                       [planes.s[k].expected([v[k] for v in w[0]]) for w in want])
    info = [small.host.copy() for _ in want]
    for im, w in zip(info, want):
        im[small.INFO:small.INFO + 4] = np.asarray(w[2], dtype=np.float32).view(np.uint32)
    bufs.append(soak.SoakBuf("hyper / norm_sq / info", small.buf, [small.host, small.host], shards_soak.finite(info, "info")))
    args = planes.args()
    case = soak.Case(bufs, lambda s: plan.adamw_all_gather_shards_mxfp4_2d(args, sc.GROUP_OF, small.hyper, 2, small.norm_sq, small.info,
                                                                          zero_grad=zero, rceil=rceil, stream=s))
    case.keep = (buckets, planes, small)
    return case


@pytest.mark.parametrize("mode", soak.MODES)
@pytest.mark.parametrize("c", CASES, ids=[f"adamw-mx4-2d-{c['total']}-zero{int(c['zero'])}" for c in CASES])
def test_adamw_mxfp4_2d_soaked(c, mode):
    total = c["total"]
    plan = m4.plan_for(total)
    try:
        with t.tuned(pipe_grid=sc.GRID):
            _, trace, _ = soak.soak(build(c, plan), soak.R, mode)
        assert trace.kernels == [a4.kernel(total, c["zero"], c["rceil"])] and trace.grids == [sc.GRID], trace.kernels
    finally:
        plan.close()
