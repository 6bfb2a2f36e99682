"""k_adamw_ag_mxfp4 through the replay soak (tests/soak.py), in the shape of tests/test_gpu_soak_adamw_mx.py: every
instantiated rank count and both ZERO values — RCEIL fixed true: it changes arithmetic, not the waits — on the
UNEQUAL (1, 3, 2, 5) list in the flat layout at pipe_grid 5, two parameter groups alternating, under every load of
soak.MODES.  This is what holds the one barrier per tile (at P = 8 with two waves that store nothing), the slot
rotation and the counted waits under load; every buffer is restored before and compared whole after every replay."""
import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_mx4_cases as m4
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_adamw_mx4 as amx4  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_soak_shards as shards_soak  # noqa: E402

pytestmark = pytest.mark.gpu


def build(total, zero, plan):
    buckets = amx4.mx4_buckets(total, sc.UNEQUAL)
    data = [one.make_data(buckets, 100 * seed, sc.finite_planes) for seed in sc.SEEDS]
    planes = amx4.Planes(buckets, "flat", data[0])
    nsq = adamw_cases.norm_sq(total)
    small = amx4.SmallG(gc.hyper_array(2), nsq)
    want = [m4.expect(d, sc.GROUP_OF, nsq, total, zero, True) for d in data]
    bufs = []
    for i, b in enumerate(buckets):
        after = [b.after(*w[1][i]) for w in want]
        for j, name in enumerate(("element rows", "scale rows")):
            bufs.append(soak.SoakBuf(f"bucket {i} {name}", b.buf[j], [b.host[j], b.host[j]], [a[j] for a in after]))
    for k in range(4):
        staged = [planes.s[k].expected([x[k] for x in d]) for d in data]
        after = [planes.s[k].expected([v[k] for v in w[0]]) for w in want]
        bufs += shards_soak.shard_bufs(one.NAMES[k], planes.s[k], staged, after)
    info = []
    for w in want:
        im = small.host.copy()
        im[small.INFO:small.INFO + 4] = np.asarray(w[2], dtype=np.float32).view(np.uint32)
        info.append(im)
    bufs.append(soak.SoakBuf("hyper / norm_sq / info", small.buf, [small.host, small.host], shards_soak.finite(info, "info")))
    args = planes.args()
    case = soak.Case(bufs, lambda s: plan.adamw_all_gather_shards_mxfp4(args, sc.GROUP_OF, small.hyper, 2, small.norm_sq, small.info,
                                                                       zero_grad=zero, rceil=True, stream=s))
    case.keep = (buckets, planes, small)
    return case


@pytest.mark.parametrize("mode", soak.MODES)
@pytest.mark.parametrize("zero", [False, True], ids=["zero0", "zero1"])
@pytest.mark.parametrize("total", sc.RANKS)
def test_adamw_mxfp4_soaked(total, zero, mode):
    plan = base.any_plan(t.SWING, sc.SIDE[total], total)
    try:
        case = build(total, zero, plan)
        with t.tuned(pipe_grid=sc.GRID):
            _, trace, _ = soak.soak(case, soak.R, mode)
        assert trace.kernels == [amx4.kernel(total, zero, True)], trace.kernels
        assert trace.grids == [sc.GRID] and total * sum(sc.UNEQUAL) >= 3 * sc.GRID, trace.grids
    finally:
        plan.close()
