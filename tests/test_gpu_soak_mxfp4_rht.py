"""k_ag_group_mxfp4_rht and k_adamw_ag_mxfp4_rht through the replay soak (tests/soak.py), in the shape of
tests/test_gpu_soak_mxfp4.py and tests/test_gpu_soak_adamw_mx4.py: P = 8 (two storing waves) and P = 64 on the UNEQUAL
list, flat, at pipe_grid 5, under every load of soak.MODES; RCEIL fixed true (arithmetic, not waits).  The rotation
adds no memory operation, so this holds that the counted waits and the one barrier per tile still stand with the
longer arithmetic between the loads and the stores; every buffer is restored before and compared whole after every
replay."""
import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_ref
import mxfp4_rht_ref as ref
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_adamw_mx4 as amx4  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_shards_mxfp4 as mx4  # noqa: E402
import test_gpu_soak_shards as shards_soak  # noqa: E402

pytestmark = pytest.mark.gpu
MASK = 0x9E3779B9


def row_bufs(buckets, rows):
    """rows[dataset][bucket] = (element row, scale row) -> the SoakBufs of the buckets' two buffers"""
    bufs = []
    for i, b in enumerate(buckets):
        after = [b.after(*r[i]) for r in rows]
        for j, name in enumerate(("element rows", "scale rows")):
            bufs.append(soak.SoakBuf(f"bucket {i} {name}", b.buf[j], [b.host[j], b.host[j]], [a[j] for a in after]))
    return bufs


def build_plain(total, plan):
    buckets, _ = mx4.unequal(total)
    data = [[ref.cancel_shard(total, 256 * k, 10 * seed + i) for i, k in enumerate(sc.UNEQUAL)] for seed in sc.SEEDS]
    shards = base.Shards(buckets, "flat")
    images = [shards.expected(d) for d in data]
    bufs = row_bufs(buckets, [[ref.expected_rows(x, MASK, True) for x in d] for d in data])
    bufs += [soak.SoakBuf(f"shards {k}", d, [im[k] for im in images], [im[k] for im in images]) for k, d in enumerate(shards.buf)]
    args = shards.args()
    case = soak.Case(bufs, lambda s: plan.all_gather_shards_mxfp4_rht(args, MASK, rceil=True, stream=s))
    case.keep = (buckets, shards)
    return case, f"k_ag_group_mxfp4_rht<{total}, true>"


def build_adamw(total, plan):
    buckets = amx4.mx4_buckets(total, sc.UNEQUAL)
    data = [one.make_data(buckets, 100 * seed, sc.finite_planes) for seed in sc.SEEDS]
    planes = amx4.Planes(buckets, "flat", data[0])
    nsq = adamw_cases.norm_sq(total)
    small = amx4.SmallG(gc.hyper_array(2), nsq)
    want = [[adamw_ref.step(*x, gc.eff(sc.GROUP_OF[i]), nsq, total, True)[0] for i, x in enumerate(d)] for d in data]
    bufs = row_bufs(buckets, [[ref.expected_rows(pl[0], MASK, True) for pl in w] for w in want])
    for k in range(4):
        staged = [planes.s[k].expected([x[k] for x in d]) for d in data]
        after = [planes.s[k].expected([pl[k] for pl in w]) for w in want]
        bufs += shards_soak.shard_bufs(one.NAMES[k], planes.s[k], staged, after)
    u = adamw_ref.uniforms(gc.GROUPS[0], nsq, total)
    im = small.host.copy()
    im[small.INFO:small.INFO + 4] = np.array([u["N"], u["c"], 1.0 if u["skip"] else 0.0, 0.0], dtype=np.float32).view(np.uint32)
    bufs.append(soak.SoakBuf("hyper / norm_sq / info", small.buf, [small.host, small.host], shards_soak.finite([im, im], "info")))
    args = planes.args()
    case = soak.Case(bufs, lambda s: plan.adamw_all_gather_shards_mxfp4_rht(args, sc.GROUP_OF, small.hyper, 2, MASK, small.norm_sq,
                                                                           small.info, zero_grad=True, rceil=True, stream=s))
    case.keep = (buckets, planes, small)
    return case, f"k_adamw_ag_mxfp4_rht<{total}, true, true>"


@pytest.mark.parametrize("mode", soak.MODES)
@pytest.mark.parametrize("build", [build_plain, build_adamw], ids=["plain", "adamw"])
@pytest.mark.parametrize("total", [8, 64])
def test_mxfp4_rht_soaked(total, build, mode):
    plan = base.any_plan(t.SWING, sc.SIDE[total], total)
    try:
        case, kernel = build(total, plan)
        with t.tuned(pipe_grid=sc.GRID):
            _, trace, _ = soak.soak(case, soak.R, mode)
        assert trace.kernels == [kernel], trace.kernels
        assert trace.grids == [sc.GRID] and total * sum(sc.UNEQUAL) >= 3 * sc.GRID, trace.grids
    finally:
        plan.close()
