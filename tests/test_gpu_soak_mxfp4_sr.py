"""k_ag_group_mxfp4_sr and k_adamw_ag_mxfp4_sr through the replay soak (tests/soak.py) as tests/test_gpu_soak_mxfp4_rht.py
runs its kernels: the random words stand between a tile's loads and their wait, so this holds that the counted waits and
the one barrier per tile still stand.  RCEIL and the rotation fixed on; the state's step unchanged between replays."""
import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_ref
import mx4_cases
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_adamw_mx4 as amx4  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_shards_mxfp4 as mx4  # noqa: E402
import test_gpu_shards_mxfp4_sr as plain  # noqa: E402  (its state)
import test_gpu_soak_mxfp4_rht as rht_soak  # noqa: E402  (its row_bufs)
import test_gpu_soak_shards as shards_soak  # noqa: E402

pytestmark = pytest.mark.gpu
MASK, STEP = 0x9E3779B9, 9


def rows_of(blocks):
    """blocks[bucket]: (total, blk) float32 -> the (element row, scale row) of every bucket of the list"""
    return [t.mxfp4_sr_quantize(np.ascontiguousarray(x, dtype=np.float32).reshape(-1), plain.SEED, STEP, i, rceil=True, sign_mask=MASK)
            for i, x in enumerate(blocks)]


def build_plain(total, plan):
    buckets, _ = mx4.unequal(total)
    data = [[mx4_cases.shard(total, 256 * k, 10 * seed + i) for i, k in enumerate(sc.UNEQUAL)] for seed in sc.SEEDS]
    shards = base.Shards(buckets, "flat")
    images = [shards.expected(d) for d in data]
    bufs = rht_soak.row_bufs(buckets, [rows_of(d) for d in data])
    bufs += [soak.SoakBuf(f"shards {k}", d, [im[k] for im in images], [im[k] for im in images]) for k, d in enumerate(shards.buf)]
    args, sr = shards.args(), plain.state(STEP)
    case = soak.Case(bufs, lambda s: plan.all_gather_shards_mxfp4_sr(args, sr.data_ptr(), sign_mask=MASK, rceil=True, stream=s))
    case.keep = (buckets, shards, sr)
    return case, f"k_ag_group_mxfp4_sr<{total}, true, true>"


def build_adamw(total, plan):
    buckets = amx4.mx4_buckets(total, sc.UNEQUAL)
    data = [one.make_data(buckets, 100 * seed, sc.finite_planes) for seed in sc.SEEDS]
    planes = amx4.Planes(buckets, "flat", data[0])
    nsq = adamw_cases.norm_sq(total)
    small = amx4.SmallG(gc.hyper_array(2), nsq)
    want = [[adamw_ref.step(*x, gc.eff(sc.GROUP_OF[i]), nsq, total, True)[0] for i, x in enumerate(d)] for d in data]
    bufs = rht_soak.row_bufs(buckets, [rows_of([pl[0] for pl in w]) for w in want])
    for k in range(4):
        staged = [planes.s[k].expected([x[k] for x in d]) for d in data]
        after = [planes.s[k].expected([pl[k] for pl in w]) for w in want]
        bufs += shards_soak.shard_bufs(one.NAMES[k], planes.s[k], staged, after)
    u = adamw_ref.uniforms(gc.GROUPS[0], nsq, total)
    im = small.host.copy()
    im[small.INFO:small.INFO + 4] = np.array([u["N"], u["c"], 1.0 if u["skip"] else 0.0, 0.0], dtype=np.float32).view(np.uint32)
    bufs.append(soak.SoakBuf("hyper / norm_sq / info", small.buf, [small.host, small.host], shards_soak.finite([im, im], "info")))
    args, sr = planes.args(), plain.state(STEP)
    case = soak.Case(bufs, lambda s: plan.adamw_all_gather_shards_mxfp4_sr(args, sc.GROUP_OF, small.hyper, 2, sr.data_ptr(), MASK, small.norm_sq,
                                                                          small.info, zero_grad=True, rceil=True, stream=s))
    case.keep = (buckets, planes, small, sr)
    return case, f"k_adamw_ag_mxfp4_sr<{total}, true, true, true>"


@pytest.mark.parametrize("mode", soak.MODES)
@pytest.mark.parametrize("build", [build_plain, build_adamw], ids=["plain", "adamw"])
@pytest.mark.parametrize("total", [8, 64])
def test_mxfp4_sr_soaked(total, build, mode):
    plan = base.any_plan(t.SWING, sc.SIDE[total], total)
    try:
        case, kernel = build(total, plan)
        with t.tuned(pipe_grid=sc.GRID):
            _, trace, _ = soak.soak(case, soak.R, mode)
        assert trace.kernels == [kernel], trace.kernels
        assert trace.grids == [sc.GRID] and total * sum(sc.UNEQUAL) >= 3 * sc.GRID, trace.grids
    finally:
        plan.close()
