"""k_ag_group_mxfp4 through the replay soak (tests/soak.py), as tests/test_gpu_soak_shards.py soaks k_ag_group_mxfp8:
every rank count and both flags on the UNEQUAL list, flat, at pipe_grid 5 (every workgroup walks at least three
tiles with loads in flight), under the three loads; two datasets alternate, every buffer is compared whole."""
import pytest

import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_shards_mxfp4 as mx4  # noqa: E402

pytestmark = pytest.mark.gpu


def build(total, rceil, plan):
    buckets, _ = mx4.unequal(total)
    keys = [[(total, 256 * k, 10 * seed + i) for i, k in enumerate(sc.UNEQUAL)] for seed in sc.SEEDS]   # mx4.cases' keys
    shards = base.Shards(buckets, "flat")
    images = [shards.expected([mx4.cases(*key) for key in ks]) for ks in keys]
    bufs = []
    for i, b in enumerate(buckets):
        after = [b.after(*mx4.expected(*ks[i], rceil)) for ks in keys]
        for j, name in enumerate(("element rows", "scale rows")):
            bufs.append(soak.SoakBuf(f"bucket {i} {name}", b.buf[j], [b.host[j], b.host[j]], [a[j] for a in after]))
    bufs += [soak.SoakBuf(f"shards {k}", d, [im[k] for im in images], [im[k] for im in images]) for k, d in enumerate(shards.buf)]
    args = shards.args()
    case = soak.Case(bufs, lambda s: plan.all_gather_shards_mxfp4(args, rceil=rceil, stream=s))
    case.keep = (buckets, shards)
    return case


@pytest.mark.parametrize("mode", soak.MODES)
@pytest.mark.parametrize("rceil", [False, True])
@pytest.mark.parametrize("total", sc.RANKS)
def test_mxfp4_soaked(total, rceil, mode):
    plan = base.any_plan(t.SWING, sc.SIDE[total], total)
    try:
        case = build(total, rceil, plan)
        with t.tuned(pipe_grid=sc.GRID):
            _, trace, _ = soak.soak(case, soak.R, mode)
        assert trace.kernels == [mx4.kernel(total, rceil)], trace.kernels
        assert trace.grids == [sc.GRID] and total * sum(sc.UNEQUAL) >= 3 * sc.GRID, trace.grids
    finally:
        plan.close()
