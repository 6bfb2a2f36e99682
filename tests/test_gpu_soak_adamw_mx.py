"""k_adamw_ag_mxfp8 through the replay soak (tests/soak.py), as tests/test_gpu_soak_shards.py soaks the older
shard-family kernels: every instantiated rank count and all four (ZERO, RCEIL) values
(tests/adamw_mx_cases.py, SOAK_CASES; tests/test_adamw_mx_table.py holds the table against the kernel file), on
the UNEQUAL (1, 3, 2, 5) list in the flat layout at pipe_grid 5 — every workgroup walks at least three tiles, so
the LDS slot rotates and the loop's waits run — with two parameter groups alternating bucket by bucket, under
`idle`, `uniform` and `uneven` load.

One capture, soak.R replays back to back, two datasets (soak_cases.finite_planes on two seeds) alternating in the
same buffers; every buffer — element rows and scale rows with skew and guard row, the four flat plane buffers
with their guard, the small hyper / norm_sq / info buffer — restored before and compared whole after every
replay, on the device.  The data is finite, so nothing is compared by class."""
import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_mx_cases as mc
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_adamw_mx as amx  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_soak_shards as shards_soak  # noqa: E402

pytestmark = pytest.mark.gpu
loads = pytest.mark.parametrize("mode", soak.MODES)


def build(c, plan):
    total, zero, rceil = c["total"], c["zero"], c["rceil"]
    buckets = amx.mx_buckets(total, c["tiles"])
    data = [one.make_data(buckets, 100 * seed, sc.finite_planes) for seed in sc.SEEDS]
    planes = amx.Planes(buckets, "flat", data[0])
    nsq = adamw_cases.norm_sq(total)
    small = amx.SmallG(gc.hyper_array(2), nsq)
    want = [mc.expect(d, mc.SOAK_GROUP_OF, nsq, total, zero, rceil) for d in data]
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
    case = soak.Case(bufs, lambda s: plan.adamw_all_gather_shards_mxfp8(args, mc.SOAK_GROUP_OF, small.hyper, 2, small.norm_sq, small.info,
                                                                       zero_grad=zero, rceil=rceil, stream=s))
    case.keep = (buckets, planes, small)
    return case


@loads
@pytest.mark.parametrize("c", mc.SOAK_CASES, ids=[mc.soak_case_id(c) for c in mc.SOAK_CASES])
def test_adamw_mxfp8_soaked(c, mode):
    total = c["total"]
    plan = base.any_plan(t.SWING, sc.SIDE[total], total)
    try:
        case = build(c, plan)
        with t.tuned(pipe_grid=c["grid"]):
            _, trace, _ = soak.soak(case, soak.R, mode)
        assert trace.kernels == [mc.soak_kernel_name(total, c["zero"], c["rceil"])] * c["launches"], trace.kernels
        assert trace.grids == [mc.SOAK_GRID] and total * sum(c["tiles"]) >= 3 * mc.SOAK_GRID, trace.grids
    finally:
        plan.close()
