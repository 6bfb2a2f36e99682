"""allred_plan_adamw_all_gather_shards_mxfp4_sr (k_adamw_ag_mxfp4_sr) held to allred.h's guarantee, BIT FOR BIT and on
WHOLE buffers: the planes and info are those the UNROTATED RNE call adamw_all_gather_shards_mxfp4 leaves, the element
rows and scale rows those all_gather_shards_mxfp4_sr writes from the resulting param plane (p' — partly NaN here —, or
p on a skipped step) under the same state, and at P = 8 those of t.mxfp4_sr_quantize."""
import numpy as np
import pytest

import adamw_groups_cases as gc
import adamw_mx4_cases as m4
import f32_tree
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import test_gpu_adamw_groups as groups  # noqa: E402
import test_gpu_adamw_mx as amx  # noqa: E402
import test_gpu_adamw_mx4 as amx4  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_shards_mxfp4_sr as plain  # noqa: E402  (its state)

pytestmark = pytest.mark.gpu
tf, stream = amx.tf, base.stream
LIST = ((1, "identity", 1), (3, "negative_v", 0), (2, "identity", 1), (2, "zero_den", 2), (3, "planes", 0))
MASKS = {8: None, 16: 0x9E3779B9, 32: None, 64: 0xFFFFFFFF}   # None: no rotation
STEP = 5


def kernel(total, zero, rceil, mask):
    return f"k_adamw_ag_mxfp4_sr<{total}, {tf(zero)}, {tf(rceil)}, {tf(mask is not None)}>"


@pytest.mark.parametrize("case", ["clip", "N-inf"])   # N-inf: the skipped step, the rows are p's
@pytest.mark.parametrize("total", sc.RANKS)
@amx.flag_pairs
def test_planes_of_the_mxfp4_step_rows_of_the_sr_all_gather(total, zero, rceil, case):
    mask = MASKS[total]
    tiles, group_of = tuple(k for k, _, _ in LIST), tuple(g for _, _, g in LIST)
    data = m4.make(total, 300 + total, LIST)
    buckets, second = amx4.mx4_buckets(total, tiles), amx4.mx4_buckets(total, tiles)
    planes = amx4.Planes(buckets, "flat", data)
    hyper0, nsq = one.uniform_cases(total)[case]
    grps = (hyper0, gc.GROUPS[1], gc.GROUPS[2])
    small, small2 = amx4.SmallG(gc.hyper_array(3, grps), nsq), amx4.SmallG(gc.hyper_array(3, grps), nsq)
    args, sr = planes.args(), plain.state(STEP)
    plan = base.any_plan(t.SWING, sc.SIDE[total], total)
    with t.tuned(pipe_grid=sc.GRID):   # every workgroup walks at least three tiles: the slot rotates
        with t.launch_trace() as tr:
            plan.adamw_all_gather_shards_mxfp4_sr(args, group_of, small.hyper, 3, sr.data_ptr(), mask, small.norm_sq, small.info,
                                                  zero_grad=zero, rceil=rceil, stream=stream())
        assert tr.kernels == [kernel(total, zero, rceil, mask)]
        new = [g.copy() for s in planes.s for g in s.got()]
        new_rows = [b.got() for b in buckets]
        new_info = groups.info_words(small)
        planes.restore()
        twin_args = [b.arg + a[5:] for b, a in zip(second, args)]
        plan.adamw_all_gather_shards_mxfp4(twin_args, group_of, small2.hyper, 3, small2.norm_sq, small2.info, zero_grad=zero, rceil=rceil,
                                           stream=stream())
        old = [g.copy() for s in planes.s for g in s.got()]
        param = [s.copy() for s in planes.s[0].got()]   # the param plane the step leaves: the plain call's shard
        for b in second:
            b.restore()
        plan.all_gather_shards_mxfp4_sr([b.arg + (a[5], a[9]) for b, a in zip(second, args)], sr.data_ptr(), sign_mask=mask, rceil=rceil,
                                        stream=stream())
    assert len(new) == len(old)
    for k, (a, b) in enumerate(zip(new, old)):
        assert f32_tree.same_f32(a.view(np.float32), b.view(np.float32)), f"plane buffer {k}"
    for i, (a, b) in enumerate(zip(new_rows, [b.got() for b in second])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"bucket {i}: rows and scales"
    assert np.array_equal(new_info, groups.info_words(small2))
    skipped = case == "N-inf"
    assert new_info.view(np.float32)[2] == (1.0 if skipped else 0.0)
    assert any((r[1][:total, :b.n // 32] == 0xFF).any() for r, b in zip(new_rows, buckets))
    if total == 8:   # numpy: bucket 1 of the list from the param plane the twin left — p itself on a skipped step
        i, n = 1, buckets[1].n
        src = planes.s[0].blocks(i, param)
        assert np.array_equal(src.view(np.uint32), np.ascontiguousarray(data[i][0]).view(np.uint32)) == skipped
        we, ws = t.mxfp4_sr_quantize(src.reshape(-1), plain.SEED, STEP, i, rceil=rceil, sign_mask=mask)
        assert np.array_equal(new_rows[i][0][0, :n // 2], we) and np.array_equal(new_rows[i][1][0, :n // 32], ws)
    plan.close()
