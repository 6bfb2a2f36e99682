"""allred_plan_adamw_all_gather_shards_mxfp4_rht (k_adamw_ag_mxfp4_rht) held to allred.h's guarantee, BIT FOR BIT and
on WHOLE buffers: the planes and info are those adamw_all_gather_shards_mxfp4 leaves, the element rows and scale rows
those all_gather_shards_mxfp4_rht writes from the resulting param plane (p' — partly NaN here —, or p on a skipped
step).  One identity bucket carries mx4_cases' planted blocks, one mxfp4_rht_ref.cancel_shard: on the latter a wrong
stage order, operand order or sign bit in the eight-lane butterfly changes nibbles."""
import numpy as np
import pytest

import adamw_groups_cases as gc
import adamw_mx4_cases as m4
import f32_tree
import mxfp4_rht_ref as ref
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import test_gpu_adamw_groups as groups  # noqa: E402
import test_gpu_adamw_mx as amx  # noqa: E402
import test_gpu_adamw_mx4 as amx4  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402

pytestmark = pytest.mark.gpu
tf, stream = amx.tf, base.stream
LIST = ((1, "identity", 1), (3, "negative_v", 0), (2, "identity", 1), (2, "zero_den", 2), (3, "planes", 0))
CANCEL = 2   # the bucket of LIST whose p is the cancel set
MASKS = {8: 0x9E3779B9, 16: 0, 32: 0xFFFFFFFF, 64: 0x9E3779B9}


def kernel(total, zero, rceil):
    return f"k_adamw_ag_mxfp4_rht<{total}, {tf(zero)}, {tf(rceil)}>"


@pytest.mark.parametrize("case", ["clip", "N-inf"])
@pytest.mark.parametrize("total", sc.RANKS)
@amx.flag_pairs
def test_planes_of_the_mxfp4_step_rows_of_the_rotated_all_gather(total, zero, rceil, case):
    mask = MASKS[total]
    tiles, group_of = tuple(k for k, _, _ in LIST), tuple(g for _, _, g in LIST)
    data = m4.make(total, 300 + total, LIST)
    data[CANCEL] = (ref.cancel_shard(total, 256 * tiles[CANCEL], total),) + data[CANCEL][1:]
    buckets, second = amx4.mx4_buckets(total, tiles), amx4.mx4_buckets(total, tiles)
    planes = amx4.Planes(buckets, "flat", data)
    hyper0, nsq = one.uniform_cases(total)[case]
    grps = (hyper0, gc.GROUPS[1], gc.GROUPS[2])
    small, small2 = amx4.SmallG(gc.hyper_array(3, grps), nsq), amx4.SmallG(gc.hyper_array(3, grps), nsq)
    args = planes.args()
    plan = base.any_plan(t.SWING, sc.SIDE[total], total)
    with t.tuned(pipe_grid=sc.GRID):   # every workgroup walks at least three tiles: the slot rotates
        with t.launch_trace() as tr:
            plan.adamw_all_gather_shards_mxfp4_rht(args, group_of, small.hyper, 3, mask, small.norm_sq, small.info, zero_grad=zero,
                                                   rceil=rceil, stream=stream())
        assert tr.kernels == [kernel(total, zero, rceil)]
        new = [g.copy() for s in planes.s for g in s.got()]
        new_rows = [b.got() for b in buckets]
        new_info = groups.info_words(small)
        planes.restore()
        twin_args = [b.arg + a[5:] for b, a in zip(second, args)]
        plan.adamw_all_gather_shards_mxfp4(twin_args, group_of, small2.hyper, 3, small2.norm_sq, small2.info, zero_grad=zero, rceil=rceil,
                                           stream=stream())
        old = [g.copy() for s in planes.s for g in s.got()]
        for b in second:
            b.restore()
        plan.all_gather_shards_mxfp4_rht([b.arg + (a[5], a[9]) for b, a in zip(second, args)], mask, rceil=rceil, stream=stream())
    assert len(new) == len(old)
    for k, (a, b) in enumerate(zip(new, old)):
        assert f32_tree.same_f32(a.view(np.float32), b.view(np.float32)), f"plane buffer {k}"
    for i, (a, b) in enumerate(zip(new_rows, [b.got() for b in second])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"bucket {i}: rows and scales"
    assert np.array_equal(new_info, groups.info_words(small2))
    assert new_info.view(np.float32)[2] == (1.0 if case == "N-inf" else 0.0)
    # the rows are the rotated ones, of p on a skipped step, and the NaN blocks are there
    we, ws = ref.expected_rows(data[CANCEL][0], mask, rceil)
    n = buckets[CANCEL].n
    assert np.array_equal(new_rows[CANCEL][0][0, :n // 2], we) and np.array_equal(new_rows[CANCEL][1][0, :n // 32], ws)
    assert any((r[1][:total, :b.n // 32] == 0xFF).any() for r, b in zip(new_rows, buckets))
    plan.close()
