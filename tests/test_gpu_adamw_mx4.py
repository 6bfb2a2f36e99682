"""allred_plan_adamw_all_gather_shards_mxfp4 / allred_plan_adamw_shards_mxfp4_launches (k_adamw_ag_mxfp4): AdamW with
parameter groups inside the MXFP4 all-gather's launch, against tests/adamw_mx4_cases.py's expectation — adamw_ref.step,
then mxfp4_ref.expected_rows of the new param plane — BIT FOR BIT: the planes fp32 as uint32, NaNs by class; nibble and
scale bytes exactly.  The buffers are test_gpu_adamw_mx's with test_gpu_shards_mxfp4's half-payload element rows;
WHOLE buffers are compared around sentinels."""
import functools

import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_mx4_cases as m4
import f32_tree
import mxfp4_ref as ref
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_adamw_groups as groups  # noqa: E402
import test_gpu_adamw_mx as amx  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
from test_gpu_shards_mxfp4 import Mx4Bucket  # noqa: E402

pytestmark = pytest.mark.gpu
Planes, check_all, SmallG, stream, tf = amx.Planes, amx.check_all, amx.SmallG, base.stream, amx.tf
P_, G_, M_, V_ = range(4)
FLAGS = m4.FLAGS


def kernel(total, zero, rceil):
    return f"k_adamw_ag_mxfp4<{total}, {tf(zero)}, {tf(rceil)}>"


def mx4_buckets(total, tiles):
    return [Mx4Bucket(total, 256 * total * k, skew=i % 2 == 1) for i, k in enumerate(tiles)]


@functools.lru_cache(maxsize=None)
def list_data(total, seed):
    return m4.make(total, seed)


@base.grids
@base.layouts
@base.sched
def test_step_and_mxfp4_all_gather(algo, side, total, layout, grid):
    """1. adamw_mx4_cases.LIST for all four flag pairs, clipping active: planes, every rank's nibble row and scale row,
    gaps, guards and skew; one launch; at the small grid every workgroup walks at least 3 tiles (the slot rotates)."""
    buckets = mx4_buckets(total, m4.TILES)
    data = list_data(total, 10 * total)
    planes = Planes(buckets, layout, data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    plan = base.any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.adamw_shards_mxfp4_launches(planes.args()) == 1
        for zero, rceil in FLAGS:
            planes.restore()
            small.restore()
            with t.launch_trace() as tr:
                plan.adamw_all_gather_shards_mxfp4(planes.args(), m4.GROUP_OF, small.hyper, 3, small.norm_sq, small.info,
                                                   zero_grad=zero, rceil=rceil, stream=stream())
            assert tr.kernels == [kernel(total, zero, rceil)]
            if grid:
                assert tr.grids == [grid] and total * sum(m4.TILES) >= 3 * grid
            want = m4.expect(data, m4.GROUP_OF, nsq, total, zero, rceil)
            assert want[2][1] < 1 and want[2][2] == 0   # clipping is active, the step is not skipped
            check_all(buckets, planes, small, want, f"zero_grad={zero}, rceil={rceil}")
    plan.close()


GUARANTEE_LIST = ((1, "identity", 1), (3, "negative_v", 0), (2, "zero_den", 2), (3, "planes", 0), (1, "planes", 2))


@pytest.mark.parametrize("algo,side,total", [(t.SWING, 4, 8), (t.SWING, 8, 64)], ids=["swing-8", "swing-8x8"])
@amx.flag_pairs
def test_planes_of_the_groups_call_rows_of_the_mxfp4_all_gather(algo, side, total, zero, rceil):
    """2. allred.h's guarantee, p' partly NaN (negative_v, zero_den): the planes are those the groups call leaves, the
    rows and scales what all_gather_shards_mxfp4 writes from that param plane, info equal, 0xFF scales present."""
    tiles = tuple(k for k, _, _ in GUARANTEE_LIST)
    group_of = tuple(g for _, _, g in GUARANTEE_LIST)
    buckets, second = mx4_buckets(total, tiles), mx4_buckets(total, tiles)
    rows16 = one.rows_buckets(total, tiles)
    planes = Planes(buckets, "flat", m4.make(total, 200 + total, GUARANTEE_LIST))
    nsq = adamw_cases.norm_sq(total)
    small, small2 = SmallG(gc.hyper_array(), nsq), SmallG(gc.hyper_array(), nsq)
    args = planes.args()
    plan = base.any_plan(algo, side, total)
    plan.adamw_all_gather_shards_mxfp4(args, group_of, small.hyper, 3, small.norm_sq, small.info, zero_grad=zero, rceil=rceil, stream=stream())
    new = [g.copy() for s in planes.s for g in s.got()]
    new_rows = [b.got() for b in buckets]
    new_info = groups.info_words(small)
    planes.restore()
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32_groups([r.arg + a[5:] for r, a in zip(rows16, args)], group_of, small2.hyper, 3, small2.norm_sq,
                                                small2.info, zero_grad=zero, stream=stream())
        plan.all_gather_shards_mxfp4([b.arg + (a[5], a[9]) for b, a in zip(second, args)], rceil=rceil, stream=stream())
    assert tr.kernels == [f"k_adamw_ag_groups_f32<{total}, {tf(zero)}>", f"k_ag_group_mxfp4<{total}, {tf(rceil)}>"]
    old = [g.copy() for s in planes.s for g in s.got()]
    assert len(new) == len(old)
    for k, (a, b) in enumerate(zip(new, old)):
        assert f32_tree.same_f32(a.view(np.float32), b.view(np.float32)), f"plane buffer {k}"
    for i, (a, b) in enumerate(zip(new_rows, [b.got() for b in second])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"bucket {i}: rows and scales"
    assert np.array_equal(new_info, groups.info_words(small2))
    assert any((r[1][:total, :b.n // 32] == 0xFF).any() for r, b in zip(new_rows, buckets))
    assert not np.array_equal(new[0], planes.s[P_].host[0])   # something was computed
    plan.close()


@pytest.mark.parametrize("case", ["N-inf", "clip"])
def test_the_skipped_step_and_its_neighbour(case):
    """3. N = +Inf: the planes untouched, the rows mxfp4(p), zero_grad still zeroes, info[2] == 1; `clip` next to it."""
    algo, side, total = t.SWING, 8, 64
    hyper0, nsq = one.uniform_cases(total)[case]
    grps = (hyper0, gc.GROUPS[1], gc.GROUPS[2])
    lst = ((1, "planes", 2), (2, "identity", 1), (1, "planes", 0))
    group_of = tuple(g for _, _, g in lst)
    buckets = mx4_buckets(total, tuple(k for k, _, _ in lst))
    data = m4.make(total, 7, lst)
    planes = Planes(buckets, "wide", data)
    small = SmallG(gc.hyper_array(3, grps), nsq)
    plan = base.any_plan(algo, side, total)
    for zero, rceil in FLAGS:
        planes.restore()
        small.restore()
        plan.adamw_all_gather_shards_mxfp4(planes.args(), group_of, small.hyper, 3, small.norm_sq, small.info, zero_grad=zero,
                                           rceil=rceil, stream=stream())
        want = m4.expect(data, group_of, nsq, total, zero, rceil, grps)
        if case == "clip":
            assert want[2][2] == 0 and want[2][1] < 1
        else:
            assert want[2][2] == 1
            for d, v, (e, s) in zip(data, want[0], want[1]):
                assert all(np.array_equal(v[k].view(np.uint32), d[k].view(np.uint32)) for k in (P_, M_, V_))
                we, ws = ref.expected_rows(d[P_], rceil)
                assert np.array_equal(e, we) and np.array_equal(s, ws)
                assert (v[G_].view(np.uint32) == 0).all() if zero else np.array_equal(v[G_].view(np.uint32), d[G_].view(np.uint32))
        check_all(buckets, planes, small, want, f"{case}, zero_grad={zero}, rceil={rceil}")
    plan.close()


def test_33_buckets_are_two_launches_and_info_is_written_once():
    """4. one-tile buckets, bucket i in group i % 3 (group 1: identity buckets)"""
    algo, side, total, count = t.SWING, 4, 8, 33
    lst = tuple((1, "identity" if i % 3 == 1 else "planes", i % 3) for i in range(count))
    group_of = [g for _, _, g in lst]
    buckets = [Mx4Bucket(total, 256 * total, skew=i % 3 == 0) for i in range(count)]
    data = m4.make(total, 100, lst)
    planes = Planes(buckets, "flat", data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    plan = base.any_plan(algo, side, total)
    assert plan.adamw_shards_mxfp4_launches(planes.args()) == 2
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_mxfp4(planes.args(), group_of, small.hyper, 3, small.norm_sq, small.info, zero_grad=True, rceil=True,
                                           stream=stream())
    assert tr.kernels == [kernel(total, True, True)] * 2
    check_all(buckets, planes, small, m4.expect(data, group_of, nsq, total, True, True), "33 buckets")
    plan.close()


def test_a_refused_list_leaves_every_buffer_untouched():
    """5. through the plan: the row payload is n / 2 bytes"""
    algo, side, total = t.SWING, 4, 8
    buckets = [Mx4Bucket(total, 256 * total * k) for k in m4.TILES]   # no skew: row_stride = n / 2 exactly
    data = list_data(total, 71)
    planes = Planes(buckets, "wide", data)
    small = SmallG(gc.hyper_array(), adamw_cases.norm_sq(total))
    args = planes.args()
    rows, rs, scales, ss, n, *rest = args[-1]
    bad = args[:-1] + [(rows, n // 2 - 16, scales, ss, n, *rest)]
    plan = base.any_plan(algo, side, total)

    def refused(call, lst):
        with pytest.raises(t.AllredError) as e:
            call(lst)
        assert e.value.status == _lib.ERR_ARG

    for rceil in (False, True):
        refused(lambda lst: plan.adamw_all_gather_shards_mxfp4(lst, m4.GROUP_OF, small.hyper, 3, small.norm_sq, small.info, rceil=rceil,
                                                               stream=stream()), bad)
    refused(plan.adamw_shards_mxfp4_launches, bad)
    assert rs == n // 2 and plan.adamw_shards_mxfp4_launches(args) == 1   # a stride of n / 2 exactly is accepted
    refused(plan.adamw_shards_mxfp8_launches, args)                       # the MXFP8 twin demands row_stride >= n
    refused(lambda lst: plan.adamw_all_gather_shards_mxfp8(lst, m4.GROUP_OF, small.hyper, 3, small.norm_sq, small.info, stream=stream()), args)
    plan.close()
    planes.check(data, "written by a refused call")
    for b in buckets:
        b.check(b.host, "rows written by a refused call")
    small.check(None, "written by a refused call")
