"""The MXFP4 all-gather from fp32 shards (allred_plan_all_gather_shards_mxfp4 and its _launches twin; k_ag_group_mxfp4)
against tests/mxfp4_ref.py, BIT FOR BIT, on tests/mx4_cases.py's planted blocks.  The buffers are
test_gpu_shards_mxfp8's buckets at HALF the row payload and test_gpu_shards_f32's Shards; WHOLE buffers are
compared around sentinels, so a stray write anywhere fails."""
import functools

import numpy as np
import pytest

import mx4_cases
import mxfp4_ref as ref
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_shards_f32 as f32t  # noqa: E402  (its Shards, schedules and parametrisations)
import test_gpu_shards_mxfp8 as mx8  # noqa: E402  (its bucket buffers)

pytestmark = pytest.mark.gpu
Shards, any_plan, stream = f32t.Shards, f32t.any_plan, f32t.stream


@functools.lru_cache(maxsize=None)
def cases(total, blk, seed):
    return mx4_cases.shard(total, blk, seed)


@functools.lru_cache(maxsize=None)
def expected(total, blk, seed, rceil):
    return ref.expected_rows(cases(total, blk, seed), rceil)


class Mx4Bucket(mx8.MxBucket):
    """mx8.MxBucket with n / 2 payload bytes per element row and a row stride to match"""

    def __init__(self, total, n, skew=False):
        super().__init__(total, n, skew)
        self.row_stride = n // 2 + (48 if skew else 0)
        self.host = (np.full((total + 1, self.row_stride), mx8.SENT8, dtype=np.uint8), self.host[1])
        self.buf = (mx8.to_dev8(self.host[0]), self.buf[1])
        self.arg = (self.buf[0].data_ptr(), self.row_stride, self.buf[1].data_ptr(), self.scale_stride, n)

    def after(self, elems, scales):
        e, s = self.host[0].copy(), self.host[1].copy()
        e[:self.total, :self.n // 2] = elems
        s[:self.total, :self.n // 32] = scales
        return e, s


def unequal(total, seed=0):
    """1, 3, 2 and 5 tiles per block, every other bucket with stride skews; the keys of the shard data"""
    buckets = [Mx4Bucket(total, 256 * total * k, skew=i % 2 == 1) for i, k in enumerate(f32t.UNEQUAL)]
    return buckets, [(total, 256 * k, 10 * seed + i) for i, k in enumerate(f32t.UNEQUAL)]


def filled(buckets, keys, layout):
    shards = Shards(buckets, layout)
    shards.fill([cases(*k) for k in keys])
    return shards


def check_all(buckets, keys, rceil, what):
    for i, (b, key) in enumerate(zip(buckets, keys)):
        b.check(b.after(*expected(*key, rceil)), f"bucket {i} (n={b.n}, rceil={rceil}): {what}")


def kernel(total, rceil):
    return f"k_ag_group_mxfp4<{total}, {'true' if rceil else 'false'}>"


@f32t.grids
@f32t.layouts
@f32t.sched
def test_every_row_receives_the_quantised_shard(algo, side, total, layout, grid):
    """(a) every P and the 1-D plan: the pair reduction, the row split, the odd-tile tail, the scale words; one launch"""
    buckets, keys = unequal(total)
    shards = filled(buckets, keys, layout)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.shards_mxfp4_launches(shards.args()) == 1
        for rceil in (False, True):
            for b in buckets:
                b.restore()
            with t.launch_trace() as tr:
                plan.all_gather_shards_mxfp4(shards.args(), rceil=rceil, stream=stream())
            assert tr.kernels == [kernel(total, rceil)]
            check_all(buckets, keys, rceil, "block b of every row = mxfp4(shard block b)")
            mx8.shards_unchanged(shards)
    plan.close()


def test_planted_blocks_as_known_answers_and_dequantised():
    """(b) the first two planted tiles as literals, from rank 0's and the last rank's rows; (e) mxfp4_dequantize of the
    output = the reference's float64 dequantisation cast to fp32, NaN where the scale is 0xFF"""
    total, tie = 8, 16 * mx4_cases.TIES
    b = Mx4Bucket(total, 256 * total)
    shards = filled([b], [(total, 256, 0)], "compact")
    plan = any_plan(t.SWING, 4, total)
    for rceil in (False, True):
        b.restore()
        plan.all_gather_shards_mxfp4(shards.args(), rceil=rceil, stream=stream())
        e, s = b.got()
        for r in (0, total - 1):
            assert list(s[r, :13]) == mx4_cases.SCALES[rceil]
            assert list(e[r, tie + 1:tie + 9]) == mx4_cases.TIE_BYTES and e[r, tie] >> 4 == 7
            assert (e[r, 9 * 16:12 * 16] == 0).all() and set(e[r, 8 * 16:9 * 16]) <= {0x00, 0x08, 0x80, 0x88}
            assert e[r, 3 * 16] & 0xF == 7 and e[r, 16 + 8] >> 4 == (5 if rceil else 7)   # amax 6 -> 6; 1.5 + ulp -> 3 x 2^-1, or saturated
        got = t.mxfp4_dequantize(e[:total, :b.n // 2], s[:total, :b.n // 32])
        with np.errstate(over="ignore"):
            want = ref.dequantize64(*expected(total, 256, 0, rceil)).astype(np.float32)
        nan = np.isnan(want)
        assert got.dtype == np.float32 and nan.sum() == 12 * 32 and np.array_equal(np.isnan(got), np.broadcast_to(nan, got.shape))
        assert np.array_equal(got[:, ~nan].view(np.uint32), np.broadcast_to(want[~nan].view(np.uint32), (total, (~nan).sum())))
    plan.close()


@pytest.mark.parametrize("count", [32, 33, 65])
def test_32_buckets_per_launch(count):
    """(c)"""
    total, launches = 8, -(-count // _lib.MX_GROUP_MAX)
    buckets = [Mx4Bucket(total, 256 * total, skew=i % 3 == 0) for i in range(count)]
    keys = [(total, 256, 100 + i % 5) for i in range(count)]
    shards = filled(buckets, keys, "flat")
    plan = any_plan(t.SWING, 4, total)
    assert plan.shards_mxfp4_launches(shards.args()) == launches
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp4(shards.args(), rceil=True, stream=stream())
    assert tr.kernels == [kernel(total, True)] * launches
    check_all(buckets, keys, True, f"{count} buckets in {launches} launches")
    mx8.shards_unchanged(shards)
    plan.close()


@pytest.mark.parametrize("rceil", [False, True])
def test_captured_once_replayed_twice_on_rewritten_shards(rceil):
    """(d) the tables travel by value: one capture on a side stream, two replays with the shards rewritten in between"""
    total = 16
    buckets, keys = unequal(total, seed=3)
    shards = filled(buckets, keys, "wide")
    args = shards.args()
    plan = any_plan(t.SWING, 4, total)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):   # an eager call first: nothing is loaded inside the capture
        plan.all_gather_shards_mxfp4(args, rceil=rceil, stream=s)
    s.synchronize()
    check_all(buckets, keys, rceil, "eager")
    for b in buckets:
        b.restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.all_gather_shards_mxfp4(args, rceil=rceil, stream=s)
    torch.cuda.synchronize()
    for b in buckets:
        b.check(b.host, "a capture runs nothing")
    for ks in (keys, [(tt, blk, seed + 50) for tt, blk, seed in keys]):
        shards.fill([cases(*k) for k in ks])
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        check_all(buckets, ks, rceil, "replay")
        mx8.shards_unchanged(shards)
    del g
    plan.close()


def test_a_refused_list_leaves_every_buffer_untouched():
    """(f) through the plan: the payload is n / 2 bytes (abutting and overlapping rows: tests/test_mx4_ranges.py)"""
    total = 8
    buckets, keys = unequal(total)
    shards = filled(buckets, keys, "compact")
    args = shards.args()
    rows, rs, scales, ss, n, shard, sst = args[-1]

    def refused(call, lst):
        with pytest.raises(t.AllredError) as e:
            call(lst)
        assert e.value.status == _lib.ERR_ARG

    plan = any_plan(t.SWING, 4, total)
    for call in (lambda lst: plan.all_gather_shards_mxfp4(lst, stream=stream()), lambda lst: plan.all_gather_shards_mxfp4(lst, rceil=True, stream=stream()),
                 plan.shards_mxfp4_launches):
        refused(call, args[:-1] + [(rows, n // 2 - 16, scales, ss, n, shard, sst)])
    assert args[0][1] == args[0][4] // 2 and plan.shards_mxfp4_launches(args) == 1   # a stride of n / 2 exactly is accepted
    refused(plan.shards_mxfp8_launches, args)         # the MXFP8 call on the same list demands row_stride >= n
    plan.close()
    for b in buckets:
        b.check(b.host, "written by a refused call")
    mx8.shards_unchanged(shards)
