"""Grouped fused BO allreduce / reduce-scatter (allred_plan_execute_group,
allred_plan_reduce_scatter_group, allred_plan_group_launches; k_tree_group) against the
CPU oracle.

Every comparison is BIT-EXACT against oracle.allreduce("bo", ...) of each bucket: block b
is tree b of the schedule, every add rounded to bf16.  The inputs are uniform bf16
patterns 0x3F80-0x42C8, for which Swing's per-block trees differ in rounding, so a wrong
block, order row or bucket changes bits.  Every bucket is a buffer of its own: its rows
at its stride, the stride skew and one guard row behind the last rank filled with a
sentinel, and the WHOLE buffer is compared — what a call must not touch keeps its bits.

Shapes, the smallest that reach each way the kernel's walk can go wrong (a tile is 256
elements of every rank; P ranks; n = 256 P k is k tiles per block, P k tiles):
  one bucket; unequal buckets [1, 3, 2, 5] tiles per block with unlike strides at the
  default grid (at most one tile per workgroup at P = 8, several at P = 64); the grid
  capped at 5 (workgroups cross bucket ends mid-walk, both LDS buffers in use) and, at
  P = 8, at 24 (strides of 24 tiles pass the whole 8-tile bucket); 64 one-tile-per-block
  buckets; 65 buckets (two grouped launches); a list mixing the grouped route with the
  two routes that keep their own launches."""
import functools

import numpy as np
import pytest

import oracle
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5A5

SCHEDULES = [(algo, side, total) for side, total in ((4, 8), (4, 16), (8, 64)) for algo in (t.SWING, t.RECDUB)]
SCHEDULES.append((t.SWING_1D, 1, 8))
sched = pytest.mark.parametrize("algo,side,total", SCHEDULES, ids=[f"algo{a}-{s}x{p}" for a, s, p in SCHEDULES])
UNEQUAL = (1, 3, 2, 5)   # tiles per block of the unequal list


@functools.lru_cache(maxsize=None)
def reference(algo, side, total, n, salt=0):
    """(inputs, oracle BO allreduce of them), both (total, n) uint16, computed once and read-only."""
    rng = np.random.default_rng(1000 * total + 10 * algo + n % 97 + 7919 * salt)
    data = rng.integers(0x3F80, 0x42C8, (total, n)).astype(np.uint16)
    want = [r.copy() for r in data]
    oracle.allreduce("bo", algo, side, want, total)
    want = np.stack(want)
    data.flags.writeable = False
    want.flags.writeable = False
    return data, want


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV)


def stream():
    return torch.cuda.current_stream()


class Bucket:
    """One bucket in a device buffer of its own: (total + 1) rows of `stride` elements, the
    skew and the guard row = SENT."""

    def __init__(self, data, want, stride=None):
        self.total, self.n = data.shape
        self.want = want
        self.stride = stride or t.preferred_rank_stride(self.n)
        self.host = np.full((self.total + 1, self.stride), SENT, dtype=np.uint16)
        self.host[:self.total, :self.n] = data
        self.buf = to_dev(self.host)
        self.arg = (self.buf.data_ptr(), self.stride, self.n)

    def restore(self):
        self.buf.copy_(to_dev(self.host))

    def got(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(np.uint16)

    def after_allreduce(self):
        e = self.host.copy()
        e[:self.total, :self.n] = self.want
        return e

    def after_reduce_scatter(self):
        e = self.host.copy()
        blk = self.n // self.total
        for b in range(self.total):
            e[b, b * blk:(b + 1) * blk] = self.want[b, b * blk:(b + 1) * blk]
        return e


def make(algo, side, total, n, salt=0, own_stride=True):
    data, want = reference(algo, side, total, n, salt)
    return Bucket(data, want, None if own_stride else n)


def unequal(algo, side, total):
    """[256 P, 256 P 3, 256 P 2, 256 P 5] elements per rank; strides preferred_rank_stride(n) and n in turn"""
    return [make(algo, side, total, 256 * total * k, salt=i, own_stride=i % 2 == 0) for i, k in enumerate(UNEQUAL)]


def check_allreduce(buckets):
    for i, b in enumerate(buckets):
        got = b.got()
        assert np.array_equal(got[:b.total, :b.n], b.want), f"bucket {i} (n={b.n})"
        assert np.array_equal(got, b.after_allreduce()), f"bucket {i} (n={b.n}): skew or guard row written"


def any_plan(algo, side, total, exec_mode=t.EXEC_FUSED, variant=t.BO):
    """a plan for its schedule: its own bucket size (one tile per block) is not the lists'"""
    return t.Plan(algo, variant, side, 256 * total, total, exec_mode)


# ------------------------------------------------------------------ allreduce
@sched
def test_one_bucket_is_plan_execute(algo, side, total):
    n = 256 * total * 2
    b = make(algo, side, total, n)
    plan = any_plan(algo, side, total)
    assert plan.group_launches([b.arg]) == 1
    plan.execute_group([b.arg], stream())
    check_allreduce([b])
    own = t.Plan(algo, t.BO, side, n, total, t.EXEC_FUSED)
    ref = to_dev(b.host)
    own.execute(ref.data_ptr(), b.stride, None, stream())
    torch.cuda.synchronize()
    assert np.array_equal(b.got(), ref.cpu().numpy().view(np.uint16))
    own.close()
    plan.close()


@pytest.mark.parametrize("grid", [0, 5], ids=["default-grid", "grid5"])
@sched
def test_unequal_buckets(algo, side, total, grid):
    """Default grid: one workgroup per tile at P = 8 (88 tiles), several tiles per workgroup at
    P = 64 (704 tiles on 512).  pipe_grid = 5: every workgroup walks through all four buckets,
    crossing their ends mid-walk, with both LDS buffer parities in use."""
    buckets = unequal(algo, side, total)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.group_launches([b.arg for b in buckets]) == 1
        plan.execute_group([b.arg for b in buckets], stream())
        check_allreduce(buckets)
    plan.close()


@pytest.mark.parametrize("algo,side", [(t.SWING, 4), (t.RECDUB, 4), (t.SWING_1D, 1)])
def test_capped_grid_passes_a_whole_bucket(algo, side):
    """P = 8, pipe_grid = 24 over buckets of 8, 24, 16 and 40 tiles: a stride of 24 tiles passes
    the 8-tile bucket (workgroups 8 .. 23 never enter it) and, later, the 16-tile one."""
    buckets = unequal(algo, side, 8)
    plan = any_plan(algo, side, 8)
    with t.tuned(pipe_grid=24):
        plan.execute_group([b.arg for b in buckets], stream())
        check_allreduce(buckets)
    plan.close()


def test_64_one_tile_per_block_buckets_in_one_launch():
    algo, side, total = t.SWING, 4, 8
    buckets = [make(algo, side, total, 256 * total, salt=i) for i in range(_lib.GROUP_MAX)]
    plan = any_plan(algo, side, total)
    assert plan.group_launches([b.arg for b in buckets]) == 1
    plan.execute_group([b.arg for b in buckets], stream())
    check_allreduce(buckets)
    plan.close()


def test_65_buckets_split_into_two_launches():
    algo, side, total = t.SWING, 4, 8
    buckets = [make(algo, side, total, 256 * total * (1 + i % 2), salt=i) for i in range(_lib.GROUP_MAX + 1)]
    plan = any_plan(algo, side, total)
    assert plan.group_launches([b.arg for b in buckets]) == 2
    plan.execute_group([b.arg for b in buckets], stream())
    check_allreduce(buckets)
    plan.close()


def test_mixed_routes():
    """A bucket that is not whole tiles (the register form), one on the persistent 64-rank route
    (1280 tiles), and two small whole-tile buckets around them, which share ONE grouped launch."""
    algo, side, total = t.SWING, 8, 64
    sizes = [256 * total, 8 * total * 3, 256 * total * 20, 256 * total * 2]
    buckets = [make(algo, side, total, n, salt=i) for i, n in enumerate(sizes)]
    args = [b.arg for b in buckets]
    plan = any_plan(algo, side, total)
    alone = 0
    for n in sizes[1:3]:
        own = t.Plan(algo, t.BO, side, n, total, t.EXEC_FUSED)
        alone += own.launches
        own.close()
    assert plan.group_launches(args) == 1 + alone
    plan.execute_group(args, stream())
    check_allreduce(buckets)
    with t.tuned(fused_form=2):   # grouping off: every bucket its own launch
        assert plan.group_launches(args) == len(args)
        for b in buckets:
            b.restore()
        plan.execute_group(args, stream())
        check_allreduce(buckets)
    plan.close()


# ------------------------------------------------------------------ reduce-scatter
@pytest.mark.parametrize("grid", [0, 5], ids=["default-grid", "grid5"])
@sched
def test_reduce_scatter_group(algo, side, total, grid):
    """Block b of rank b's row of every bucket = the oracle's block b; everything else in every
    buffer — the other blocks, the skew, the guard row — keeps its input bits."""
    buckets = unequal(algo, side, total)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        plan.reduce_scatter_group([b.arg for b in buckets], stream())
        for i, b in enumerate(buckets):
            got, blk = b.got(), b.n // b.total
            for r in range(b.total):
                assert np.array_equal(got[r, r * blk:(r + 1) * blk], b.want[r, r * blk:(r + 1) * blk]), (i, r)
            assert np.array_equal(got, b.after_reduce_scatter()), f"bucket {i}: something else was written"
    plan.close()


# ------------------------------------------------------------------ arbitrary bits, graph capture
def test_arbitrary_bit_patterns_equal_plan_execute():
    """NaN payloads, infinities and denormals in one bucket of a group: the bits of Plan.execute."""
    algo, side, total = t.SWING, 4, 16
    n = 256 * total * 3
    raw = np.random.default_rng(5).integers(0, 0x10000, (total, n)).astype(np.uint16)
    buckets = unequal(algo, side, total)
    odd = Bucket(raw, raw)
    buckets.insert(2, odd)
    own = t.Plan(algo, t.BO, side, n, total, t.EXEC_FUSED)
    ref = to_dev(odd.host)
    own.execute(ref.data_ptr(), odd.stride, None, stream())
    torch.cuda.synchronize()
    odd.want = ref.cpu().numpy().view(np.uint16)[:total, :n].copy()
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=5):
        plan.execute_group([b.arg for b in buckets], stream())
        check_allreduce(buckets)
    own.close()
    plan.close()


def test_graph_capture_replays_the_eager_bits():
    """The grouped launch's table travels in the kernel arguments, so the call can be captured:
    one capture on one stream (a single linear branch), one replay on restored data."""
    algo, side, total = t.SWING, 4, 16
    buckets = unequal(algo, side, total)
    args = [b.arg for b in buckets]
    plan = any_plan(algo, side, total)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.execute_group(args, s)
    s.synchronize()
    eager = [b.got() for b in buckets]
    check_allreduce(buckets)
    for b in buckets:
        b.restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.execute_group(args, s)
    torch.cuda.synchronize()
    for b in buckets:   # a capture runs nothing
        assert np.array_equal(b.got(), b.host)
    g.replay()
    torch.cuda.synchronize()
    for b, e in zip(buckets, eager):
        assert np.array_equal(b.got(), e)
    del g
    plan.close()


# ------------------------------------------------------------------ refusals
def test_refusals_leave_every_buffer_untouched():
    algo, side, total = t.SWING, 4, 8
    buckets = unequal(algo, side, total)
    args = [b.arg for b in buckets]
    s = stream()

    def refused(status, call):
        with pytest.raises(t.AllredError) as e:
            call()
        assert e.value.status == status, (e.value.status, status)

    others = [any_plan(algo, side, total, variant=t.LO), any_plan(algo, side, total, variant=t.MEM),
              any_plan(algo, side, total, exec_mode=t.EXEC_STEPS)]
    for plan in others:
        refused(_lib.ERR_UNSUPPORTED, lambda: plan.execute_group(args, s))
        refused(_lib.ERR_UNSUPPORTED, lambda: plan.reduce_scatter_group(args, s))
        refused(_lib.ERR_UNSUPPORTED, lambda: plan.group_launches(args))
        plan.close()
    plan = any_plan(algo, side, total)
    ptr, stride, n = args[1]
    bad_lists = [
        args + [(ptr + 2 * stride, stride, n)],                   # inside bucket 1's rows
        args[:1] + [(ptr, stride, n)] + args[1:],                 # the same bucket twice
        args[:1] + args[2:] + [(ptr, stride, n + 8 * total - 8)],  # n % (8 P) != 0, last in the list
        args[:1] + args[2:] + [(ptr, n - 8, n)],                  # stride < n
        args[:1] + args[2:] + [(ptr, stride + 4, n)],             # stride % 8 != 0
        args[:1] + args[2:] + [(ptr + 2, stride, n)],             # not 16-byte aligned
        args[:1] + args[2:] + [(0, stride, n)],                   # a null bucket
        args[:1] + args[2:] + [(ptr, stride, 0)],                 # an empty bucket
    ]
    for bad in bad_lists:
        refused(_lib.ERR_ARG, lambda: plan.execute_group(bad, s))
        refused(_lib.ERR_ARG, lambda: plan.reduce_scatter_group(bad, s))
        refused(_lib.ERR_ARG, lambda: plan.group_launches(bad))
    arr = (_lib.Bucket * len(args))(*args)
    assert _lib.lib.allred_plan_execute_group(plan._h, arr, -1, None) == _lib.ERR_ARG
    assert _lib.lib.allred_plan_execute_group(plan._h, None, 2, None) == _lib.ERR_ARG
    assert _lib.lib.allred_plan_reduce_scatter_group(plan._h, None, 2, None) == _lib.ERR_ARG
    assert _lib.lib.allred_plan_group_launches(plan._h, None, 2) == _lib.ERR_ARG
    assert _lib.lib.allred_plan_execute_group(None, arr, len(args), None) == _lib.ERR_ARG
    # count == 0: OK, nothing launched
    plan.execute_group([], s)
    plan.reduce_scatter_group([], s)
    assert plan.group_launches([]) == 0
    assert _lib.lib.allred_plan_execute_group(plan._h, None, 0, None) == _lib.OK
    plan.close()
    for i, b in enumerate(buckets):
        assert np.array_equal(b.got(), b.host), f"bucket {i} written by a refused call"
