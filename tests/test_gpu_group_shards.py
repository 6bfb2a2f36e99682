"""Grouped reduce-scatter into, and grouped all-gather from, per-bucket shard buffers
(allred_plan_reduce_scatter_shards, allred_plan_all_gather_shards,
allred_plan_shards_launches; k_tree_group with its shard table, k_ag_group).

Reduce-scatter expectations are BIT-EXACT against oracle.allreduce("bo", ...) of each bucket
(block b = tree b of the schedule, every add rounded to bf16) on uniform bf16 patterns
0x3F80-0x42C8, for which Swing's per-block trees differ in rounding.  All-gather
expectations need no oracle: block b of every row equals the source block's bits.

Every bucket is a buffer of its own — its rows at its stride, the stride skew and one guard
row behind the last rank filled with a sentinel — and every shard buffer is sentinel-filled
with a guard behind it; WHOLE buffers are compared, so a stray write anywhere fails.  Shard
layouts: compact (shard_stride = blk), wide (blk + 64, the gaps sentinel) and flat — ONE
rank-major buffer of `total` rows of F = sum of blk elements shared by all buckets, bucket
i's shard at column off_i with shard_stride = F, so the buckets' enclosing ranges interleave.

Shapes, the smallest that reach each way the walk can go wrong (a tile is 256 elements of
every rank; n = 256 P k is k tiles per block): unequal buckets [1, 3, 2, 5] tiles per block,
strides preferred_rank_stride(n) and n in turn, at the default grid, at pipe_grid 5
(workgroups cross bucket ends mid-walk with the next tile's load in flight) and, at P = 8,
24 (a stride passes a whole bucket); 64 and 65 buckets; a list mixing the grouped route with
the two routes that keep their own launches."""
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
GUARD = 64                # sentinel elements behind a shard buffer
RS, AG = _lib.OP_REDUCE_SCATTER, _lib.OP_ALL_GATHER

SCHEDULES = [(algo, side, total) for side, total in ((4, 8), (4, 16), (8, 64)) for algo in (t.SWING, t.RECDUB)]
SCHEDULES.append((t.SWING_1D, 1, 8))
sched = pytest.mark.parametrize("algo,side,total", SCHEDULES, ids=[f"algo{a}-{s}x{p}" for a, s, p in SCHEDULES])
grids = pytest.mark.parametrize("grid", [0, 5], ids=["default-grid", "grid5"])
layouts = pytest.mark.parametrize("layout", ["compact", "wide", "flat"])
UNEQUAL = (1, 3, 2, 5)   # tiles per block of the unequal list


@functools.lru_cache(maxsize=None)
def pattern(total, n, salt=0):
    """(total, n) uint16 of bf16 patterns 0x3F80-0x42C8, computed once and read-only"""
    rng = np.random.default_rng(1000 * total + n % 97 + 7919 * salt)
    data = rng.integers(0x3F80, 0x42C8, (total, n)).astype(np.uint16)
    data.flags.writeable = False
    return data


@functools.lru_cache(maxsize=None)
def reference(algo, side, total, n, salt=0):
    """(inputs, oracle BO allreduce of them), both (total, n) uint16, computed once and read-only"""
    data = pattern(total, n, salt)
    want = [r.copy() for r in data]
    oracle.allreduce("bo", algo, side, want, total)
    want = np.stack(want)
    want.flags.writeable = False
    return data, want


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV)


def stream():
    return torch.cuda.current_stream()


class Bucket:
    """One bucket in a device buffer of its own: (total + 1) rows of `stride` elements, the
    skew and the guard row = SENT.  want: the oracle's allreduce of data, or None."""

    def __init__(self, data, want=None, stride=None):
        self.total, self.n = data.shape
        self.blk = self.n // self.total
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

    def block(self, src, b):
        return src[b, b * self.blk:(b + 1) * self.blk]

    def after_allreduce(self):
        e = self.host.copy()
        e[:self.total, :self.n] = self.want
        return e

    def after_reduce_scatter(self):
        e = self.host.copy()
        for b in range(self.total):
            e[b, b * self.blk:(b + 1) * self.blk] = self.block(self.want, b)
        return e

    def after_all_gather(self, blocks=None):
        """block b of every row = blocks[b] (a shard's), or row b's own block b (in place)"""
        e = self.host.copy()
        for b in range(self.total):
            e[:self.total, b * self.blk:(b + 1) * self.blk] = self.block(self.host, b) if blocks is None else blocks[b]
        return e


class Shards:
    """The shard buffers of a bucket list in one layout, sentinel-filled, a guard behind each:
    compact / wide: one buffer per bucket; flat: one rank-major buffer for all of them."""

    def __init__(self, buckets, layout):
        self.buckets = buckets
        total = buckets[0].total
        self.where = []    # per bucket: (buffer, offset, stride), elements
        self.host = []
        if layout == "flat":
            F = sum(b.blk for b in buckets)
            self.host.append(np.full((total + 1) * F, SENT, dtype=np.uint16))   # the last row: the guard
            off = 0
            for b in buckets:
                self.where.append((0, off, F))
                off += b.blk
        else:
            for i, b in enumerate(buckets):
                stride = b.blk + (64 if layout == "wide" else 0)
                self.host.append(np.full(total * stride + GUARD, SENT, dtype=np.uint16))
                self.where.append((i, 0, stride))
        self.buf = [to_dev(h) for h in self.host]

    def arg(self, i):
        k, off, stride = self.where[i]
        return self.buckets[i].arg + (self.buf[k].data_ptr() + 2 * off, stride)

    def args(self, only=None):
        """5-tuples for the buckets in `only` (default: all), 3-tuples — in place — for the others"""
        return [self.arg(i) if only is None or i in only else b.arg for i, b in enumerate(self.buckets)]

    def slot(self, i, b):
        k, off, stride = self.where[i]
        return k, slice(off + b * stride, off + b * stride + self.buckets[i].blk)

    def fill(self, blocks):
        """blocks[i][b]: the blk elements of bucket i's block b, into the host mirror and the device"""
        for i, bk in enumerate(self.buckets):
            for b in range(bk.total):
                k, s = self.slot(i, b)
                self.host[k][s] = blocks[i][b]
        self.restore()

    def restore(self):
        for d, h in zip(self.buf, self.host):
            d.copy_(to_dev(h))

    def got(self):
        torch.cuda.synchronize()
        return [d.cpu().numpy().view(np.uint16) for d in self.buf]

    def after_reduce_scatter(self, only=None):
        e = [h.copy() for h in self.host]
        for i, bk in enumerate(self.buckets):
            if only is not None and i not in only:
                continue
            for b in range(bk.total):
                k, s = self.slot(i, b)
                e[k][s] = bk.block(bk.want, b)
        return e

    def check(self, expected, what):
        for k, (g, e) in enumerate(zip(self.got(), expected)):
            assert np.array_equal(g, e), f"shard buffer {k}: {what}"


def make(algo, side, total, n, salt=0, own_stride=True, oracle_too=True):
    if oracle_too:
        data, want = reference(algo, side, total, n, salt)
    else:
        data, want = pattern(total, n, salt), None
    return Bucket(data, want, None if own_stride else n)


def unequal(algo, side, total, oracle_too=True):
    """[256 P, 256 P 3, 256 P 2, 256 P 5] elements per rank; strides preferred_rank_stride(n) and n in turn"""
    return [make(algo, side, total, 256 * total * k, salt=i, own_stride=i % 2 == 0, oracle_too=oracle_too)
            for i, k in enumerate(UNEQUAL)]


def source_blocks(buckets, salt=50):
    """what a shard holds before an all-gather: per bucket (total, blk) patterns unlike the rank rows'"""
    return [pattern(b.total, b.blk, salt + i) for i, b in enumerate(buckets)]


def any_plan(algo, side, total, exec_mode=t.EXEC_FUSED, variant=t.BO):
    """a plan for its schedule: its own bucket size (one tile per block) is not the lists'"""
    return t.Plan(algo, variant, side, 256 * total, total, exec_mode)


def check_buckets(buckets, expected, what):
    for i, (b, e) in enumerate(zip(buckets, expected)):
        assert np.array_equal(b.got(), e), f"bucket {i} (n={b.n}): {what}"


def per_bucket_all_gather(algo, side, b, shard=None):
    """the bits Plan.all_gather of a plan of the bucket's own size leaves in a copy of its buffer"""
    own = t.Plan(algo, t.BO, side, b.n, b.total, t.EXEC_FUSED)
    ref = to_dev(b.host)
    if shard is None:
        own.all_gather(ref.data_ptr(), b.stride, stream=stream())
    else:
        own.all_gather(ref.data_ptr(), b.stride, shard[0], shard[1], stream=stream())
    torch.cuda.synchronize()
    own.close()
    return ref.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------ 1. all-gather in place
def all_gather_in_place(algo, side, total, grid):
    buckets = unequal(algo, side, total, oracle_too=False)
    args = [b.arg for b in buckets]
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.shards_launches(args, AG) == 1
        plan.all_gather_shards(args, stream())
        check_buckets(buckets, [b.after_all_gather() for b in buckets],
                      "block b of every row = row b's block b, everything else untouched")
    check_buckets(buckets, [per_bucket_all_gather(algo, side, b) for b in buckets], "the per-bucket Plan.all_gather bits")
    plan.close()


@grids
@sched
def test_all_gather_in_place(algo, side, total, grid):
    all_gather_in_place(algo, side, total, grid)


@pytest.mark.parametrize("algo,side", [(t.SWING, 4), (t.RECDUB, 4), (t.SWING_1D, 1)])
def test_all_gather_in_place_capped_grid_passes_a_whole_bucket(algo, side):
    """P = 8, pipe_grid = 24 over buckets of 8, 24, 16 and 40 tiles: a stride of 24 tiles passes the
    8-tile bucket and, later, the 16-tile one."""
    all_gather_in_place(algo, side, 8, 24)


# ------------------------------------------------------------------ 2. all-gather from shards
@grids
@layouts
@sched
def test_all_gather_from_shards(algo, side, total, layout, grid):
    """Every row, rank b's included, receives the shard's block b; the shard buffers are only read."""
    buckets = unequal(algo, side, total, oracle_too=False)
    shards = Shards(buckets, layout)
    src = source_blocks(buckets)
    shards.fill(src)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.shards_launches(shards.args(), AG) == 1
        plan.all_gather_shards(shards.args(), stream())
        check_buckets(buckets, [b.after_all_gather(s) for b, s in zip(buckets, src)], "block b of every row = the shard's block b")
        shards.check(shards.host, "an all-gather wrote its shard")
    if grid == 0:
        want = [per_bucket_all_gather(algo, side, b, shards.arg(i)[3:]) for i, b in enumerate(buckets)]
        check_buckets(buckets, want, "the per-bucket Plan.all_gather(in=...) bits")
    plan.close()


# ------------------------------------------------------------------ 3. reduce-scatter into shards
@grids
@layouts
@sched
def test_reduce_scatter_into_shards(algo, side, total, layout, grid):
    """The shard blocks = the oracle's block b; gaps and guards stay sentinel; every rank buffer —
    rows, skew, guard row — is wholly unchanged."""
    buckets = unequal(algo, side, total)
    shards = Shards(buckets, layout)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.shards_launches(shards.args(), RS) == 1
        plan.reduce_scatter_shards(shards.args(), stream())
        shards.check(shards.after_reduce_scatter(), "block b = tree b, nothing else written")
        check_buckets(buckets, [b.host for b in buckets], "a reduce-scatter into a shard wrote its rank rows")
    plan.close()


@grids
@sched
def test_reduce_scatter_mixing_in_place_and_shards(algo, side, total, grid):
    """Buckets 0 and 2 into a flat buffer of their own, 1 and 3 in place, in one launch."""
    buckets = unequal(algo, side, total)
    with_shard = {0, 2}
    shards = Shards(buckets, "flat")
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        args = shards.args(only=with_shard)
        assert plan.shards_launches(args, RS) == 1
        plan.reduce_scatter_shards(args, stream())
        shards.check(shards.after_reduce_scatter(only=with_shard), "only the buckets with a shard go there")
        check_buckets(buckets, [b.host if i in with_shard else b.after_reduce_scatter() for i, b in enumerate(buckets)],
                      "in place: block b to rank b's row; with a shard: rows untouched")
    plan.close()


@sched
def test_reduce_scatter_without_shards_is_reduce_scatter_group(algo, side, total):
    buckets = unequal(algo, side, total)
    args = [b.arg for b in buckets]
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=5):
        plan.reduce_scatter_group(args, stream())
        group = [b.got() for b in buckets]
        for b in buckets:
            b.restore()
        plan.reduce_scatter_shards(args, stream())
        check_buckets(buckets, group, "not the bytes of reduce_scatter_group")
        check_buckets(buckets, [b.after_reduce_scatter() for b in buckets], "not the oracle's blocks")
    plan.close()


# ------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("through", ["in-place", "flat"])
@sched
def test_reduce_scatter_then_all_gather_is_execute_group(algo, side, total, through):
    buckets = unequal(algo, side, total)
    plan = any_plan(algo, side, total)
    plan.execute_group([b.arg for b in buckets], stream())
    whole = [b.got() for b in buckets]
    for b in buckets:
        b.restore()
    shards = Shards(buckets, "flat")
    args = shards.args() if through == "flat" else [b.arg for b in buckets]
    with t.tuned(pipe_grid=5):
        plan.reduce_scatter_shards(args, stream())
        plan.all_gather_shards(args, stream())
    check_buckets(buckets, whole, "not the bits of execute_group")
    check_buckets(buckets, [b.after_allreduce() for b in buckets], "not the oracle's allreduce")
    if through == "flat":
        shards.check(shards.after_reduce_scatter(), "the shards hold the reduced blocks")
    plan.close()


# ------------------------------------------------------------------ 5. arbitrary bits
@pytest.mark.parametrize("through", ["in-place", "compact"])
def test_arbitrary_bit_patterns_come_out_as_copied(through):
    """NaN payloads, infinities and denormals: all 16 bits of every element are copied."""
    algo, side, total = t.SWING, 4, 16
    rng = np.random.default_rng(5)
    buckets = [Bucket(rng.integers(0, 0x10000, (total, 256 * total * k)).astype(np.uint16)) for k in UNEQUAL]
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=5):
        if through == "in-place":
            plan.all_gather_shards([b.arg for b in buckets], stream())
            check_buckets(buckets, [b.after_all_gather() for b in buckets], "bits changed on the way")
        else:
            shards = Shards(buckets, "compact")
            src = [rng.integers(0, 0x10000, (total, b.blk)).astype(np.uint16) for b in buckets]
            shards.fill(src)
            plan.all_gather_shards(shards.args(), stream())
            check_buckets(buckets, [b.after_all_gather(s) for b, s in zip(buckets, src)], "bits changed on the way")
            shards.check(shards.host, "an all-gather wrote its shard")
    plan.close()


# ------------------------------------------------------------------ 6. bucket counts and routes
@pytest.mark.parametrize("count,launches", [(_lib.GROUP_MAX, 1), (_lib.GROUP_MAX + 1, 2)])
def test_64_buckets_in_one_launch_65_in_two(count, launches):
    """One-tile-per-block buckets into one flat shard buffer and back."""
    algo, side, total = t.SWING, 4, 8
    buckets = [make(algo, side, total, 256 * total, salt=i) for i in range(count)]
    shards = Shards(buckets, "flat")
    plan = any_plan(algo, side, total)
    assert plan.shards_launches(shards.args(), RS) == launches
    assert plan.shards_launches(shards.args(), AG) == launches
    plan.reduce_scatter_shards(shards.args(), stream())
    shards.check(shards.after_reduce_scatter(), "block b = tree b")
    check_buckets(buckets, [b.host for b in buckets], "rank rows written")
    plan.all_gather_shards(shards.args(), stream())
    check_buckets(buckets, [b.after_allreduce() for b in buckets], "not the oracle's allreduce")
    plan.close()


@pytest.mark.parametrize("op", [RS, AG], ids=["reduce-scatter", "all-gather"])
def test_mixed_routes(op):
    """8x8 Swing: a bucket that is not whole tiles (the register form / k_ag) and one of 1280 tiles
    (the persistent 64-rank route) keep their own launches; the two small whole-tile buckets
    around them share ONE grouped launch.  All four with shards; fused_form 2 turns grouping off."""
    algo, side, total = t.SWING, 8, 64
    sizes = [256 * total, 8 * total * 3, 256 * total * 20, 256 * total * 2]
    buckets = [make(algo, side, total, n, salt=i, oracle_too=op == RS) for i, n in enumerate(sizes)]
    shards = Shards(buckets, "compact")
    src = source_blocks(buckets)
    plan = any_plan(algo, side, total)

    def run_and_check():
        if op == RS:
            plan.reduce_scatter_shards(shards.args(), stream())
            shards.check(shards.after_reduce_scatter(), "block b = tree b")
            check_buckets(buckets, [b.host for b in buckets], "rank rows written")
        else:
            plan.all_gather_shards(shards.args(), stream())
            check_buckets(buckets, [b.after_all_gather(s) for b, s in zip(buckets, src)], "block b of every row = the shard's")
            shards.check(shards.host, "an all-gather wrote its shard")

    if op == AG:
        shards.fill(src)
    alone = 1 + 1   # the per-bucket routes of buckets 1 and 2: one launch each, for either op
    assert plan.shards_launches(shards.args(), op) == alone + 1
    run_and_check()
    with t.tuned(fused_form=2):   # grouping off: every bucket its own launch, the same bits
        assert plan.shards_launches(shards.args(), op) == len(buckets)
        for b in buckets:
            b.restore()
        shards.restore()
        run_and_check()
    plan.close()


# ------------------------------------------------------------------ 7. graph capture
@pytest.mark.parametrize("op", [RS, AG], ids=["reduce-scatter", "all-gather"])
def test_graph_capture_replays_the_eager_bits(op):
    """Both tables travel in the kernel arguments, so the calls can be captured: one capture on one
    stream (a single linear branch), one replay on restored data."""
    algo, side, total = t.SWING, 4, 16
    buckets = unequal(algo, side, total, oracle_too=op == RS)
    shards = Shards(buckets, "flat")
    if op == AG:
        shards.fill(source_blocks(buckets))
    args = shards.args()
    plan = any_plan(algo, side, total)
    call = plan.reduce_scatter_shards if op == RS else plan.all_gather_shards
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call(args, s)
    s.synchronize()
    eager = [b.got() for b in buckets], shards.got()
    for b in buckets:
        b.restore()
    shards.restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(args, s)
    torch.cuda.synchronize()
    check_buckets(buckets, [b.host for b in buckets], "a capture runs nothing")
    shards.check(shards.host, "a capture runs nothing")
    g.replay()
    torch.cuda.synchronize()
    check_buckets(buckets, eager[0], "the replay differs from the eager call")
    shards.check(eager[1], "the replay differs from the eager call")
    if op == RS:
        shards.check(shards.after_reduce_scatter(), "block b = tree b")
    del g
    plan.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_every_buffer_untouched():
    algo, side, total = t.SWING, 4, 8
    buckets = unequal(algo, side, total, oracle_too=False)
    shards = Shards(buckets, "compact")
    args = shards.args()
    s = stream()

    def refused(status, call):
        with pytest.raises(t.AllredError) as e:
            call()
        assert e.value.status == status, (e.value.status, status)

    def refused_everywhere(status, plan, lst):
        refused(status, lambda: plan.reduce_scatter_shards(lst, s))
        refused(status, lambda: plan.all_gather_shards(lst, s))
        refused(status, lambda: plan.shards_launches(lst, RS))
        refused(status, lambda: plan.shards_launches(lst, AG))

    others = [any_plan(algo, side, total, variant=t.LO), any_plan(algo, side, total, variant=t.MEM),
              any_plan(algo, side, total, exec_mode=t.EXEC_STEPS)]
    for plan in others:
        refused_everywhere(_lib.ERR_UNSUPPORTED, plan, args)
        refused_everywhere(_lib.ERR_UNSUPPORTED, plan, [b.arg for b in buckets])
        plan.close()
    plan = any_plan(algo, side, total)
    ptr, stride, n, shard, shard_stride = args[1]
    blk = n // total
    rest = args[:1] + args[2:]
    bad_lists = [
        # the per-bucket refusals of the grouped calls
        args + [(ptr + 2 * stride, stride, n)],                   # inside bucket 1's rows
        args[:1] + [(ptr, stride, n)] + args[1:],                 # the same bucket twice
        rest + [(ptr, stride, n + 8 * total - 8, shard, shard_stride)],   # n % (8 P) != 0, last in the list
        rest + [(ptr, n - 8, n, shard, shard_stride)],            # stride < n
        rest + [(ptr, stride + 4, n, shard, shard_stride)],       # stride % 8 != 0
        rest + [(ptr + 2, stride, n, shard, shard_stride)],       # not 16-byte aligned
        rest + [(0, stride, n, shard, shard_stride)],             # a null bucket
        rest + [(ptr, stride, 0, shard, shard_stride)],           # an empty bucket
        # the shard's own
        rest + [(ptr, stride, n, shard, blk - 8)],                # shard_stride < blk
        rest + [(ptr, stride, n, shard, blk + 4)],                # shard_stride % 8 != 0
        rest + [(ptr, stride, n, shard + 2, shard_stride)],       # a shard off by 2 bytes
        rest + [(ptr, stride, n, args[2][0] + 2 * args[2][1], blk)],   # a shard block inside bucket 2's rows
        rest + [(ptr, stride, n, args[2][0] + 2 * args[2][2], blk)],   # ... starting in the skew of its row 0
        rest + [(ptr, stride, n, args[2][3], shard_stride)],      # the same shard twice
        rest + [(ptr, stride, n, shard, 1 << 62)],                # address arithmetic that would overflow
    ]
    for bad in bad_lists:
        refused_everywhere(_lib.ERR_ARG, plan, bad)
    for op in (2, -1):
        refused(_lib.ERR_ARG, lambda: plan.shards_launches(args, op))
        refused(_lib.ERR_ARG, lambda: plan.shards_launches([], op))
    arr = (_lib.ShardBucket * len(args))(*args)
    lib = _lib.lib
    for call in (lib.allred_plan_reduce_scatter_shards, lib.allred_plan_all_gather_shards):
        assert call(plan._h, arr, -1, None) == _lib.ERR_ARG
        assert call(plan._h, None, 2, None) == _lib.ERR_ARG
        assert call(None, arr, len(args), None) == _lib.ERR_ARG
        assert call(plan._h, None, 0, None) == _lib.OK
    for op in (RS, AG):
        assert lib.allred_plan_shards_launches(plan._h, arr, -1, op) == _lib.ERR_ARG
        assert lib.allred_plan_shards_launches(plan._h, None, 2, op) == _lib.ERR_ARG
        assert lib.allred_plan_shards_launches(plan._h, None, 0, op) == 0
    # count == 0: OK, nothing launched
    plan.reduce_scatter_shards([], s)
    plan.all_gather_shards([], s)
    assert plan.shards_launches([], RS) == 0 and plan.shards_launches([], AG) == 0
    plan.close()
    check_buckets(buckets, [b.host for b in buckets], "written by a refused call")
    shards.check(shards.host, "written by a refused call")
