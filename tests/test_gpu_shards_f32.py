"""The grouped calls on fp32 shards (allred_plan_reduce_scatter_shards_f32,
allred_plan_all_gather_shards_f32, allred_plan_shards_f32_launches; k_tree_group_f32,
k_ag_group_f32).

Expectations come from tests/f32_tree.py (numpy float32: the tree of block b in tree_order[b]
order with no intermediate rounding, one multiply by scale, one add of the old value; bf16_rne
by the integer rule) and are compared BIT FOR BIT — fp32 as uint32, NaNs by class.  The inputs
are hard_inputs.cancel, on which the order of an fp32 tree shows in most columns
(tests/test_f32_tree.py), so one tree for all blocks, or natural rank order, fails here.

Every bucket is a buffer of its own — its rows at its stride, the stride skew and one guard row
behind the last rank filled with a sentinel — and every fp32 shard buffer is filled with a
sentinel bit pattern with a guard behind it; WHOLE buffers are compared, so a stray write
anywhere fails.  Shard layouts: compact (shard_stride = blk), wide (blk + 64, the gaps
sentinel) and flat — ONE rank-major buffer of `total` rows of F = sum of blk floats shared by
all buckets, bucket i's shard at column off_i with shard_stride = F.

Shapes: unequal buckets of (1, 3, 2, 5) tiles per block (a tile is 256 elements of every rank),
strides preferred_rank_stride(n) and n in turn, at the default grid and at pipe_grid 5, where
workgroups cross bucket and block ends mid-walk with the next tile's loads in flight."""
import functools

import numpy as np
import pytest

import f32_tree
import far_arena
import hard_inputs
import route_cases
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT16 = 0xA5A5
SENT32 = 0xA5A5A5A5       # a small negative float: finite, so a read of it would go unnoticed but a write of it cannot happen
GUARD = 64                # sentinel floats behind a shard buffer
RS, AG = _lib.OP_REDUCE_SCATTER, _lib.OP_ALL_GATHER

SCHEDULES = [(algo, route_cases.SIDE[total], total) for total in (8, 16, 32, 64) for algo in (t.SWING, t.RECDUB)]
SCHEDULES.append((t.SWING_1D, 1, 8))
sched = pytest.mark.parametrize("algo,side,total", SCHEDULES, ids=[f"algo{a}-{s}x{p}" for a, s, p in SCHEDULES])
grids = pytest.mark.parametrize("grid", [0, 5], ids=["default-grid", "grid5"])
layouts = pytest.mark.parametrize("layout", ["compact", "wide", "flat"])
UNEQUAL = (1, 3, 2, 5)   # tiles per block of the unequal list


@functools.lru_cache(maxsize=None)
def tree_order(algo, side, total):
    return tuple(tuple(row) for row in t.schedule(algo, side, total)["tree_order"])


@functools.lru_cache(maxsize=None)
def inputs(kind, total, n, seed):
    data = getattr(hard_inputs, kind)(total, n, seed)
    data.flags.writeable = False
    return data


@functools.lru_cache(maxsize=None)
def sums(kind, algo, side, total, n, seed):
    """(inputs, their per-block fp32 tree sums (total, blk)), computed once and read-only"""
    data = inputs(kind, total, n, seed)
    s = f32_tree.tree_sums(data, tree_order(algo, side, total))
    s.flags.writeable = False
    return data, s


def to_dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV)


def to_dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def stream():
    return torch.cuda.current_stream()


class Bucket:
    """One bucket in a device buffer of its own: (total + 1) rows of `stride` bf16 elements, the
    skew and the guard row = SENT16.  sums: the fp32 tree sums of its blocks, or None."""

    def __init__(self, data, sums=None, stride=None):
        self.total, self.n = data.shape
        self.blk = self.n // self.total
        self.sums = sums
        self.stride = stride or t.preferred_rank_stride(self.n)
        self.host = np.full((self.total + 1, self.stride), SENT16, dtype=np.uint16)
        self.host[:self.total, :self.n] = data
        self.buf = to_dev16(self.host)
        self.arg = (self.buf.data_ptr(), self.stride, self.n)

    def restore(self):
        self.buf.copy_(to_dev16(self.host))

    def got(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(np.uint16)

    def after_all_gather(self, blocks16):
        """block b of every row = blocks16[b]"""
        e = self.host.copy()
        for b in range(self.total):
            e[:self.total, b * self.blk:(b + 1) * self.blk] = blocks16[b]
        return e


class Shards:
    """The fp32 shard buffers of a bucket list in one layout, as uint32 bit patterns, SENT32-filled,
    a guard behind each: compact / wide: one buffer per bucket; flat: one rank-major buffer."""

    def __init__(self, buckets, layout):
        self.buckets = buckets
        total = buckets[0].total
        self.where = []    # per bucket: (buffer, offset, stride), floats
        self.host = []
        if layout == "flat":
            F = sum(b.blk for b in buckets)
            self.host.append(np.full((total + 1) * F, SENT32, dtype=np.uint32))   # the last row: the guard
            off = 0
            for b in buckets:
                self.where.append((0, off, F))
                off += b.blk
        else:
            for i, b in enumerate(buckets):
                stride = b.blk + (64 if layout == "wide" else 0)
                self.host.append(np.full(total * stride + GUARD, SENT32, dtype=np.uint32))
                self.where.append((i, 0, stride))
        self.buf = [to_dev32(h) for h in self.host]

    def arg(self, i):
        k, off, stride = self.where[i]
        return self.buckets[i].arg + (self.buf[k].data_ptr() + 4 * off, stride)

    def args(self):
        return [self.arg(i) for i in range(len(self.buckets))]

    def slot(self, i, b):
        k, off, stride = self.where[i]
        return k, slice(off + b * stride, off + b * stride + self.buckets[i].blk)

    def fill(self, blocks):
        """blocks[i]: (total, blk) float32 or uint32, bucket i's blocks, into the host mirror and the device"""
        for i, bk in enumerate(self.buckets):
            for b in range(bk.total):
                k, s = self.slot(i, b)
                self.host[k][s] = np.ascontiguousarray(blocks[i][b]).view(np.uint32)
        self.restore()

    def blocks(self, i, src=None):
        """(total, blk) float32: bucket i's blocks as the host mirror (or `src`, e.g. got()) holds them"""
        src = self.host if src is None else src
        out = []
        for b in range(self.buckets[i].total):
            k, s = self.slot(i, b)
            out.append(src[k][s])
        return np.stack(out).view(np.float32)

    def restore(self):
        for d, h in zip(self.buf, self.host):
            d.copy_(to_dev32(h))

    def got(self):
        torch.cuda.synchronize()
        return [d.cpu().numpy().view(np.uint32) for d in self.buf]

    def expected(self, values):
        """the host mirror with bucket i's blocks = values[i] ((total, blk) float32)"""
        e = [h.copy() for h in self.host]
        for i, bk in enumerate(self.buckets):
            for b in range(bk.total):
                k, s = self.slot(i, b)
                e[k][s] = np.ascontiguousarray(values[i][b]).view(np.uint32)
        return e

    def check(self, expected, what):
        for k, (g, e) in enumerate(zip(self.got(), expected)):
            assert f32_tree.same_f32(g.view(np.float32), e.view(np.float32)), f"shard buffer {k}: {what}"


def unequal(algo, side, total, kind="cancel", seed=0):
    """[256 P, 256 P 3, 256 P 2, 256 P 5] elements per rank; strides preferred_rank_stride(n) and n in turn"""
    out = []
    for i, k in enumerate(UNEQUAL):
        n = 256 * total * k
        data, s = sums(kind, algo, side, total, n, 100 * seed + i)
        out.append(Bucket(data, s, None if i % 2 == 0 else n))
    return out


def any_plan(algo, side, total, exec_mode=t.EXEC_FUSED, variant=t.BO):
    """a plan for its schedule: its own bucket size (one tile per block) is not the lists'"""
    return t.Plan(algo, variant, side, 256 * total, total, exec_mode)


def check_buckets(buckets, expected, what, by_class=False):
    for i, (b, e) in enumerate(zip(buckets, expected)):
        got = b.got()
        assert f32_tree.same_bf16(got, e) if by_class else np.array_equal(got, e), f"bucket {i} (n={b.n}): {what}"


def random_floats(rng, shape, lo_exp=100, hi_exp=160):
    """finite float32 of both signs, magnitudes 2^(lo_exp - 127) .. 2^(hi_exp - 126): beyond 2^24 included"""
    bits = (rng.integers(0, 2, shape, dtype=np.uint32) << 31) | (rng.integers(lo_exp, hi_exp, shape, dtype=np.uint32) << 23) \
        | rng.integers(0, 1 << 23, shape, dtype=np.uint32)
    return bits.view(np.float32)


# ------------------------------------------------------------------ 1. reduce-scatter
@grids
@layouts
@sched
def test_reduce_scatter_is_the_fp32_tree_times_scale(algo, side, total, layout, grid):
    """Block b = tree b in fp32, times scale, for scale 1, 1 / P and 0.1f; gaps and guards keep the
    sentinel; every rank buffer — rows, skew, guard row — is wholly unchanged."""
    buckets = unequal(algo, side, total)
    shards = Shards(buckets, layout)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.shards_f32_launches(shards.args(), RS) == 1
        for scale in (1.0, 1.0 / total, 0.1):
            shards.restore()
            with t.launch_trace() as tr:
                plan.reduce_scatter_shards_f32(shards.args(), scale, stream=stream())
            assert tr.kernels == [f"k_tree_group_f32<{total}, false>"]
            shards.check(shards.expected([f32_tree.scaled(b.sums, scale) for b in buckets]),
                         f"scale {scale}: block b = fp32 tree b x scale, nothing else written")
        check_buckets(buckets, [b.host for b in buckets], "a reduce-scatter into fp32 shards wrote its rank rows")
    plan.close()


# ------------------------------------------------------------------ 2. accumulate
@grids
@sched
def test_accumulate_adds_into_the_shard(algo, side, total, grid):
    """One call: old + v; a second call on another gradient list: (old + v1) + v2 — each a separate
    fp32 add of a separately rounded product.  Without the flag the shard is not read: a NaN-filled
    shard comes out NaN-free."""
    first, second = unequal(algo, side, total, seed=1), unequal(algo, side, total, seed=2)
    shards = Shards(first, "flat")
    rng = np.random.default_rng(total + grid)
    old = [random_floats(rng, (total, b.blk)) for b in first]
    assert any((np.abs(o) > 2.0 ** 24).any() for o in old)
    shards.fill(old)
    scale = 1.0 / total
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        with t.launch_trace() as tr:
            plan.reduce_scatter_shards_f32(shards.args(), scale, accumulate=True, stream=stream())
        assert tr.kernels == [f"k_tree_group_f32<{total}, true>"]
        once = [f32_tree.scaled(b.sums, scale, o) for b, o in zip(first, old)]
        shards.check(shards.expected(once), "old + v")
        # the second gradient list: the same shard buffers, other rank rows
        args2 = [b.arg + a[3:] for b, a in zip(second, shards.args())]
        plan.reduce_scatter_shards_f32(args2, scale, accumulate=True, stream=stream())
        twice = [f32_tree.scaled(b.sums, scale, o) for b, o in zip(second, once)]
        shards.check(shards.expected(twice), "(old + v1) + v2")
        check_buckets(first + second, [b.host for b in first + second], "rank rows written")
        # no flag: the shard is never read
        shards.fill([np.full((total, b.blk), 0x7FC00000, dtype=np.uint32) for b in first])
        plan.reduce_scatter_shards_f32(shards.args(), scale, stream=stream())
        assert not any(f32_tree.is_nan32(shards.blocks(i, shards.got())).any() for i in range(len(first)))
        shards.check(shards.expected([f32_tree.scaled(b.sums, scale) for b in first]), "v over a NaN-filled shard")
    plan.close()


# ------------------------------------------------------------------ 3. non-finite values, known answers
@sched
def test_nonfinite_columns_come_out_by_class(algo, side, total):
    buckets = unequal(algo, side, total, kind="nonfinite", seed=3)
    shards = Shards(buckets, "compact")
    plan = any_plan(algo, side, total)
    classes = {"nan": None, "inf_minus_inf": None, "pos_inf": 0x7F800000, "overflow": 0x7F800000, "neg_inf": 0xFF800000}
    with t.tuned(pipe_grid=5):
        plan.reduce_scatter_shards_f32(shards.args(), 1.0, stream=stream())
        shards.check(shards.expected([b.sums for b in buckets]), "bit-equal outside NaNs, NaN where the tree is")
        got = shards.got()
        for i, b in enumerate(buckets):
            blocks = shards.blocks(i, got).view(np.uint32)
            cols = hard_inputs.nonfinite_columns(total, b.n)
            assert len(cols) == 15
            for c, cls in cols:
                bits = int(blocks[c // b.blk, c % b.blk])   # the owner's block
                if classes[cls] is None:
                    assert (bits & 0x7FFFFFFF) > 0x7F800000, f"bucket {i} column {c} ({cls}): 0x{bits:08X} is no NaN"
                else:
                    assert bits == classes[cls], f"bucket {i} column {c} ({cls}): 0x{bits:08X}"
    plan.close()


@sched
def test_soft_data_gives_the_exact_sum(algo, side, total):
    """a known answer that needs no tree: on [1, 100) data every fp32 order is the float64 sum"""
    buckets = unequal(algo, side, total, kind="soft", seed=4)
    shards = Shards(buckets, "wide")
    plan = any_plan(algo, side, total)
    plan.reduce_scatter_shards_f32(shards.args(), stream=stream())
    got = shards.got()
    for i, b in enumerate(buckets):
        data = b.host[:total, :b.n]
        exact = f32_tree.widen(data).astype(np.float64).sum(axis=0).reshape(total, b.blk)
        assert np.array_equal(shards.blocks(i, got).astype(np.float64), exact), f"bucket {i}"
    plan.close()


# ------------------------------------------------------------------ 4. all-gather
PLANTED = {   # fp32 bits -> the bf16 they must become (None: a NaN)
    0x3F808000: 0x3F80, 0x3F818000: 0x3F82,                    # ties, to even both ways
    0x3F807FFF: 0x3F80, 0x3F808001: 0x3F81, 0x3F817FFF: 0x3F81, 0x3F818001: 0x3F82,   # one ulp either side of a tie
    0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80,                    # above the largest finite bf16: Inf
    0x00000000: 0x0000, 0x80000000: 0x8000,                    # signed zeros
    0x00018000: 0x0002, 0x00008000: 0x0000, 0x00000001: 0x0000, 0x807FFFFF: 0x8080, 0x00010000: 0x0001,   # denormals
    0x7F800000: 0x7F80, 0xFF800000: 0xFF80,                    # infinities
    0x7FC00001: None, 0xFFFFFFFF: None, 0x7F800001: None,      # NaNs, one whose payload lies below bit 16
}


def planted_blocks(rng, total, blk):
    """(total, blk) uint32: random bit patterns; the planted values in the first and the last vectors of
    every block, hence on both sides of every block boundary of the rank row"""
    bits = rng.integers(0, 1 << 32, (total, blk), dtype=np.uint64).astype(np.uint32)
    vals = np.array(list(PLANTED), dtype=np.uint32)
    bits[:, :len(vals)] = vals
    bits[:, blk - len(vals):] = vals[::-1]
    return bits


@grids
@layouts
@sched
def test_all_gather_rounds_once_to_bf16(algo, side, total, layout, grid):
    """Every row's block b, row b included, = bf16_rne(shard block b); the shards are bit-unchanged;
    nothing past n is written."""
    buckets = [Bucket(inputs("soft", total, 256 * total * k, 5), None, None if i % 2 == 0 else 256 * total * k)
               for i, k in enumerate(UNEQUAL)]
    shards = Shards(buckets, layout)
    rng = np.random.default_rng(7 * total)
    src = [planted_blocks(rng, total, b.blk) for b in buckets]
    shards.fill(src)
    want = [f32_tree.bf16_rne(s.view(np.float32)) for s in src]
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.shards_f32_launches(shards.args(), AG) == 1
        with t.launch_trace() as tr:
            plan.all_gather_shards_f32(shards.args(), stream())
        assert tr.kernels == [f"k_ag_group_f32<{total}>"]
        check_buckets(buckets, [b.after_all_gather(w) for b, w in zip(buckets, want)], "block b of every row = bf16_rne(shard)",
                      by_class=True)
        for g, h in zip(shards.got(), shards.host):
            assert np.array_equal(g, h), "an all-gather wrote its shard"
    # the planted values as known answers, in rank 0's row and in the owner's
    got = buckets[0].got()
    blk = buckets[0].blk
    for r in (0, total - 1):
        for b in (0, total // 2, total - 1):
            for j, (bits, bf) in enumerate(PLANTED.items()):
                for col in (b * blk + j, (b + 1) * blk - 1 - j):
                    g = int(got[r, col])
                    assert (g & 0x7FFF) > 0x7F80 if bf is None else g == bf, f"0x{bits:08X} -> 0x{g:04X} (row {r}, column {col})"
    plan.close()


@sched
def test_round_trip_leaves_the_rounded_tree_in_every_rank(algo, side, total):
    buckets = unequal(algo, side, total, seed=6)
    shards = Shards(buckets, "flat")
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=5):
        plan.reduce_scatter_shards_f32(shards.args(), 1.0, stream=stream())
        plan.all_gather_shards_f32(shards.args(), stream())
    check_buckets(buckets, [b.after_all_gather(f32_tree.bf16_rne(b.sums)) for b in buckets],
                  "block b of every rank = bf16_rne(fp32 tree b)", by_class=True)
    plan.close()


# ------------------------------------------------------------------ 5. counts and routing
@pytest.mark.parametrize("count,launches", [(_lib.GROUP_MAX, 1), (_lib.GROUP_MAX + 1, 2)])
def test_64_buckets_in_one_launch_65_in_two(count, launches):
    algo, side, total = t.SWING, 4, 8
    buckets = []
    for i in range(count):
        data, s = sums("cancel", algo, side, total, 256 * total, 1000 + i)
        buckets.append(Bucket(data, s))
    shards = Shards(buckets, "flat")
    plan = any_plan(algo, side, total)
    for op, name, call in ((RS, f"k_tree_group_f32<{total}, false>", lambda: plan.reduce_scatter_shards_f32(shards.args(), 0.1, stream=stream())),
                           (AG, f"k_ag_group_f32<{total}>", lambda: plan.all_gather_shards_f32(shards.args(), stream()))):
        assert plan.shards_f32_launches(shards.args(), op) == launches
        with t.launch_trace() as tr:
            call()
        assert tr.count == launches and tr.kernels == [name] * launches
        if op == RS:
            values = [f32_tree.scaled(b.sums, 0.1) for b in buckets]
            shards.check(shards.expected(values), "block b = tree b x 0.1")
            check_buckets(buckets, [b.host for b in buckets], "rank rows written")
    check_buckets(buckets, [b.after_all_gather(f32_tree.bf16_rne(v)) for b, v in zip(buckets, values)], "bf16_rne(shard)")
    plan.close()


@pytest.mark.parametrize("accumulate", [False, True])
def test_a_large_64_rank_bucket_stays_in_the_grouped_kernel(accumulate):
    """1024 tiles, 16 per block, 64 ranks: the bf16 calls hand such a bucket to k_tree_lds_lag; there is
    no fp32 form of that kernel, so it takes the grouped kernel — one launch, the same bits."""
    algo, side, total = t.SWING, 8, 64
    data, s = sums("cancel", algo, side, total, 256 * total * 16, 77)
    b = Bucket(data, s)
    shards = Shards([b], "compact")
    old = None
    if accumulate:
        old = random_floats(np.random.default_rng(1), (total, b.blk))
        shards.fill([old])
    plan = any_plan(algo, side, total)
    assert plan.shards_f32_launches(shards.args(), RS) == 1 and plan.shards_f32_launches(shards.args(), AG) == 1
    with t.launch_trace() as tr:
        plan.reduce_scatter_shards_f32(shards.args(), 1.0 / 64, accumulate=accumulate, stream=stream())
        plan.all_gather_shards_f32(shards.args(), stream())
    assert tr.kernels == [f"k_tree_group_f32<64, {'true' if accumulate else 'false'}>", "k_ag_group_f32<64>"]
    value = f32_tree.scaled(s, 1.0 / 64, old)
    shards.check(shards.expected([value]), "block b = tree b / 64")
    check_buckets([b], [b.after_all_gather(f32_tree.bf16_rne(value))], "bf16_rne(shard)", by_class=True)
    plan.close()


# ------------------------------------------------------------------ 6. graph capture
@pytest.mark.parametrize("op,accumulate", [(RS, False), (RS, True), (AG, False)], ids=["reduce-scatter", "accumulate", "all-gather"])
def test_graph_capture_replays_the_eager_bits(op, accumulate):
    """Every table and the scale travel in the kernel arguments, so the calls can be captured: one
    capture on one stream (a single linear branch), one replay on restored data."""
    algo, side, total = t.SWING, 4, 16
    buckets = unequal(algo, side, total, seed=8)
    shards = Shards(buckets, "flat")
    rng = np.random.default_rng(2)
    if op == AG or accumulate:
        shards.fill([random_floats(rng, (total, b.blk)) for b in buckets])
    args = shards.args()
    plan = any_plan(algo, side, total)

    def call(s):
        if op == RS:
            plan.reduce_scatter_shards_f32(args, 0.1, accumulate=accumulate, stream=s)
        else:
            plan.all_gather_shards_f32(args, s)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call(s)
    s.synchronize()
    eager = [b.got() for b in buckets], shards.got()
    for b in buckets:
        b.restore()
    shards.restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(s)
    torch.cuda.synchronize()
    check_buckets(buckets, [b.host for b in buckets], "a capture runs nothing")
    for got, h in zip(shards.got(), shards.host):
        assert np.array_equal(got, h), "a capture runs nothing"
    g.replay()
    torch.cuda.synchronize()
    check_buckets(buckets, eager[0], "the replay differs from the eager call")
    for got, e in zip(shards.got(), eager[1]):
        assert np.array_equal(got, e), "the replay differs from the eager call"
    if op == RS:
        old = [shards.blocks(i) for i in range(len(buckets))] if accumulate else [None] * len(buckets)
        shards.check(shards.expected([f32_tree.scaled(b.sums, 0.1, o) for b, o in zip(buckets, old)]), "tree b x 0.1 (+ old)")
    del g
    plan.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_every_buffer_untouched():
    algo, side, total = t.SWING, 4, 8
    buckets = unequal(algo, side, total)
    shards = Shards(buckets, "compact")
    args = shards.args()
    s = stream()

    def refused(status, call):
        with pytest.raises(t.AllredError) as e:
            call()
        assert e.value.status == status, (e.value.status, status)

    def refused_everywhere(status, plan, lst):
        refused(status, lambda: plan.reduce_scatter_shards_f32(lst, 1.0, stream=s))
        refused(status, lambda: plan.reduce_scatter_shards_f32(lst, 0.5, accumulate=True, stream=s))
        refused(status, lambda: plan.all_gather_shards_f32(lst, s))
        refused(status, lambda: plan.shards_f32_launches(lst, RS))
        refused(status, lambda: plan.shards_f32_launches(lst, AG))

    others = [any_plan(algo, side, total, variant=t.LO), any_plan(algo, side, total, variant=t.MEM),
              any_plan(algo, side, total, exec_mode=t.EXEC_STEPS)]
    for plan in others:
        refused_everywhere(_lib.ERR_UNSUPPORTED, plan, args)
        plan.close()
    # a P = 4 plan: no kernel form below 8 ranks
    p4 = t.Plan(t.SWING, t.BO, 2, 256 * 4, 4, t.EXEC_FUSED)
    four = [(a[0], a[1], 256 * 4, a[3], 256) for a in args[:1]]
    refused_everywhere(_lib.ERR_UNSUPPORTED, p4, four)
    p4.close()
    plan = any_plan(algo, side, total)
    ptr, stride, n, shard, shard_stride = args[1]
    blk = n // total
    rest = args[:1] + args[2:]
    # a bucket that is not whole tiles: unsupported, for the whole list, wherever it stands
    part = (ptr, stride, 8 * total * 3, shard, 8 * 3)
    refused_everywhere(_lib.ERR_UNSUPPORTED, plan, rest + [part])
    refused_everywhere(_lib.ERR_UNSUPPORTED, plan, [part] + rest)
    bad_lists = [
        rest + [(ptr, stride, n, 0, shard_stride)],              # a NULL shard: there is no in-place form
        rest + [(ptr, stride, n, shard, blk - 4)],               # shard_stride < blk
        rest + [(ptr, stride, n, shard, blk + 2)],               # shard_stride % 4 != 0
        rest + [(ptr, stride, n, shard + 4, shard_stride)],      # a shard off by one float
        rest + [(ptr, stride, n, shard + 8, shard_stride)],      # ... by two: 8-byte aligned is not enough
        rest + [(ptr, stride, n, args[2][3] + 4 * (args[2][2] // total) - 16, blk)],   # on the last 16 bytes of a block of bucket 2's shard
        rest + [(ptr, stride, n, args[2][3], shard_stride)],     # the same shard twice
        rest + [(ptr, stride, n, args[2][0] + 2 * args[2][1], blk)],   # a shard block inside bucket 2's rows
        rest + [(ptr, stride, n, args[2][0] + 2 * args[2][2], blk)] if args[2][1] > args[2][2] else None,   # ... in its row 0's skew
        rest + [(ptr, stride, n, shard, 1 << 62)],               # address arithmetic that would overflow
        rest + [(ptr, stride, n, shard, 1 << 63)],               # ... in the doubling already
        # the per-bucket refusals of the grouped calls
        args + [(ptr + 2 * stride, stride, n, shard, shard_stride)],   # inside bucket 1's rows
        rest + [(ptr, n - 8, n, shard, shard_stride)],           # stride < n
        rest + [(ptr + 2, stride, n, shard, shard_stride)],      # rows not 16-byte aligned
        rest + [(0, stride, n, shard, shard_stride)],            # a null bucket
        rest + [(ptr, stride, 0, shard, shard_stride)],          # an empty bucket
    ]
    for bad in bad_lists:
        if bad is not None:
            refused_everywhere(_lib.ERR_ARG, plan, bad)
    arr = (_lib.ShardBucketF32 * len(args))(*[(a[0], a[1], a[2], a[3], a[4]) for a in args])
    lib = _lib.lib
    for flags in (2, 3, 0x100, -2):                              # an unknown flag bit
        assert lib.allred_plan_reduce_scatter_shards_f32(plan._h, arr, len(args), 1.0, flags, None) == _lib.ERR_ARG
    for op in (2, -1):                                           # a bad op
        refused(_lib.ERR_ARG, lambda: plan.shards_f32_launches(args, op))
        refused(_lib.ERR_ARG, lambda: plan.shards_f32_launches([], op))
    assert lib.allred_plan_reduce_scatter_shards_f32(plan._h, arr, -1, 1.0, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_reduce_scatter_shards_f32(plan._h, None, 2, 1.0, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_reduce_scatter_shards_f32(None, arr, len(args), 1.0, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_f32(plan._h, arr, -1, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_f32(plan._h, None, 2, None) == _lib.ERR_ARG
    # count == 0: OK, nothing launched
    with t.launch_trace() as tr:
        plan.reduce_scatter_shards_f32([], 1.0, stream=s)
        plan.reduce_scatter_shards_f32([], 1.0, accumulate=True, stream=s)
        plan.all_gather_shards_f32([], s)
        assert lib.allred_plan_reduce_scatter_shards_f32(plan._h, None, 0, 1.0, 0, None) == _lib.OK
    assert tr.count == 0
    assert plan.shards_f32_launches([], RS) == 0 and plan.shards_f32_launches([], AG) == 0
    # and the list itself is fine: the dry run accepts it without writing
    assert lib.allred_plan_shards_f32_launches(plan._h, arr, len(args), RS) == 1
    plan.close()
    check_buckets(buckets, [b.host for b in buckets], "written by a refused call")
    for got, h in zip(shards.got(), shards.host):
        assert np.array_equal(got, h), "a shard written by a refused call"


def test_a_non_finite_scale_is_the_callers_arithmetic():
    algo, side, total = t.SWING, 4, 8
    data, s = sums("soft", algo, side, total, 256 * total, 9)
    b = Bucket(data, s)
    shards = Shards([b], "compact")
    plan = any_plan(algo, side, total)
    plan.reduce_scatter_shards_f32(shards.args(), float("inf"), stream=stream())
    got = shards.blocks(0, shards.got()).view(np.uint32)
    assert (got == 0x7F800000).all()   # positive sums x +Inf
    plan.close()


# ------------------------------------------------------------------ 6. rows and shards beyond 2^32 elements
@pytest.fixture(scope="module")
def far():
    f = far_arena.F32Far(planes=1)   # an allocation failure is an error of the test, not a skip
    yield f
    f.close()


def far_args(far):
    """bucket i: its far rank rows, and its blocks of the flat fp32 buffer, F floats apart"""
    return [far.bucket(i) + (far.planes[i][0].ptr, far.stride_f32) for i in range(len(far.rows))]


def test_far_rows_and_a_far_flat_shard_buffer(far):
    """8x8 Swing, buckets of 1 and 3 tiles per block (tests/far_arena.py): the rank rows of the larger at the far
    bf16 stride (a list takes no two buckets whose row footprints meet), the shards blocks of ONE flat fp32 buffer of row stride F = roundup4(ceil(2^32 / 63)) + 64
    floats — 63 F is beyond 2^32 floats, middle blocks beyond 2^30 and 2^31.  The reduce-scatter, then
    the all-gather of what it stored: every payload row with 4 KiB of guard on both sides bit for bit,
    then the whole arena sentinel again.  `shard + b * shard_stride` or `ranks + r * stride` in 32 bits
    fails the compare (tests/test_far_layout.py)."""
    algo, side, total = t.SWING, 8, 64
    scale = 1.0 / total
    datas = [sums("cancel", algo, side, total, 256 * total * k, 300 + i) for i, k in enumerate(far_arena.F32_TILES)]
    for rows, (data, _) in zip(far.rows, datas):
        rows.upload(data)
    args = far_args(far)
    plan = any_plan(algo, side, total)
    try:
        with t.tuned(pipe_grid=5):
            with t.launch_trace() as tr:
                plan.reduce_scatter_shards_f32(args, scale, stream=stream())
            torch.cuda.synchronize()
            assert tr.kernels == [f"k_tree_group_f32<{total}, false>"]
            stored = [f32_tree.scaled(s, scale) for _, s in datas]
            for i, (data, _) in enumerate(datas):
                assert f32_tree.same_f32(far.planes[i][0].read().view(np.float32), stored[i]), f"bucket {i}: block b = fp32 tree b x scale"
                assert np.array_equal(far.rows[i].read(), data), f"bucket {i}: the rank rows are only read"
            with t.launch_trace() as tr:
                plan.all_gather_shards_f32(args, stream())
            torch.cuda.synchronize()
            assert tr.kernels == [f"k_ag_group_f32<{total}>"]
            for i, (data, _) in enumerate(datas):
                row = f32_tree.bf16_rne(stored[i]).reshape(-1)
                assert f32_tree.same_bf16(far.rows[i].read(), np.broadcast_to(row, data.shape)), f"bucket {i}: block b of every row"
                assert f32_tree.same_f32(far.planes[i][0].read().view(np.float32), stored[i]), f"bucket {i}: an all-gather wrote its shard"
    finally:
        plan.close()
        far.wipe()
    far.assert_sentinel()
