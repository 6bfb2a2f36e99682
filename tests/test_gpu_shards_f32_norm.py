"""allred_plan_reduce_scatter_shards_f32_norm / allred_plan_shards_f32_norm_workspace_bytes
(k_tree_group_f32_norm): the fp32 grouped reduce-scatter that also leaves the per-rank squared
norm of what it stored, in the same launch.

Expectations: the shards are tests/f32_tree.py's (and bit-equal to what
allred_plan_reduce_scatter_shards_f32 stores for the same arguments); norm_sq is
tests/f32_norm.py's over the stored values — the fixed order of allred.h — compared BIT FOR BIT,
NaNs by class.  The data come from tests/f32_norm_cases.py, and tests/test_f32_norm.py pins on the
CPU that they tell the stated order from a left-to-right tile sum, an fma chain, the c levels before
the q level and a sequential sum of the partials.

The buffers are tests/test_gpu_shards_f32.py's (whole buffers around sentinel guards).  norm_sq is
`total` floats between sentinel guards, pre-filled with NaN before every call; the workspace is
workspace_bytes between sentinel guards, its counter zeroed ONCE when it is made: after every call
the counter's 64 bytes must be zero again and every guard intact."""
import functools

import numpy as np
import pytest

import f32_norm
import f32_norm_cases as cases
import far_arena
import f32_tree
import tenstorrentallreduce_amd as t
import test_gpu_shards_f32 as base
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENT32 = base.SENT32
NAN32 = 0x7FC00000
GUARD = 64                # sentinel words on both sides of norm_sq and of the workspace (256 bytes: the pointers stay aligned)
RS = _lib.OP_REDUCE_SCATTER

sched = pytest.mark.parametrize("algo,side,total", cases.SCHEDULES, ids=cases.SCHEDULE_IDS)
grids = base.grids
layouts = base.layouts
stream = base.stream


def make_buckets(datas):
    """Bucket objects for [(data, sums)]: strides preferred_rank_stride(n) and n in turn"""
    return [base.Bucket(d, s, None if i % 2 == 0 else d.shape[1]) for i, (d, s) in enumerate(datas)]


class Norm:
    """norm_sq and the workspace of one list, each between guards"""

    def __init__(self, plan, args, total):
        self.total = total
        self.bytes = plan.shards_f32_norm_workspace_bytes(args)
        assert self.bytes == 64 + 4 * sum(a[2] // 256 for a in args)
        ws = np.full(2 * GUARD + self.bytes // 4, SENT32, dtype=np.uint32)
        ws[GUARD:GUARD + 16] = 0                                    # the caller zeroes the counter once
        self.ws = base.to_dev32(ws)
        self.sq_host = np.full(2 * GUARD + total, SENT32, dtype=np.uint32)
        self.sq_host[GUARD:GUARD + total] = NAN32
        self.sq = base.to_dev32(self.sq_host)
        self.sq_ptr = self.sq.data_ptr() + 4 * GUARD
        self.ws_ptr = self.ws.data_ptr() + 4 * GUARD
        assert self.ws_ptr % 16 == 0

    def prefill(self):
        """NaN into norm_sq: launch 0 overwrites, nothing of it may leak"""
        self.sq.copy_(base.to_dev32(self.sq_host))

    def got(self):
        torch.cuda.synchronize()
        return self.sq.cpu().numpy().view(np.uint32)[GUARD:GUARD + self.total].view(np.float32).copy()

    def check_untouched(self, what):
        torch.cuda.synchronize()
        assert np.array_equal(self.sq.cpu().numpy().view(np.uint32), self.sq_host), f"norm_sq written: {what}"

    def check(self, want, what):
        torch.cuda.synchronize()
        sq = self.sq.cpu().numpy().view(np.uint32)
        ws = self.ws.cpu().numpy().view(np.uint32)
        assert (sq[:GUARD] == SENT32).all() and (sq[GUARD + self.total:] == SENT32).all(), f"outside norm_sq's floats: {what}"
        assert (ws[:GUARD] == SENT32).all() and (ws[GUARD + self.bytes // 4:] == SENT32).all(), f"outside the workspace: {what}"
        assert (ws[GUARD:GUARD + 16] == 0).all(), f"the counter's 64 bytes are not zero after the call: {what}"
        got = sq[GUARD:GUARD + self.total].view(np.float32)
        assert f32_tree.same_f32(got, want), f"norm_sq: {what}\n got {got}\nwant {want}"


def call(plan, shards, norm, scale=1.0, accumulate=False, args=None, s=None):
    plan.reduce_scatter_shards_f32_norm(args or shards.args(), norm.sq_ptr, norm.ws_ptr, scale, accumulate=accumulate,
                                        stream=s or stream())


@functools.lru_cache(maxsize=None)
def want_unequal(algo, side, total, scale):
    values = cases.stored(cases.bucket_list(algo, side, total, cases.UNEQUAL), scale)
    return values, f32_norm.expect_norm_sq(values)


# ------------------------------------------------------------------ 1. the shards' bits, and the norm of them
@grids
@layouts
@sched
def test_norm_is_the_fixed_order_sum_of_the_stored_squares(algo, side, total, layout, grid):
    """(1, 3, 2, 5) tiles per block, hard_inputs.cancel, scale 1, 1 / P and 0.1f: the shard buffers equal, whole and
    bit for bit, what the existing call leaves; norm_sq is the stated order's; rank rows, guards, counter as they were."""
    datas = cases.bucket_list(algo, side, total, cases.UNEQUAL)
    buckets = make_buckets(datas)
    shards = base.Shards(buckets, layout)
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, shards.args(), total)
    with t.tuned(pipe_grid=grid):
        assert plan.shards_f32_launches(shards.args(), RS) == 1
        for scale in cases.SCALES(total):
            shards.restore()
            with t.launch_trace() as tr:
                plan.reduce_scatter_shards_f32(shards.args(), scale, stream=stream())
            assert tr.kernels == [f"k_tree_group_f32<{total}, false>"]   # the existing call's trace is what it was
            plain = shards.got()
            shards.restore()
            norm.prefill()
            with t.launch_trace() as tr:
                call(plan, shards, norm, scale)
            assert tr.kernels == [f"k_tree_group_f32_norm<{total}, false>"]
            for k, (g, e) in enumerate(zip(shards.got(), plain)):
                assert np.array_equal(g, e), f"shard buffer {k} differs from the existing call's (scale {scale})"
            values, want = want_unequal(algo, side, total, scale)
            shards.check(shards.expected(values), f"scale {scale}")
            norm.check(want, f"scale {scale}")
        base.check_buckets(buckets, [b.host for b in buckets], "the rank rows are only read")
    plan.close()


# ------------------------------------------------------------------ 2. accumulate: the norm follows the stored value
@grids
@sched
def test_accumulate_once_and_twice_norms_the_accumulated_value(algo, side, total, grid):
    first = cases.bucket_list(algo, side, total, cases.UNEQUAL, seed=1)
    second = cases.bucket_list(algo, side, total, cases.UNEQUAL, seed=2)
    b1, b2 = make_buckets(first), make_buckets(second)
    shards = base.Shards(b1, "flat")
    old = [cases.random_floats(np.random.default_rng(total), s.shape) for _, s in first]
    scale = 1.0 / total
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, shards.args(), total)
    with t.tuned(pipe_grid=grid):
        shards.fill(old)
        plan.reduce_scatter_shards_f32(shards.args(), scale, accumulate=True, stream=stream())
        plain = shards.got()
        shards.restore()
        with t.launch_trace() as tr:
            call(plan, shards, norm, scale, accumulate=True)
        assert tr.kernels == [f"k_tree_group_f32_norm<{total}, true>"]
        for g, e in zip(shards.got(), plain):
            assert np.array_equal(g, e), "the shards differ from the existing call's"
        once = cases.stored(first, scale, old)
        shards.check(shards.expected(once), "old + v1")
        norm.check(f32_norm.expect_norm_sq(once), "the norm of old + v1")
        # the second gradient list into the same shards: the norm of (old + v1) + v2
        args2 = [b.arg + a[3:] for b, a in zip(b2, shards.args())]
        norm.prefill()
        call(plan, shards, norm, scale, accumulate=True, args=args2)
        twice = cases.stored(second, scale, once)
        shards.check(shards.expected(twice), "(old + v1) + v2")
        norm.check(f32_norm.expect_norm_sq(twice), "the norm of (old + v1) + v2")
        base.check_buckets(b1 + b2, [b.host for b in b1 + b2], "rank rows written")
    plan.close()


# ------------------------------------------------------------------ 3. soft data: the float64 sum of squares
@sched
def test_soft_data_against_float64(algo, side, total):
    """Every term is non-negative, and a result passes one squaring and at most 2 + 6 + ceil(L / 64) + 6 + 1 adds:
    relative error <= (16 + ceil(L / 64)) 2^-24, times 1.01 for the second-order terms."""
    datas = cases.bucket_list(algo, side, total, cases.UNEQUAL, kind="soft", seed=4)
    buckets = make_buckets(datas)
    shards = base.Shards(buckets, "wide")
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, shards.args(), total)
    call(plan, shards, norm, 1.0 / total)
    values = cases.stored(datas, 1.0 / total)
    shards.check(shards.expected(values), "soft / P")
    norm.check(f32_norm.expect_norm_sq(values), "soft / P")
    got_shards = shards.got()
    stored64 = np.concatenate([shards.blocks(i, got_shards).astype(np.float64) for i in range(len(buckets))], axis=1)
    exact = (stored64 * stored64).sum(axis=1)
    L = sum(cases.UNEQUAL)
    bound = (16 + -(-L // 64)) * 2.0 ** -24 * 1.01
    err = np.abs(norm.got().astype(np.float64) - exact) / exact
    assert (err <= bound).all(), (err.max(), bound)
    plan.close()


# ------------------------------------------------------------------ 4. non-finite values: the owner's entry only
@pytest.mark.parametrize("algo,side,total", [cases.SCHEDULES[0], cases.SCHEDULES[6]], ids=["8", "64"])
def test_nonfinite_values_show_in_their_rank_only(algo, side, total):
    datas = cases.bucket_list(algo, side, total, cases.UNEQUAL, seed=3)
    buckets = make_buckets(datas)
    shards = base.Shards(buckets, "compact")
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, shards.args(), total)
    rng = np.random.default_rng(9)
    clean_old = [cases.random_floats(rng, s.shape, 120, 135) for _, s in datas]
    clean = f32_norm.expect_norm_sq(cases.stored(datas, 0.1, clean_old))
    owner = total - 3
    for planted, is_class in ((0x7FC00000, np.isnan), (0x7F800000, np.isposinf), (0xFF800000, np.isposinf)):
        old = [o.copy() for o in clean_old]
        old[1].view(np.uint32)[owner, 300] = planted       # bucket 1 has 3 tiles per block: the second tile of block `owner`
        shards.fill(old)
        norm.prefill()
        with t.tuned(pipe_grid=5):
            call(plan, shards, norm, 0.1, accumulate=True)
        values = cases.stored(datas, 0.1, old)
        shards.check(shards.expected(values), f"planted 0x{planted:08X}")
        want = f32_norm.expect_norm_sq(values)
        norm.check(want, f"planted 0x{planted:08X}")
        got = norm.got()
        assert is_class(got[owner]), got[owner]
        keep = np.arange(total) != owner
        assert np.isfinite(got[keep]).all() and np.array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))
    plan.close()


# ------------------------------------------------------------------ 5. few tiles, many partials, many launches
@pytest.mark.parametrize("algo,side,total", [cases.SCHEDULES[0], cases.SCHEDULES[7]], ids=["8", "64"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_one_bucket_of_one_tile_per_block(algo, side, total, accumulate):
    """P tiles in all: a grid of P workgroups, one tile each, and one partial per rank"""
    datas = cases.bucket_list(algo, side, total, (1,), seed=7)
    buckets = make_buckets(datas)
    shards = base.Shards(buckets, "compact")
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, shards.args(), total)
    assert norm.bytes == 64 + 4 * total
    old = None
    if accumulate:
        old = [cases.random_floats(np.random.default_rng(3), s.shape, 120, 135) for _, s in datas]
        shards.fill(old)
    with t.launch_trace() as tr:
        call(plan, shards, norm, 0.1, accumulate=accumulate)
    assert tr.count == 1
    values = cases.stored(datas, 0.1, old)
    shards.check(shards.expected(values), "one tile per block")
    want = f32_norm.expect_norm_sq(values)
    assert np.array_equal(want.view(np.uint32), np.array([f32_norm.tile_partial(values[0][b]) for b in range(total)]).view(np.uint32))
    norm.check(want, "one partial per rank: the tile partial itself")
    plan.close()


@grids
def test_eighty_partials_per_rank_take_the_strided_sum(grid):
    total, tiles = cases.STRIDED
    algo, side = t.SWING, 4
    datas = cases.bucket_list(algo, side, total, tiles, seed=5)
    buckets = make_buckets(datas)
    shards = base.Shards(buckets, "flat")
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, shards.args(), total)
    with t.tuned(pipe_grid=grid):
        call(plan, shards, norm, 0.1)
    values = cases.stored(datas, 0.1)
    shards.check(shards.expected(values), "sixteen buckets of 5 tiles per block")
    norm.check(f32_norm.expect_norm_sq(values), "80 partials per rank: S[l] + S[l + 64], then the tree")
    plan.close()


@pytest.mark.parametrize("count", cases.CHAIN_COUNTS)
def test_the_chain_across_launches(count):
    """64 buckets: one launch; 65: two; 130: three.  Launch 0 overwrites the NaN-filled norm_sq, launch k adds its R."""
    algo, side, total = t.SWING, 4, 8
    datas = cases.bucket_list(algo, side, total, (1,) * count, seed=6)
    buckets = make_buckets(datas)
    shards = base.Shards(buckets, "flat")
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, shards.args(), total)
    launches = -(-count // _lib.GROUP_MAX)
    assert plan.shards_f32_launches(shards.args(), RS) == launches
    with t.launch_trace() as tr:
        call(plan, shards, norm, 0.1)
    assert tr.count == launches and tr.kernels == [f"k_tree_group_f32_norm<{total}, false>"] * launches
    values = cases.stored(datas, 0.1)
    shards.check(shards.expected(values), f"{count} buckets")
    norm.check(f32_norm.expect_norm_sq(values), f"{count} buckets: (R_0 + R_1) + R_2")
    plan.close()


# ------------------------------------------------------------------ 6. graph capture: the counter resets itself
@pytest.mark.parametrize("accumulate", [False, True])
def test_one_capture_three_replays_on_fresh_rows(accumulate):
    algo, side, total = t.SWING, 4, 16
    rounds = [cases.bucket_list(algo, side, total, cases.UNEQUAL, seed=10 + r) for r in range(3)]
    buckets = make_buckets(rounds[0])
    shards = base.Shards(buckets, "flat")
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, shards.args(), total)
    old = [cases.random_floats(np.random.default_rng(4), s.shape, 120, 135) for _, s in rounds[0]] if accumulate else None
    if accumulate:
        shards.fill(old)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call(plan, shards, norm, 0.1, accumulate=accumulate, s=s)   # an eager call first: nothing is loaded inside the capture
    s.synchronize()
    shards.restore()
    norm.prefill()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(plan, shards, norm, 0.1, accumulate=accumulate, s=s)
    torch.cuda.synchronize()
    norm.check_untouched("a capture runs nothing")
    for got, h in zip(shards.got(), shards.host):
        assert np.array_equal(got, h), "a capture runs nothing"
    for r, datas in enumerate(rounds):
        for b, (d, _) in zip(buckets, datas):             # fresh rows in the captured buffers
            b.host[:total, :b.n] = d
            b.restore()
        norm.prefill()
        torch.cuda.synchronize()
        g.replay()
        values = cases.stored(datas, 0.1, old)
        shards.check(shards.expected(values), f"replay {r}")
        norm.check(f32_norm.expect_norm_sq(values), f"replay {r}")
        if accumulate:
            old = values
    del g
    plan.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_write_nothing():
    algo, side, total = t.SWING, 4, 8
    datas = cases.bucket_list(algo, side, total, cases.UNEQUAL)
    buckets = make_buckets(datas)
    shards = base.Shards(buckets, "wide")
    args = shards.args()
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, args, total)
    sq, ws, nbytes = norm.sq_ptr, norm.ws_ptr, norm.bytes
    lib = _lib.lib
    arr = (_lib.ShardBucketF32 * len(args))(*[tuple(a) for a in args])

    def status(lst, sq_ptr, ws_ptr, flags=0, p=plan):
        a = (_lib.ShardBucketF32 * len(lst))(*[tuple(x) for x in lst]) if lst else None
        return lib.allred_plan_reduce_scatter_shards_f32_norm(p._h, a, len(lst), 0.5, flags, sq_ptr or None, ws_ptr or None, None)

    ranks, stride, n, shard, shard_stride = args[1]
    blk = n // total
    assert shard_stride > blk
    skewed = next(a for a in args + [None] if a is None or a[1] > a[2])   # a bucket whose rank stride has a skew
    assert skewed is not None, "no bucket of the list has a stride skew"
    skew = skewed[0] + 2 * skewed[2]                            # the first byte of its row 0's skew
    bad = {
        "norm_sq NULL": (0, ws), "norm_sq not 4-byte aligned": (sq + 2, ws),
        "norm_ws NULL": (sq, 0), "norm_ws 8-byte aligned only": (sq, ws + 8), "norm_ws 4-byte aligned only": (sq, ws + 4),
        "norm_sq on the workspace's last byte": (ws + nbytes - 4, ws), "norm_sq's last byte on the workspace's first": (ws - 4 * total + 4, ws),
        "norm_sq on the counter": (ws, ws), "the workspace's last byte on norm_sq's first": (sq, sq - nbytes + 16),
        "norm_sq on the last bytes of a rank row": (ranks + 2 * n - 4, ws), "norm_sq in a stride skew": (skew, ws),
        "norm_sq on the last bytes of a shard block": (shard + 4 * (3 * shard_stride + blk) - 4, ws),
        "norm_sq's last float on a shard block's first": (shard + 4 * shard_stride - 4 * total + 4, ws),
        "norm_ws on the last bytes of a rank row": (sq, ranks + 2 * n - 16), "norm_ws in a stride skew": (sq, skew),
        "norm_ws on the last bytes of a shard block": (sq, shard + 4 * (2 * shard_stride + blk) - 16),
        "norm_ws ending on a shard block's first bytes": (sq, shard + 4 * shard_stride - nbytes + 16),
    }
    for what, (a, b) in bad.items():
        assert status(args, a, b) == _lib.ERR_ARG, what
        assert status(args, a, b, _lib.SHARD_ACCUMULATE) == _lib.ERR_ARG, what
    # byte-exact: norm_sq in the gap of bucket 1's wide stride (64 floats behind every block), right behind a block
    assert status(args, shard + 4 * blk, ws) == _lib.OK
    gap_sq = shards.got()
    shards.restore()
    # the f32 call's checks apply unchanged
    assert status(args, sq, ws, flags=2) == _lib.ERR_ARG
    assert status(args[:1] + [(ranks, stride, n, 0, shard_stride)], sq, ws) == _lib.ERR_ARG               # a NULL shard
    assert status(args + [(ranks, stride, n, shard, shard_stride)], sq, ws) == _lib.ERR_ARG               # one bucket twice
    assert status(args[:1] + [(ranks, stride, 8 * total * 3, shard, 24)], sq, ws) == _lib.ERR_UNSUPPORTED  # not whole tiles
    assert lib.allred_plan_reduce_scatter_shards_f32_norm(None, arr, len(args), 1.0, 0, sq, ws, None) == _lib.ERR_ARG
    assert lib.allred_plan_reduce_scatter_shards_f32_norm(plan._h, arr, -1, 1.0, 0, sq, ws, None) == _lib.ERR_ARG
    assert lib.allred_plan_reduce_scatter_shards_f32_norm(plan._h, None, 2, 1.0, 0, sq, ws, None) == _lib.ERR_ARG
    for other in (base.any_plan(algo, side, total, variant=t.LO), base.any_plan(algo, side, total, exec_mode=t.EXEC_STEPS)):
        assert status(args, sq, ws, p=other) == _lib.ERR_UNSUPPORTED
        assert other.shards_f32_norm_workspace_bytes(args) == 0
        other.close()
    with pytest.raises(t.AllredError) as e:
        plan.reduce_scatter_shards_f32_norm(args, 0, ws, stream=stream())
    assert e.value.status == _lib.ERR_ARG
    # the size query: 0 for what the call would refuse, 64 for an empty list
    assert plan.shards_f32_norm_workspace_bytes(args[:1] + [(ranks, stride, n, 0, shard_stride)]) == 0
    assert plan.shards_f32_norm_workspace_bytes(args[:1] + [(ranks, stride, 8 * total * 3, shard, 24)]) == 0
    assert lib.allred_plan_shards_f32_norm_workspace_bytes(plan._h, arr, -1) == 0
    assert plan.shards_f32_norm_workspace_bytes([]) == 64
    # count == 0: OK, nothing launched, norm_sq not written — the pointers are still checked
    with t.launch_trace() as tr:
        plan.reduce_scatter_shards_f32_norm([], sq, ws, stream=stream())
        assert status([], sq, ws) == _lib.OK and status([], 0, ws) == _lib.ERR_ARG and status([], sq, ws + 8) == _lib.ERR_ARG
    assert tr.count == 0
    norm.check_untouched("by a refused call, or by one with count == 0")
    base.check_buckets(buckets, [b.host for b in buckets], "written by a refused call")
    for got, h in zip(shards.got(), shards.host):
        assert np.array_equal(got, h), "a shard written by a refused call"
    # the accepted call in the gap wrote its P floats there and nothing else of the gap
    k, slot = shards.slot(1, 0)
    want = shards.expected(cases.stored(datas, 0.5))
    want[k][slot.stop:slot.stop + total] = f32_norm.expect_norm_sq(cases.stored(datas, 0.5)).view(np.uint32)
    for g, e in zip(gap_sq, want):
        assert f32_tree.same_f32(g.view(np.float32), e.view(np.float32)), "norm_sq in the gap of a wide stride"
    plan.close()


# ------------------------------------------------------------------ rows and shards beyond 2^32 elements
far = base.far   # the module-scoped arena fixture of tests/test_gpu_shards_f32.py: one arena per module


def test_far_rows_and_a_far_flat_shard_buffer(far):
    """The far layout of tests/test_gpu_shards_f32.py (8x8 Swing, 1 and 3 tiles per block, 63 F beyond
    2^32 floats): the shards bit for bit tests/f32_tree.py's, norm_sq tests/f32_norm.py's, the rank
    rows only read, every guard intact and the whole arena sentinel again."""
    algo, side, total = t.SWING, 8, 64
    scale = 1.0 / total
    datas = cases.bucket_list(algo, side, total, far_arena.F32_TILES, seed=3)
    for rows, (data, _) in zip(far.rows, datas):
        rows.upload(data)
    args = base.far_args(far)
    plan = base.any_plan(algo, side, total)
    norm = Norm(plan, args, total)
    try:
        with t.tuned(pipe_grid=5):
            with t.launch_trace() as tr:
                call(plan, None, norm, scale, args=args)
            torch.cuda.synchronize()
            assert tr.kernels == [f"k_tree_group_f32_norm<{total}, false>"]
            values = cases.stored(datas, scale)
            for i, (data, _) in enumerate(datas):
                assert f32_tree.same_f32(far.planes[i][0].read().view(np.float32), values[i]), f"bucket {i}: the shard"
                assert np.array_equal(far.rows[i].read(), data), f"bucket {i}: the rank rows are only read"
            norm.check(f32_norm.expect_norm_sq(values), "far rows, far shards")
    finally:
        plan.close()
        far.wipe()
    far.assert_sentinel()
