"""Both MXFP8 orientations from one all-gather pass (allred_plan_all_gather_shards_mxfp8_2d,
allred_plan_all_gather_shards_mxfp8_2d_launches; k_ag_group_mxfp8_2d).

A bucket is one row-major fp32 matrix W[nrows][cols] in shard blocks of R rows.  The row-wise outputs are
held against tests/mxfp8_ref.py AND against what all_gather_shards_mxfp8 writes on the same shard; the
column-wise outputs against tests/mx2d_ref.py AND against what all_gather_shards_mxfp8 writes from a shard that
holds W^T.  Everything BIT FOR BIT, whole buffers, around sentinel skews and guard rows; the shards are
test_gpu_shards_f32's (compact / wide / flat).  The data is mx2d_ref.hard_t (the 24 planted blocks down the
columns) and mx2d_ref.hard_rows (along the rows)."""
import functools
import os
import re

import numpy as np
import pytest

import far_arena
import mx2d_cases as mc
import mx2d_ref
import mxfp8_ref as ref
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_shards_f32 as f32t  # noqa: E402
import test_gpu_shards_mxfp8 as mxt  # noqa: E402  (its MxBucket, the layouts and the parametrisations)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT8 = mxt.SENT8
Shards, sched, grids, layouts, any_plan, stream, to_dev8 = (mxt.Shards, mxt.sched, mxt.grids, mxt.layouts, mxt.any_plan,
                                                            mxt.stream, mxt.to_dev8)
G = _lib.MX2D_GROUP_MAX
# (cols, R), tests/mx2d_cases.py: one square per block; three column groups of a patch two squares high; five column
# groups; a whole 64 x 64 patch; two column groups.  ONE row group per block, every one (tests/test_mx2d_classes.py)
SHAPES = mc.SHAPES
KINDS = ("hard_t", "hard_rows")
with open(os.path.join(os.path.dirname(os.path.abspath(t.__file__)), "csrc", "mx2d_span.hpp")) as _f:
    LG_SIDE = int(re.search(r"#define TSA_MX2D_LG_SIDE (\d+)", _f.read()).group(1))


def tf(x):
    return "true" if x else "false"


def kernel(total, rceil, rows=True):
    return f"k_ag_group_mxfp8_2d<{total}, {tf(rceil)}, {tf(rows)}>"


def shapes_of(total):
    """the bucket list of a schedule: P = 64 runs one square per block"""
    return mc.SHAPES_64 if total == 64 else SHAPES


def row_group_shapes(total):
    """the bucket list of the tests of several row groups per shard block"""
    return mc.ROW_GROUP_SHAPES_64 if total == 64 else mc.ROW_GROUP_SHAPES


@functools.lru_cache(maxsize=None)
def matrix(kind, total, cols, R, seed):
    W = getattr(mx2d_ref, kind)(total, cols, R, seed)
    W.flags.writeable = False
    return W


@functools.lru_cache(maxsize=None)
def expected(kind, total, cols, R, seed, rceil):
    W = matrix(kind, total, cols, R, seed)
    out = mx2d_ref.expected_rows(W, total, rceil) + mx2d_ref.expected_t(W, rceil)
    for a in out:
        a.flags.writeable = False
    return out   # rows, scales, t rows, t scales


class Bucket2d:
    """One bucket's four outputs, two MxBuckets (sentinel skews, a guard row each): .r row-wise (None: not given), .c
    column-wise.  arg: the first ten fields of allred_mx2d_bucket_f32."""

    def __init__(self, total, cols, R, skew=False, rows=True):
        self.total, self.cols, self.R = total, cols, R
        self.n = total * R * cols
        self.blk = self.n // total
        self.r = mxt.MxBucket(total, self.n, skew) if rows else None
        self.c = mxt.MxBucket(total, self.n, not skew)
        self.arg = (self.r.arg[:4] if rows else (None, 0, None, 0)) + self.c.arg[:4] + (self.n, cols)

    def parts(self):
        return [p for p in (self.r, self.c) if p is not None]

    def restore(self):
        for p in self.parts():
            p.restore()

    def check(self, want, what):
        """want: (rows, scales, t rows, t scales) of every rank, or None: every buffer as it was"""
        if want is None:
            for p in self.parts():
                p.check(p.host, what)
            return
        if self.r is not None:
            self.r.check(self.r.after(want[0], want[1]), what + " [row-wise]")
        self.c.check(self.c.after(want[2], want[3]), what + " [column-wise]")


def make(total, shapes, rows=True, seed=0):
    buckets = [Bucket2d(total, cols, R, skew=i % 2 == 1, rows=rows) for i, (cols, R) in enumerate(shapes)]
    keys = [(total, cols, R, 10 * seed + i) for i, (cols, R) in enumerate(shapes)]
    return buckets, keys


def fill(shards, kind, keys):
    shards.fill([mx2d_ref.blocks(matrix(kind, *k), k[0]) for k in keys])


def check_all(buckets, kind, keys, rceil, what):
    for i, (b, k) in enumerate(zip(buckets, keys)):
        b.check(expected(kind, *k, rceil), f"bucket {i} (cols={b.cols}, R={b.R}, {kind}, rceil={rceil}): {what}")


shards_unchanged = mxt.shards_unchanged


# ------------------------------------------------------------------ 1. every schedule, layout, grid, data and flag
@grids
@layouts
@sched
def test_both_orientations_in_every_rank(algo, side, total, layout, grid):
    buckets, keys = make(total, shapes_of(total))
    shards = Shards(buckets, layout)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        for kind in KINDS:
            fill(shards, kind, keys)
            assert plan.shards_mxfp8_2d_launches(shards.args()) == 1
            for rceil in (False, True):
                for b in buckets:
                    b.restore()
                with t.launch_trace() as tr:
                    plan.all_gather_shards_mxfp8_2d(shards.args(), rceil=rceil, stream=stream())
                assert tr.kernels == [kernel(total, rceil)]
                if grid:
                    assert tr.grids == [grid]
                check_all(buckets, kind, keys, rceil, "rows = mxfp8(W), t rows = mxfp8(W^T)")
                shards_unchanged(shards)
    plan.close()


# ------------------------------------------------------------------ 2. the guarantees, GPU against GPU
@pytest.mark.parametrize("rceil", [False, True])
@sched
def test_rows_and_t_rows_are_what_the_row_wise_call_writes(algo, side, total, rceil):
    """rows / scales: all_gather_shards_mxfp8 on the same shard.  t rows / t scales: all_gather_shards_mxfp8 on a
    shard buffer that holds W^T.  Then rows = scales = None: ROWS = false in the trace, the t outputs identical."""
    held_against_the_row_wise_call(algo, side, total, rceil, shapes_of(total), seed=1)


def held_against_the_row_wise_call(algo, side, total, rceil, shapes, seed):
    buckets, keys = make(total, shapes, seed=seed)
    shards = Shards(buckets, "wide")
    fill(shards, "hard_t", keys)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=5):
        plan.all_gather_shards_mxfp8_2d(shards.args(), rceil=rceil, stream=stream())
        got = [(b.r.got(), b.c.got()) for b in buckets]
        # the parent's call, twice, into fresh buffers
        same = [mxt.MxBucket(total, b.n, skew=b.r.row_stride != b.n) for b in buckets]
        s1 = Shards(same, "wide")
        s1.fill([mx2d_ref.blocks(matrix("hard_t", *k), total) for k in keys])
        plan.all_gather_shards_mxfp8(s1.args(), rceil=rceil, stream=stream())
        tr_b = [mxt.MxBucket(total, b.n, skew=b.c.row_stride != b.n) for b in buckets]
        s2 = Shards(tr_b, "compact")
        s2.fill([np.ascontiguousarray(matrix("hard_t", *k).T).reshape(total, -1) for k in keys])
        plan.all_gather_shards_mxfp8(s2.args(), rceil=rceil, stream=stream())
        for i, (g, a, b) in enumerate(zip(got, same, tr_b)):
            for name, x, y in zip(("rows", "scales"), g[0], a.got()):
                assert np.array_equal(x, y), f"bucket {i}: {name} differ from all_gather_shards_mxfp8 on the same shard"
            for name, x, y in zip(("t rows", "t scales"), g[1], b.got()):
                assert np.array_equal(x, y), f"bucket {i}: {name} differ from all_gather_shards_mxfp8 on a shard holding W^T"
        # column-wise only
        only, _ = make(total, shapes, rows=False, seed=seed)
        s3 = Shards(only, "wide")
        fill(s3, "hard_t", keys)
        with t.launch_trace() as tr:
            plan.all_gather_shards_mxfp8_2d(s3.args(), rceil=rceil, stream=stream())
        assert tr.kernels == [kernel(total, rceil, rows=False)] and tr.grids == [5]
        for i, (g, b) in enumerate(zip(got, only)):
            for x, y in zip(g[1], b.c.got()):
                assert np.array_equal(x, y), f"bucket {i}: the t outputs without rows differ"
        shards_unchanged(s3)
        for b in buckets:   # the first call's buffers: no other byte touched since
            for x, y in zip(got[buckets.index(b)][0], b.r.got()):
                assert np.array_equal(x, y)
    plan.close()


def test_dequantised_t_rows_are_the_transpose():
    """finite Gaussian data of mixed magnitude: mxfp8_dequantize of the t rows is W^T within the format's error"""
    algo, side, total, cols, R = t.SWING, 4, 8, 96, 64
    rng = np.random.default_rng(5)
    nrows = total * R
    W = (rng.standard_normal((nrows, cols)) * np.exp2(rng.integers(-20, 12, (nrows // 32, cols)).repeat(32, axis=0))).astype(np.float32)
    b = Bucket2d(total, cols, R)
    shards = Shards([b], "flat")
    shards.fill([mx2d_ref.blocks(W, total)])
    plan = any_plan(algo, side, total)
    plan.all_gather_shards_mxfp8_2d(shards.args(), rceil=True, stream=stream())
    e, s = b.c.got()
    we, ws = mx2d_ref.expected_t(W, True)
    b.check(mx2d_ref.expected_rows(W, total, True) + (we, ws), "gaussian")
    got = t.mxfp8_dequantize(e[total - 1, :b.n], s[total - 1, :b.n // 32]).reshape(cols, nrows)
    X = ref.scale_exponent(ref.block_amax_bits(W.T.copy()), True)
    err = np.abs(got.astype(np.float64) - W.T.astype(np.float64))
    assert (err <= np.exp2(X + 4.0).repeat(32, axis=1)).all()   # half a step of the top e4m3 binade: 2^(X + 8) * 2^-4
    plan.close()


# ------------------------------------------------------------------ 3. lists: mixed shapes, launch splitting
@pytest.mark.parametrize("count", [1, G, G + 1, 2 * G + 1])
def test_21_buckets_per_launch(count):
    algo, side, total = t.SWING, 4, 8
    launches = -(-count // G)
    shapes = [SHAPES[i % 3] for i in range(count)]
    buckets = [Bucket2d(total, cols, R, skew=i % 3 == 0, rows=i % 4 != 3) for i, (cols, R) in enumerate(shapes)]
    keys = [(total, cols, R, 100 + i % 5) for i, (cols, R) in enumerate(shapes)]
    shards = Shards(buckets, "flat")
    fill(shards, "hard_t", keys)
    plan = any_plan(algo, side, total)
    assert plan.shards_mxfp8_2d_launches(shards.args()) == launches
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp8_2d(shards.args(), rceil=True, stream=stream())
    # a launch traces ROWS = true when one of its buckets has rows
    assert tr.count == launches and tr.kernels == [kernel(total, True)] * launches
    check_all(buckets, "hard_t", keys, True, f"{count} buckets in {launches} launches")
    shards_unchanged(shards)
    plan.close()


# ------------------------------------------------------------------ 4. side stream, late inputs, graph replay
def test_on_a_side_stream_behind_late_inputs():
    algo, side, total = t.SWING, 4, 16
    buckets, keys = make(total, SHAPES[:3], seed=2)
    shards = Shards(buckets, "flat")
    fill(shards, "hard_t", keys)
    staged = [f32t.to_dev32(h) for h in shards.host]
    scratch = torch.empty(1 << 28, dtype=torch.uint8, device=DEV)
    plan = any_plan(algo, side, total)
    s = torch.cuda.Stream()
    for d in shards.buf:
        d.fill_(0x7FC00000)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for i in range(16):
            scratch.fill_(i)
        for d, h in zip(shards.buf, staged):
            d.copy_(h, non_blocking=True)
        plan.all_gather_shards_mxfp8_2d(shards.args(), rceil=False, stream=s)
    s.synchronize()
    check_all(buckets, "hard_t", keys, False, "on a side stream behind late inputs")
    del scratch
    plan.close()


@pytest.mark.parametrize("rceil", [False, True])
def test_captured_once_replayed_three_times_on_rewritten_shards(rceil):
    algo, side, total = t.SWING, 4, 16
    buckets, keys = make(total, SHAPES[:4], seed=3)
    shards = Shards(buckets, "wide")
    fill(shards, "hard_t", keys)
    args = shards.args()
    plan = any_plan(algo, side, total)
    s = torch.cuda.Stream()
    with t.tuned(pipe_grid=5):
        with torch.cuda.stream(s):   # an eager call first: nothing is loaded inside the capture
            plan.all_gather_shards_mxfp8_2d(args, rceil=rceil, stream=s)
        s.synchronize()
        check_all(buckets, "hard_t", keys, rceil, "eager")
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with t.launch_trace() as tr:
                plan.all_gather_shards_mxfp8_2d(args, rceil=rceil, stream=s)
    torch.cuda.synchronize()
    assert tr.kernels == [kernel(total, rceil)]
    for b in buckets:
        b.check(None, "a capture runs nothing")
    for kind, ks in (("hard_t", keys), ("hard_rows", keys), ("hard_t", [k[:3] + (k[3] + 50,) for k in keys])):
        fill(shards, kind, ks)
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        check_all(buckets, kind, ks, rceil, "replay")
        shards_unchanged(shards)
    del g
    plan.close()


# ------------------------------------------------------------------ 5. t rows beyond 2^32 bytes
def test_far_t_rows():
    """8x8 Swing, one bucket of one square per block, column-wise only.  One arena, not filled: a 4 GiB front pad and 64
    t rows at a stride that puts the last one beyond 2^32 bytes, the t scale rows behind them at the same stride.
    A guard window around every payload row is initialised and compared."""
    algo, side, total, cols, R = t.SWING, 8, 64, 32, 32
    n, GD = total * R * cols, far_arena.GUARD
    stride = far_arena.roundup(-(-(1 << 32) // (total - 1)), 16) + 16 * 17
    assert (total - 1) * stride > 1 << 32 and stride % 16 == 0
    rows_at = far_arena.FRONT + GD
    scales_at = far_arena.roundup(rows_at + total * stride, GD) + GD
    nbytes = scales_at + total * stride + GD
    arena = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    windows = [(at + r * stride, width) for at, width in ((rows_at, n), (scales_at, n // 32)) for r in range(total)]
    for a, width in windows:
        arena[a - GD:a + width + GD].fill_(SENT8)
    W = matrix("hard_t", total, cols, R, 9)
    shard = f32t.to_dev32(mx2d_ref.blocks(W, total).copy())
    args = [(None, 0, None, 0, arena.data_ptr() + rows_at, stride, arena.data_ptr() + scales_at, stride, n, cols,
             shard.data_ptr(), R * cols)]
    plan = any_plan(algo, side, total)
    try:
        with t.tuned(pipe_grid=5):
            for rceil in (False, True):
                with t.launch_trace() as tr:
                    plan.all_gather_shards_mxfp8_2d(args, rceil=rceil, stream=stream())
                torch.cuda.synchronize()
                assert tr.kernels == [kernel(total, rceil, rows=False)]
                _, _, we, ws = expected("hard_t", total, cols, R, 9, rceil)
                for k, (a, width) in enumerate(windows):
                    got = arena[a - GD:a + width + GD].cpu().numpy()
                    want = np.full(width + 2 * GD, SENT8, dtype=np.uint8)
                    want[GD:GD + width] = we if width == n else ws
                    assert np.array_equal(got, want), f"{'t element' if k < total else 't scale'} row {k % total} (rceil={rceil})"
                    arena[a:a + width].fill_(SENT8)
        assert np.array_equal(shard.cpu().numpy().view(np.uint32), mx2d_ref.blocks(W, total).view(np.uint32))
    finally:
        plan.close()
        del arena
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 6. refusals, count == 0, outputs in a gap
def test_refusals_leave_every_buffer_untouched():
    algo, side, total = t.SWING, 4, 8
    buckets, keys = make(total, SHAPES[:3])
    shards = Shards(buckets, "compact")
    fill(shards, "hard_t", keys)
    args = shards.args()
    s = stream()

    def refused(status, call):
        with pytest.raises(t.AllredError) as e:
            call()
        assert e.value.status == status, (e.value.status, status)

    def refused_everywhere(status, plan, lst):
        refused(status, lambda: plan.all_gather_shards_mxfp8_2d(lst, stream=s))
        refused(status, lambda: plan.all_gather_shards_mxfp8_2d(lst, rceil=True, stream=s))
        refused(status, lambda: plan.shards_mxfp8_2d_launches(lst))

    for plan in (any_plan(algo, side, total, variant=t.LO), any_plan(algo, side, total, variant=t.MEM),
                 any_plan(algo, side, total, exec_mode=t.EXEC_STEPS)):
        refused_everywhere(_lib.ERR_UNSUPPORTED, plan, args)
        plan.close()
    rows, rs, sc, ss, tr_, trs, tsc, tss, n, cols, shard, sst = args[1]    # cols 96, R 64
    blk = n // total
    rest = args[:1] + args[2:]
    p4 = t.Plan(t.SWING, t.BO, 2, 256 * 4, 4, t.EXEC_FUSED)   # total < 8
    refused_everywhere(_lib.ERR_UNSUPPORTED, p4, [(rows, rs, sc, ss, tr_, trs, tsc, tss, 4 * 32 * 32, 32, shard, 1024)])
    p4.close()
    plan = any_plan(algo, side, total)
    assert n % 48 == 0 and (n // 48) % (32 * total) == 0
    for part in [(rows, rs, sc, ss, tr_, trs, tsc, tss, n, 48, shard, sst),              # cols % 32 != 0, nothing else wrong
                 (rows, rs, sc, ss, tr_, trs, tsc, tss, 96 * 128, 96, shard, sst),       # nrows = 128: % (32 total) != 0
                 (rows, rs, sc, ss, tr_, trs, tsc, tss, 96 * 32 * 12, 96, shard, sst)]:  # nrows = 384, R = 48: % 32 != 0
        refused_everywhere(_lib.ERR_UNSUPPORTED, plan, rest + [part])   # the whole list, wherever it stands
        refused_everywhere(_lib.ERR_UNSUPPORTED, plan, [part] + rest)
    o = args[2]
    B = lambda **kw: rest + [tuple({**dict(zip("rows rs sc ss tr trs tsc tss n cols shard sst".split(), args[1])), **kw}.values())]  # noqa: E731
    bad_lists = [
        B(rows=None), B(sc=None),                                   # exactly one of rows and scales
        B(tr=None), B(tsc=None), B(shard=None),                     # NULL pointers
        B(cols=0), B(cols=7 * 32 * 5),                              # cols == 0; elems_per_rank % cols != 0
        B(rows=rows + 8), B(sc=sc + 4), B(tr=tr_ + 8), B(tsc=tsc + 4), B(shard=shard + 8),   # alignment
        B(rs=n - 16), B(rs=rs + 8), B(ss=n // 32 - 8), B(ss=ss + 4),
        B(trs=n - 16), B(trs=trs + 8), B(tss=n // 32 - 8), B(tss=tss + 4),
        B(sst=blk - 4), B(sst=blk + 2),
        B(n=0), B(n=n + 8),
        B(tr=rows), B(tsc=sc), B(tsc=rows + total * rs - 8),        # a t output on the bucket's own row-wise outputs
        B(tsc=tr_ + total * trs - 8), B(sc=tr_),                    # ... the scale rows on the t rows' last 8 bytes
        B(tr=o[4]), B(tsc=o[6]), B(tr=o[0] + o[1]), B(tsc=o[2]),    # on another bucket's outputs
        B(shard=o[10]), B(shard=tr_, sst=blk),                      # one shard twice; the shard on the t rows
        B(tsc=shard + 4 * blk - 8),                                 # t scales on the last 8 bytes of shard block 0
        B(sst=1 << 62), B(sst=1 << 63), B(trs=1 << 62), B(tss=1 << 62), B(rs=1 << 62),   # overflow
    ]
    for bad in bad_lists:
        refused_everywhere(_lib.ERR_ARG, plan, bad)
    arr, cnt = plan._mx2d_buckets_f32(args)
    lib = _lib.lib
    for flags in (2, 3, 0x100, -2):
        assert lib.allred_plan_all_gather_shards_mxfp8_2d(plan._h, arr, cnt, flags, None) == _lib.ERR_ARG
        assert lib.allred_plan_all_gather_shards_mxfp8_2d(plan._h, None, 0, flags, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8_2d(plan._h, arr, -1, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8_2d(plan._h, None, 2, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8_2d(None, arr, cnt, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8_2d_launches(plan._h, arr, -1) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8_2d_launches(plan._h, None, 2) == _lib.ERR_ARG
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp8_2d([], stream=s)
        plan.all_gather_shards_mxfp8_2d([], rceil=True, stream=s)
        assert lib.allred_plan_all_gather_shards_mxfp8_2d(plan._h, None, 0, 1, None) == _lib.OK
    assert tr.count == 0 and plan.shards_mxfp8_2d_launches([]) == 0
    assert lib.allred_plan_all_gather_shards_mxfp8_2d_launches(plan._h, arr, cnt) == 1   # the list itself is fine
    plan.close()
    for b in buckets:
        b.check(None, "written by a refused call")
    shards_unchanged(shards)


def test_all_four_outputs_fill_a_stride_gap_exactly():
    """ONE buffer: 8 shard blocks of 1024 floats (cols 32, R 32) at a wide stride; the four output intervals, one behind
    the other, fill the gap behind block 0 exactly.  Accepted, every byte of the buffer what it must be; every overlap
    of one byte quantum refused."""
    algo, side, total, cols, R = t.SWING, 4, 8, 32, 32
    blk = R * cols
    n = total * blk
    gap = 2 * total * n + 2 * total * (n // 32)
    sst = blk + gap // 4
    size = 4 * (total * sst + 64)
    W = matrix("hard_t", total, cols, R, 4)
    x = mx2d_ref.blocks(W, total)
    host = np.full(size, SENT8, dtype=np.uint8)
    for b in range(total):
        host[4 * b * sst:4 * (b * sst + blk)] = x[b].view(np.uint8)
    buf = to_dev8(host)
    at = [4 * blk, 4 * blk + total * n, 4 * blk + 2 * total * n, 4 * blk + 2 * total * n + total * (n // 32)]   # rows, t rows, scales, t scales
    p = [buf.data_ptr() + a for a in at]
    good = (p[0], n, p[2], n // 32, p[1], n, p[3], n // 32, n, cols, buf.data_ptr(), sst)
    plan = any_plan(algo, side, total)
    assert plan.shards_mxfp8_2d_launches([good]) == 1
    plan.all_gather_shards_mxfp8_2d([good], rceil=True, stream=stream())
    torch.cuda.synchronize()
    we, ws, wte, wts = expected("hard_t", total, cols, R, 4, True)
    want = host.copy()
    for a, w in zip(at, (we, wte, ws, wts)):
        want[a:a + total * len(w)] = np.tile(w, total)
    assert np.array_equal(buf.cpu().numpy(), want)
    for k, d in ((0, -16), (4, -16), (2, 8), (6, 8), (6, -8), (4, 16)):   # on block 0's tail, a neighbour, or block 1's head
        bad = list(good)
        bad[k] += d
        with pytest.raises(t.AllredError) as e:
            plan.all_gather_shards_mxfp8_2d([tuple(bad)], stream=stream())
        assert e.value.status == _lib.ERR_ARG, (k, d)
    plan.close()
    assert np.array_equal(buf.cpu().numpy(), want)


# ------------------------------------------------------------------ 7. the t rows through the scaled MFMA
def test_t_rows_feed_the_scaled_mfma():
    """8 ranks, one bucket of cols = 32, R = 32: a t row is W^T, 32 rows of 256 bytes (two k-steps).  Rank 0's and the
    last rank's t rows go to v_mfma_scale_f32_16x16x128_f8f6f4 through tests/mx_consumer.hip's helper as they lie, 16
    matrix rows at a time; the MFMA reads them as W^T dequantised."""
    import test_gpu_mx_consumer as mfma
    algo, side, total, cols, R = t.SWING, 4, 8, 32, 32
    k = total * R
    b = Bucket2d(total, cols, R, skew=True)
    shards = Shards([b], "flat")
    fill(shards, "hard_t", [(total, cols, R, 22)])
    plan = any_plan(algo, side, total)
    plan.all_gather_shards_mxfp8_2d(shards.args(), stream=stream())
    want4 = expected("hard_t", total, cols, R, 22, False)
    b.check(want4, "the rows the MFMA is about to read")
    want = ref.dequantize64(want4[2], want4[3]).reshape(cols, k)
    nan_rows = np.isnan(want).any(axis=1)
    assert nan_rows.any() and not nan_rows.all()
    for r in (0, total - 1):
        for half in (0, 1):
            rows = slice(16 * half, 16 * half + 16)
            got = mfma.every_element(b.c.buf[0].data_ptr() + r * b.c.row_stride + 16 * half * k, k,
                                     b.c.buf[1].data_ptr() + r * b.c.scale_stride + 16 * half * (k // 32), k // 32, 16, k)
            nr = nan_rows[rows]
            assert np.isnan(got[nr]).all() and not np.isnan(got[~nr]).any()
            mfma.report(f"rank {r} rows {rows}", mfma.same_value(got[~nr], want[rows][~nr], f"rank {r}'s t row"))
    plan.close()


# ------------------------------------------------------------------ 8. several row groups per shard block
# SHAPES above has ONE row group per block at the build's 64 x 64 patch: the row-group terms of mx2d_unit_at — in the
# shard read, in the row-wise rows, in the t rows — vanish there.  mc.ROW_GROUP_SHAPES has two or three row groups
# under each patch class; tests/test_mx2d_classes.py shows on the CPU which mistakes only these shapes see.
ROW_GROUP_SEED = 4


def squares_by_workgroup(total, shapes, grid):
    """per workgroup, the square counts of the units it walks: unit x of the launch — the buckets in list order, a
    bucket's blocks in order, a block's units in order (group_span.hpp) — goes to workgroup x % grid"""
    squares = []
    for cols, R in shapes:
        lgh, lgw, rgs, cgs = mc.shape_class(cols, R, LG_SIDE)
        squares += [1 << (lgh + lgw)] * (total * rgs * cgs)
    return [squares[g::grid] for g in range(grid)]


@pytest.mark.parametrize("kind", KINDS)
@grids
@layouts
@sched
def test_several_row_groups_per_block(algo, side, total, layout, grid, kind):
    shapes = row_group_shapes(total)
    assert all(mc.shape_class(cols, R, LG_SIDE)[2] >= 2 for cols, R in shapes)
    if grid:   # every workgroup walks patches of one, two and four squares: the LDS images rotate across unequal patches
        walks = squares_by_workgroup(total, shapes, grid)
        assert len(walks) == grid and all(set(w) == {1, 2, 4} and len(w) >= 3 for w in walks), [sorted(set(w)) for w in walks]
    buckets, keys = make(total, shapes, seed=ROW_GROUP_SEED)
    shards = Shards(buckets, layout)
    fill(shards, kind, keys)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.shards_mxfp8_2d_launches(shards.args()) == 1
        for rceil in (False, True):
            for b in buckets:
                b.restore()
            with t.launch_trace() as tr:
                plan.all_gather_shards_mxfp8_2d(shards.args(), rceil=rceil, stream=stream())
            assert tr.kernels == [kernel(total, rceil)]
            if grid:
                assert tr.grids == [grid]
            check_all(buckets, kind, keys, rceil, "rows = mxfp8(W), t rows = mxfp8(W^T), several row groups per block")
            shards_unchanged(shards)
    plan.close()


@pytest.mark.parametrize("rceil", [False, True])
@pytest.mark.parametrize("side,total", [(4, 8), (4, 16), (8, 64)])
def test_row_groups_rows_and_t_rows_are_what_the_row_wise_call_writes(side, total, rceil):
    """test 2's guarantees, GPU against GPU, on the lists of several row groups per block"""
    held_against_the_row_wise_call(t.SWING, side, total, rceil, row_group_shapes(total), seed=ROW_GROUP_SEED)


@pytest.mark.parametrize("rows_first", [True, False], ids=["rows-then-none", "none-then-rows"])
def test_a_launch_with_rows_beside_a_launch_without(rows_first):
    """G + 2 buckets, two launches: the buckets of one have row-wise outputs (but for every fourth), those of the other
    have none.  The launcher's side table is reset between the launches: the trace says ROWS = true for the one and
    ROWS = false for the other, in either order.  Each launch holds buckets of several row groups per block."""
    algo, side, total = t.SWING, 4, 8
    cycle = ((32, 96), (96, 64), (64, 128))
    shapes = [cycle[i % 3] for i in range(G + 2)]
    for launch in (shapes[:G], shapes[G:]):
        assert any(mc.shape_class(cols, R, LG_SIDE)[2] >= 2 for cols, R in launch)
    has_rows = [(i < G) == rows_first and i % 4 != 3 for i in range(G + 2)]
    assert any(has_rows[:G]) == rows_first and any(has_rows[G:]) != rows_first
    buckets = [Bucket2d(total, cols, R, skew=i % 3 == 0, rows=has_rows[i]) for i, (cols, R) in enumerate(shapes)]
    keys = [(total, cols, R, 100 + i % 5) for i, (cols, R) in enumerate(shapes)]
    shards = Shards(buckets, "flat")
    fill(shards, "hard_t", keys)
    plan = any_plan(algo, side, total)
    assert plan.shards_mxfp8_2d_launches(shards.args()) == 2
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp8_2d(shards.args(), rceil=True, stream=stream())
    assert tr.kernels == [kernel(total, True, rows=rows_first), kernel(total, True, rows=not rows_first)]
    check_all(buckets, "hard_t", keys, True, f"{G} buckets {'with' if rows_first else 'without'} rows, then 2 {'without' if rows_first else 'with'}")
    shards_unchanged(shards)
    plan.close()


def finite_in_the_odd_columns(W):
    """W = hard_t with nrows = 768: a column is 24 MX blocks, every planted kind once, so every t row would hold a NaN
    block and the MFMA would answer NaN for every matrix row.  In the odd columns each block with a NaN or an Inf is
    replaced by the block eight above it, a finite kind: sixteen matrix rows keep their NaNs, sixteen are finite."""
    import test_gpu_mx_consumer as mfma
    nrows, cols = W.shape
    wt = np.ascontiguousarray(W.T).reshape(cols, nrows // 32, 32)
    kind = mx2d_ref.planted_kind(nrows, cols)
    for j in range(1, cols, 2):
        for b in np.flatnonzero(np.isin(kind[j], mfma.NAN_BLOCKS)):
            assert b >= 8 and kind[j, b - 8] not in mfma.NAN_BLOCKS
            wt[j, b] = wt[j, b - 8]
    assert np.isfinite(wt[1::2]).all() and not np.isfinite(wt[0::2]).all(axis=(1, 2)).any()
    return np.ascontiguousarray(wt.reshape(cols, nrows).T)


def test_t_rows_across_row_groups_feed_the_scaled_mfma():
    """8 ranks, one bucket of cols = 32, R = 96: a t row is W^T, 32 matrix rows of k = 768 bytes, six k-steps, and each
    matrix row crosses three row groups in every shard block — the neighbours along nrows that the test above never
    crosses inside a block.  Rank 0's and the last rank's t rows go to the MFMA as they lie, 16 matrix rows at a time."""
    import test_gpu_mx_consumer as mfma
    algo, side, total, cols, R = t.SWING, 4, 8, 32, 96
    assert mc.shape_class(cols, R, LG_SIDE)[2] == 3
    k = total * R
    W = finite_in_the_odd_columns(matrix("hard_t", total, cols, R, 22))
    b = Bucket2d(total, cols, R, skew=True)
    shards = Shards([b], "flat")
    shards.fill([mx2d_ref.blocks(W, total)])
    plan = any_plan(algo, side, total)
    plan.all_gather_shards_mxfp8_2d(shards.args(), stream=stream())
    want4 = mx2d_ref.expected_rows(W, total) + mx2d_ref.expected_t(W)
    b.check(want4, "the rows the MFMA is about to read")
    want = ref.dequantize64(want4[2], want4[3]).reshape(cols, k)
    nan_rows = np.isnan(want).any(axis=1)
    assert np.array_equal(nan_rows, np.arange(cols) % 2 == 0)
    for r in (0, total - 1):
        for half in (0, 1):
            rows = slice(16 * half, 16 * half + 16)
            got = mfma.every_element(b.c.buf[0].data_ptr() + r * b.c.row_stride + 16 * half * k, k,
                                     b.c.buf[1].data_ptr() + r * b.c.scale_stride + 16 * half * (k // 32), k // 32, 16, k)
            nr = nan_rows[rows]
            assert np.isnan(got[nr]).all() and not np.isnan(got[~nr]).any()
            mfma.report(f"rank {r} rows {rows}", mfma.same_value(got[~nr], want[rows][~nr], f"rank {r}'s t row"))
    plan.close()
