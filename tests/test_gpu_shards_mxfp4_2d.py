"""Both MXFP4 orientations from one all-gather pass (allred_plan_all_gather_shards_mxfp4_2d and its _launches twin;
k_ag_group_mxfp4_2d) against tests/mx4_2d_ref.py, BIT FOR BIT, whole buffers around sentinel skews and guard rows.
The buffers are test_gpu_shards_mxfp4's nibble buckets in test_gpu_shards_mxfp8_2d's Bucket2d; the data is the 17
planted blocks of tests/mx4_cases.py laid down the columns (hard_t) and along the rows (hard_rows)."""
import functools
import os
import re

import numpy as np
import pytest

import mx4_2d_ref as r2
import mxfp4_ref as ref
import soak_cases as sc
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_shards_f32 as f32t  # noqa: E402
import test_gpu_shards_mxfp4 as mx4  # noqa: E402  (its nibble bucket)
import test_gpu_shards_mxfp8 as mx8  # noqa: E402
import test_gpu_shards_mxfp8_2d as m2  # noqa: E402  (its Bucket2d)

pytestmark = pytest.mark.gpu
Shards, stream = f32t.Shards, f32t.stream
G = _lib.MX4_2D_GROUP_MAX
KINDS = ("hard_t", "hard_rows")
with open(os.path.join(os.path.dirname(os.path.abspath(t.__file__)), "csrc", "mx4_2d_span.hpp")) as _f:
    LG_STRIP = int(re.search(r"#define TSA_MX4_2D_LG_STRIP (\d+)", _f.read()).group(1))


def units(total, cols, R):
    """the work units of a bucket (csrc/mx4_2d_span.hpp): strips of 1 << LG_STRIP row groups by column groups of the
    largest power of two of squares, up to 16 squares a strip, that cols / 32 divides by"""
    sw = max(w for w in (1, 2, 4) if w << LG_STRIP <= 16 and cols // 32 % w == 0)
    return (total * R // (32 << LG_STRIP)) * (cols // (32 * sw))


def plan_for(total, **kw):
    return f32t.any_plan(t.SWING, sc.SIDE[total], total, **kw)


def kernel(total, rceil, rows=True):
    return f"k_ag_group_mxfp4_2d<{total}, {m2.tf(rceil)}, {m2.tf(rows)}>"


@functools.lru_cache(maxsize=None)
def matrix(kind, total, cols, R, seed):
    return getattr(r2, kind)(total, cols, R, seed)


@functools.lru_cache(maxsize=None)
def expected(kind, total, cols, R, seed, rceil):
    return r2.expected(matrix(kind, total, cols, R, seed), total, rceil)   # rows, scales, t rows, t scales


class Bucket2d(m2.Bucket2d):
    """m2.Bucket2d over nibble rows: n / 2 payload bytes per element row"""

    def __init__(self, total, cols, R, skew=False, rows=True):
        self.total, self.cols, self.R, self.n, self.blk = total, cols, R, total * R * cols, R * cols
        self.r = mx4.Mx4Bucket(total, self.n, skew) if rows else None
        self.c = mx4.Mx4Bucket(total, self.n, not skew)
        self.arg = (self.r.arg[:4] if rows else (None, 0, None, 0)) + self.c.arg[:4] + (self.n, cols)


def make(total, shapes, rows=lambda i: True, seed=0):
    buckets = [Bucket2d(total, cols, R, skew=i % 2 == 1, rows=rows(i)) for i, (cols, R) in enumerate(shapes)]
    return buckets, [(total, cols, R, 10 * seed + i) for i, (cols, R) in enumerate(shapes)]


def fill(shards, kind, keys):
    shards.fill([matrix(kind, *k).reshape(k[0], -1) for k in keys])


def check_all(buckets, kind, keys, rceil, what):
    for i, (b, k) in enumerate(zip(buckets, keys)):
        b.check(expected(kind, *k, rceil), f"bucket {i} (cols={b.cols}, R={b.R}, {kind}, rceil={rceil}): {what}")


# ------------------------------------------------------------------ (a) every rank receives both orientations
@pytest.mark.parametrize("grid", [0, 5], ids=["default-grid", "grid5"])
@pytest.mark.parametrize("rows", [True, False], ids=["rows", "t-only"])
@pytest.mark.parametrize("total,cols,R", r2.SHAPES)
def test_both_orientations_in_every_rank(total, cols, R, rows, grid):
    buckets, keys = make(total, [(cols, R)], rows=lambda i: rows)
    shards = Shards(buckets, "wide")
    plan = plan_for(total)
    with t.tuned(pipe_grid=grid):
        for kind in KINDS:
            fill(shards, kind, keys)
            assert plan.shards_mxfp4_2d_launches(shards.args()) == 1
            for rceil in (False, True):
                buckets[0].restore()
                with t.launch_trace() as tr:
                    plan.all_gather_shards_mxfp4_2d(shards.args(), rceil=rceil, stream=stream())
                assert tr.kernels == [kernel(total, rceil, rows)] and (not grid or tr.grids == [min(grid, units(total, cols, R))])
                check_all(buckets, kind, keys, rceil, "rows = mxfp4(W), t rows = mxfp4(W^T)")
                mx8.shards_unchanged(shards)
    plan.close()


# ------------------------------------------------------------------ (b) GPU against GPU
@pytest.mark.parametrize("total,cols,R", [(8, 64, 96), (64, 32, 32)])
def test_rows_and_t_rows_are_what_the_row_wise_call_writes(total, cols, R):
    """rows / scales: all_gather_shards_mxfp4 on the same shard; t rows / t scales: all_gather_shards_mxfp4 on a shard
    that holds W^T; mxfp4_dequantize of the t rows: the reference's float64 dequantisation cast to fp32"""
    rceil = total == 8
    buckets, keys = make(total, [(cols, R)], seed=1)
    b, W = buckets[0], matrix("hard_t", total, cols, R, 10)
    shards = Shards(buckets, "flat")
    fill(shards, "hard_t", keys)
    plan = plan_for(total)
    plan.all_gather_shards_mxfp4_2d(shards.args(), rceil=rceil, stream=stream())
    for part, blocks, what in ((b.r, W, "the same shard"), (b.c, np.ascontiguousarray(W.T), "a shard holding W^T")):
        one = mx4.Mx4Bucket(total, b.n, skew=part.row_stride != b.n // 2)
        s1 = Shards([one], "compact")
        s1.fill([blocks.reshape(total, -1)])
        plan.all_gather_shards_mxfp4(s1.args(), rceil=rceil, stream=stream())
        for name, x, y in zip(("elements", "scales"), part.got(), one.got()):
            assert np.array_equal(x, y), f"{name} differ from all_gather_shards_mxfp4 on {what}"
    e, s = b.c.got()
    got = t.mxfp4_dequantize(e[:total, :b.n // 2], s[:total, :b.n // 32])
    with np.errstate(over="ignore"):
        want = ref.dequantize64(*expected("hard_t", total, cols, R, 10, rceil)[2:]).astype(np.float32)
    nan = np.isnan(want)
    assert nan.any() and np.array_equal(np.isnan(got), np.broadcast_to(nan, got.shape))
    assert np.array_equal(got[:, ~nan].view(np.uint32), np.broadcast_to(want[~nan].view(np.uint32), (total, (~nan).sum())))
    plan.close()


# ------------------------------------------------------------------ (c) a list of two launches
def test_one_bucket_more_than_a_launch_holds():
    total, cycle = 8, ((32, 32), (96, 64), (64, 96))
    buckets, keys = make(total, [cycle[i % 3] for i in range(G + 1)], rows=lambda i: i % 3 != 0, seed=2)
    assert buckets[G].r is None
    shards = Shards(buckets, "flat")
    fill(shards, "hard_t", keys)
    plan = plan_for(total)
    assert plan.shards_mxfp4_2d_launches(shards.args()) == 2
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp4_2d(shards.args(), rceil=True, stream=stream())
    assert tr.kernels == [kernel(total, True, True), kernel(total, True, False)]
    check_all(buckets, "hard_t", keys, True, f"{G + 1} buckets in 2 launches")
    mx8.shards_unchanged(shards)
    plan.close()


# ------------------------------------------------------------------ (d) graph replay
def test_captured_once_replayed_twice_on_rewritten_shards():
    total = 16
    buckets, keys = make(total, [(64, 32), (96, 64), (32, 96)], rows=lambda i: i != 1, seed=3)
    shards = Shards(buckets, "wide")
    fill(shards, "hard_t", keys)
    args = shards.args()
    plan = plan_for(total)
    s = torch.cuda.Stream()
    with t.tuned(pipe_grid=5):
        with torch.cuda.stream(s):   # an eager call first: nothing is loaded inside the capture
            plan.all_gather_shards_mxfp4_2d(args, stream=s)
        s.synchronize()
        check_all(buckets, "hard_t", keys, False, "eager")
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.all_gather_shards_mxfp4_2d(args, stream=s)
    torch.cuda.synchronize()
    for b in buckets:
        b.check(None, "a capture runs nothing")
    for kind, ks in (("hard_rows", keys), ("hard_t", [k[:3] + (k[3] + 50,) for k in keys])):
        fill(shards, kind, ks)
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        check_all(buckets, kind, ks, False, "replay")
        mx8.shards_unchanged(shards)
    del g
    plan.close()


# ------------------------------------------------------------------ (e) refusals; the four outputs in a stride gap
FIELDS = "rows rs sc ss tr trs tsc tss n cols shard sst".split()


@pytest.fixture(scope="module")
def gap():
    """ONE buffer: 8 shard blocks of 1024 floats (cols 32, R 32) at a wide stride; rows, t rows, scales and t scales, one
    behind the other, fill the gap behind block 0 EXACTLY.  The list is accepted and every byte of the buffer is what it
    must be.  Yields (plan, the accepted bucket as a dict, the buffer, its expected bytes)."""
    total, cols, R = 8, 32, 32
    blk = R * cols
    n = total * blk
    sst = blk + (total * n + 2 * total * (n // 32)) // 4
    W = matrix("hard_t", total, cols, R, 4)
    host = np.full(4 * (total * sst + 64), mx8.SENT8, dtype=np.uint8)
    for b in range(total):
        host[4 * b * sst:4 * (b * sst + blk)] = W.reshape(total, -1)[b].view(np.uint8)
    buf = mx8.to_dev8(host)
    at = np.cumsum([4 * blk, total * n // 2, total * n // 2, total * n // 32])   # rows, t rows, scales, t scales
    assert at[3] + total * n // 32 == 4 * sst
    p = [buf.data_ptr() + int(a) for a in at]
    good = dict(zip(FIELDS, (p[0], n // 2, p[2], n // 32, p[1], n // 2, p[3], n // 32, n, cols, buf.data_ptr(), sst)))
    plan = plan_for(total)
    assert plan.shards_mxfp4_2d_launches([tuple(good.values())]) == 1
    plan.all_gather_shards_mxfp4_2d([tuple(good.values())], rceil=True, stream=stream())
    torch.cuda.synchronize()
    we, ws, wte, wts = expected("hard_t", total, cols, R, 4, True)
    want = host.copy()
    for a, w in zip(at, (we, wte, ws, wts)):
        want[a:a + total * len(w)] = np.tile(w, total)
    assert np.array_equal(buf.cpu().numpy(), want)
    yield plan, good, buf, want
    plan.close()


ARG, UNSUP = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
REFUSED = [   # (what changes in the accepted bucket: a value, or a byte delta on a pointer), the status
    (dict(rs=4096 - 16), ARG), (dict(trs=4096 - 16), ARG),                 # a stride one quantum short of elems_per_rank / 2
    (dict(rows=None), ARG), (dict(sc=None), ARG),                          # exactly one of rows and scales
    (dict(cols=16), UNSUP), (dict(cols=64), UNSUP),                        # cols % 32; nrows = 128: % (32 total)
    (dict(rows=-16), ARG), (dict(tr=-16), ARG), (dict(sc=+8), ARG),        # one quantum onto block 0's tail, the rows, the t scales,
    (dict(tsc=+8), ARG), (dict(tsc=-8), ARG), (dict(tr=+16), ARG),         # ... block 1's head, the scales, the scales
]


@pytest.mark.parametrize("change,status", REFUSED, ids=[f"{k}={v}" for c, _ in REFUSED for k, v in c.items()])
def test_a_refused_list_writes_nothing(gap, change, status):
    plan, good, buf, want = gap
    bad = dict(good)
    for k, v in change.items():
        bad[k] = good[k] + v if v is not None and k in ("rows", "sc", "tr", "tsc") else v
    lst = [tuple(bad.values())]
    for call in (lambda: plan.all_gather_shards_mxfp4_2d(lst, stream=stream()), lambda: plan.all_gather_shards_mxfp4_2d(lst, rceil=True, stream=stream()),
                 lambda: plan.shards_mxfp4_2d_launches(lst)):
        with pytest.raises(t.AllredError) as e:
            call()
        assert e.value.status == status
    assert np.array_equal(buf.cpu().numpy(), want)


def test_a_foreign_flag_bit_is_refused(gap):
    plan, good, buf, want = gap
    arr, cnt = plan._mx2d_buckets_f32([tuple(good.values())])
    for flags in (2, 3, 0x100, -2):
        assert _lib.lib.allred_plan_all_gather_shards_mxfp4_2d(plan._h, arr, cnt, flags, None) == ARG
    assert np.array_equal(buf.cpu().numpy(), want)
