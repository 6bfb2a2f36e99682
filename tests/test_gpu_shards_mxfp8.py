"""The MXFP8 all-gather from fp32 shards (allred_plan_all_gather_shards_mxfp8,
allred_plan_all_gather_shards_mxfp8_launches; k_ag_group_mxfp8).

Expectations come from tests/mxfp8_ref.py (numpy, written from the semantics of include/allred.h) and
are compared BIT FOR BIT.  The data is tests/mx_cases.py: 24 planted MX blocks cycled over every shard,
on which floor / RCEIL, RNE / truncation, an amax over fewer than 32 elements, a NaN-blind max and a
bf16-rounded amax all show (tests/test_mxfp8_ref.py).

Every bucket has an element buffer and a scale buffer of its own — `total` rows at their stride, the
stride skew and one guard row behind the last rank filled with a sentinel — and the fp32 shards are
test_gpu_shards_f32's Shards (compact / wide / flat, sentinel gaps and guards).  WHOLE buffers are
compared, so a stray write anywhere fails."""
import functools

import numpy as np
import pytest

import f32_tree
import far_arena
import mx_cases
import mxfp8_ref as ref
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_shards_f32 as f32t  # noqa: E402  (its Shards, schedules and parametrisations)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT8 = 0xA5
Shards, sched, grids, layouts, UNEQUAL, any_plan, stream = (f32t.Shards, f32t.sched, f32t.grids, f32t.layouts, f32t.UNEQUAL,
                                                           f32t.any_plan, f32t.stream)


@functools.lru_cache(maxsize=None)
def cases(total, blk, seed):
    x = mx_cases.shard(total, blk, seed)
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def expected(total, blk, seed, rceil):
    e, s = ref.expected_rows(cases(total, blk, seed), rceil)
    e.flags.writeable = False
    s.flags.writeable = False
    return e, s


def to_dev8(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class MxBucket:
    """One bucket's outputs in device buffers of their own: (total + 1) element rows of row_stride bytes and
    (total + 1) scale rows of scale_stride bytes, all SENT8.  skew: strides wider than the payload."""

    def __init__(self, total, n, skew=False):
        self.total, self.n, self.blk = total, n, n // total
        self.row_stride = n + (48 if skew else 0)
        self.scale_stride = n // 32 + (24 if skew else 0)
        self.host = (np.full((total + 1, self.row_stride), SENT8, dtype=np.uint8),
                     np.full((total + 1, self.scale_stride), SENT8, dtype=np.uint8))
        self.buf = tuple(to_dev8(h) for h in self.host)
        self.arg = (self.buf[0].data_ptr(), self.row_stride, self.buf[1].data_ptr(), self.scale_stride, n)

    def restore(self):
        for d, h in zip(self.buf, self.host):
            d.copy_(to_dev8(h))

    def got(self):
        torch.cuda.synchronize()
        return tuple(d.cpu().numpy() for d in self.buf)

    def after(self, elems, scales):
        """every rank's rows = (elems, scales); skew and guard rows keep the sentinel"""
        e, s = self.host[0].copy(), self.host[1].copy()
        e[:self.total, :self.n] = elems
        s[:self.total, :self.n // 32] = scales
        return e, s

    def check(self, want, what):
        for name, g, w in zip(("element rows", "scale rows"), self.got(), want):
            bad = np.argwhere(g != w)
            assert bad.size == 0, f"{what}: {name} differ in {len(bad)} bytes, first at row {bad[0][0]} byte {bad[0][1]}: " \
                                  f"0x{g[tuple(bad[0])]:02X}, expected 0x{w[tuple(bad[0])]:02X}"


def unequal(total, seed=0):
    """[256 P, 256 P 3, 256 P 2, 256 P 5] elements per rank, every other bucket with stride skews; the shard data"""
    buckets = [MxBucket(total, 256 * total * k, skew=i % 2 == 1) for i, k in enumerate(UNEQUAL)]
    return buckets, [(total, 256 * k, 10 * seed + i) for i, k in enumerate(UNEQUAL)]


def check_all(buckets, keys, rceil, what):
    for i, (b, key) in enumerate(zip(buckets, keys)):
        b.check(b.after(*expected(*key, rceil)), f"bucket {i} (n={b.n}, rceil={rceil}): {what}")


def shards_unchanged(shards):
    for g, h in zip(shards.got(), shards.host):
        assert np.array_equal(g, h), "the call wrote its shard, a gap or a guard"


# ------------------------------------------------------------------ 1. every schedule, layout, grid and flag
@grids
@layouts
@sched
def test_every_row_receives_the_quantised_shard(algo, side, total, layout, grid):
    """Block b of EVERY element row = the e4m3 bytes of shard block b, every scale row its E8M0 bytes, for both
    flag values; skews, guard rows, the shards with their gaps and guards keep their bits."""
    buckets, keys = unequal(total)
    shards = Shards(buckets, layout)
    shards.fill([cases(*k) for k in keys])
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.shards_mxfp8_launches(shards.args()) == 1
        for rceil in (False, True):
            for b in buckets:
                b.restore()
            with t.launch_trace() as tr:
                plan.all_gather_shards_mxfp8(shards.args(), rceil=rceil, stream=stream())
            assert tr.kernels == [f"k_ag_group_mxfp8<{total}, {'true' if rceil else 'false'}>"]
            check_all(buckets, keys, rceil, "block b of every row = mxfp8(shard block b)")
            shards_unchanged(shards)
    plan.close()


def test_planted_blocks_as_known_answers():
    """what the first planted tile must become, read from rank 0's and the last rank's rows"""
    algo, side, total = t.SWING, 4, 8
    b = MxBucket(total, 256 * total)
    shards = Shards([b], "compact")
    shards.fill([cases(total, 256, 0)])
    plan = any_plan(algo, side, total)
    for rceil, want in ((False, [119, 119, 119, 127, 107, 0, 0, 246]), (True, [119, 120, 119, 127, 107, 0, 0, 247])):
        b.restore()
        plan.all_gather_shards_mxfp8(shards.args(), rceil=rceil, stream=stream())
        e, s = b.got()
        for r in (0, total - 1):
            assert list(s[r, :8]) == want
            assert e[r, 3 * 32] == 0x7E and e[r, 4 * 32 + 9] == 0xFE and e[r, 5] == 0x7E      # 448 x 2^k -> +-448, 1.75 x 2^8 -> 448
            assert e[r, 32 + 17] == (0x76 if rceil else 0x7E)                                   # one ulp above: 224 x 2, or saturated
            assert list(s[r, 8:12]) == [0, 0xFF, 0xFF, 0xFF] and (e[r, 9 * 32:12 * 32] == 0x7F).all()
            assert set(e[r, 8 * 32:9 * 32]) == {0x00, 0x80}
    plan.close()


# ------------------------------------------------------------------ 2. random data, against the bf16 call's source
@sched
def test_random_data_dequantises_next_to_what_the_bf16_call_rounds(algo, side, total):
    """Gaussian shards of mixed magnitude: the dequantised rows are the dequantised CPU expectation, and every
    element is within 2^(X + 4) of the fp32 value all_gather_shards_f32 rounds to bf16 on the same shards
    (an element the floor rule saturates: below 2^(X + 6); under RCEIL there is none)."""
    rng = np.random.default_rng(total + algo)
    buckets, _ = unequal(total)
    rows16 = [f32t.Bucket(np.zeros((total, b.n), dtype=np.uint16)) for b in buckets]
    src = [(rng.standard_normal((total, b.blk)) * np.exp2(rng.integers(-20, 12, (total, b.blk // 32)).repeat(32, axis=1))
            ).astype(np.float32) for b in buckets]
    shards = Shards(buckets, "flat")
    shards.fill(src)
    plan = any_plan(algo, side, total)
    with t.tuned(pipe_grid=5):
        plan.all_gather_shards_f32([r.arg + a[5:] for r, a in zip(rows16, shards.args())], stream())
        for r, x in zip(rows16, src):
            assert np.array_equal(r.got()[:total, :r.n], np.broadcast_to(f32_tree.bf16_rne(x).reshape(-1), (total, r.n)))
        for rceil in (False, True):
            plan.all_gather_shards_mxfp8(shards.args(), rceil=rceil, stream=stream())
            for b, x in zip(buckets, src):
                e, s = b.got()
                we, ws = ref.expected_rows(x, rceil)
                b.check(b.after(we, ws), f"rceil={rceil}")
                got = t.mxfp8_dequantize(e[:total, :b.n], s[:total, :b.n // 32])
                assert np.array_equal(got, np.broadcast_to(t.mxfp8_dequantize(we, ws), got.shape))
                A = ref.block_amax_bits(x.reshape(-1))
                X, special = ref.scale_exponent(A, rceil), ref.is_special(A)
                sat = ref.saturated(x.reshape(-1), X, special)
                assert not special.any() and (sat.any() or rceil) and not (sat.any() and rceil)
                err = np.abs(got[0].astype(np.float64) - x.reshape(-1).astype(np.float64))
                assert (err <= np.where(sat, np.exp2(X + 6.0).repeat(32), np.exp2(X + 4.0).repeat(32))).all()
    plan.close()


# ------------------------------------------------------------------ 3. launch splitting
@pytest.mark.parametrize("count", [_lib.MX_GROUP_MAX, _lib.MX_GROUP_MAX + 1, 2 * _lib.MX_GROUP_MAX + 1])
def test_32_buckets_per_launch(count):
    algo, side, total = t.SWING, 4, 8
    launches = -(-count // 32)
    buckets = [MxBucket(total, 256 * total, skew=i % 3 == 0) for i in range(count)]
    keys = [(total, 256, 100 + i % 5) for i in range(count)]
    shards = Shards(buckets, "flat")
    shards.fill([cases(*k) for k in keys])
    plan = any_plan(algo, side, total)
    assert plan.shards_mxfp8_launches(shards.args()) == launches
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp8(shards.args(), rceil=True, stream=stream())
    assert tr.count == launches and tr.kernels == [f"k_ag_group_mxfp8<{total}, true>"] * launches
    check_all(buckets, keys, True, f"{count} buckets in {launches} launches")
    shards_unchanged(shards)
    plan.close()


# ------------------------------------------------------------------ 4. side stream, late inputs, graph replay
def test_on_a_side_stream_behind_late_inputs():
    """every shard holds NaN bits until, on the side stream and behind a few milliseconds of fills, the data
    arrives; the call is enqueued right behind it on that stream and only that stream is waited for"""
    algo, side, total = t.SWING, 4, 16
    buckets, keys = unequal(total, seed=2)
    shards = Shards(buckets, "flat")
    shards.fill([cases(*k) for k in keys])
    staged = [f32t.to_dev32(h) for h in shards.host]
    scratch = torch.empty(1 << 28, dtype=torch.uint8, device=DEV)
    plan = any_plan(algo, side, total)
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        for b in buckets:
            b.restore()
        for d in shards.buf:
            d.fill_(0x7FC00000)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for i in range(16):
                scratch.fill_(i)
            for d, h in zip(shards.buf, staged):
                d.copy_(h, non_blocking=True)
            plan.all_gather_shards_mxfp8(shards.args(), rceil=False, stream=s)
        s.synchronize()
        check_all(buckets, keys, False, "on a side stream behind late inputs")
    del scratch
    plan.close()


@pytest.mark.parametrize("rceil", [False, True])
def test_captured_once_replayed_twice_on_rewritten_shards(rceil):
    """the tables travel by value: one capture on one stream, two replays with the shard rewritten in between"""
    algo, side, total = t.SWING, 4, 16
    buckets, keys = unequal(total, seed=3)
    keys2 = [(tt, blk, seed + 50) for tt, blk, seed in keys]
    shards = Shards(buckets, "wide")
    shards.fill([cases(*k) for k in keys])
    args = shards.args()
    plan = any_plan(algo, side, total)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):   # an eager call first: nothing is loaded inside the capture
        plan.all_gather_shards_mxfp8(args, rceil=rceil, stream=s)
    s.synchronize()
    check_all(buckets, keys, rceil, "eager")
    for b in buckets:
        b.restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        with t.launch_trace() as tr:
            plan.all_gather_shards_mxfp8(args, rceil=rceil, stream=s)
    torch.cuda.synchronize()
    assert tr.kernels == [f"k_ag_group_mxfp8<{total}, {'true' if rceil else 'false'}>"]
    for b in buckets:
        b.check(b.host, "a capture runs nothing")
    for ks in (keys, keys2):
        shards.fill([cases(*k) for k in ks])
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        check_all(buckets, ks, rceil, "replay")
        shards_unchanged(shards)
    del g
    plan.close()


# ------------------------------------------------------------------ 5. rows beyond 2^32 bytes
def test_far_element_rows_and_far_scale_rows():
    """8x8 Swing, one bucket of one tile per block.  One arena, allocated and not filled: a 4 GiB front pad, 64
    element rows at a stride that puts the last row beyond 2^32 bytes, behind them 64 scale rows at the same
    stride.  Only a guard window around every payload row is initialised (to the sentinel) and compared: a row
    offset computed in 32 bits puts the payload somewhere else and leaves the window's payload sentinel."""
    algo, side, total = t.SWING, 8, 64
    n, G = 256 * total, far_arena.GUARD
    stride = far_arena.roundup(-(-(1 << 32) // (total - 1)), 16) + 16 * 17
    assert (total - 1) * stride > 1 << 32 and stride % 16 == 0
    rows_at = far_arena.FRONT + G
    scales_at = far_arena.roundup(rows_at + total * stride, G) + G
    nbytes = scales_at + total * stride + G
    arena = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    windows = [(at + r * stride, width) for at, width in ((rows_at, n), (scales_at, n // 32)) for r in range(total)]
    for a, width in windows:
        arena[a - G:a + width + G].fill_(SENT8)
    shard = f32t.to_dev32(cases(total, 256, 9).copy())
    args = [(arena.data_ptr() + rows_at, stride, arena.data_ptr() + scales_at, stride, n, shard.data_ptr(), 256)]
    plan = any_plan(algo, side, total)
    try:
        with t.tuned(pipe_grid=5):
            for rceil in (False, True):
                with t.launch_trace() as tr:
                    plan.all_gather_shards_mxfp8(args, rceil=rceil, stream=stream())
                torch.cuda.synchronize()
                assert tr.kernels == [f"k_ag_group_mxfp8<{total}, {'true' if rceil else 'false'}>"]
                we, ws = expected(total, 256, 9, rceil)
                for k, (a, width) in enumerate(windows):
                    got = arena[a - G:a + width + G].cpu().numpy()
                    want = np.full(width + 2 * G, SENT8, dtype=np.uint8)
                    want[G:G + width] = we if width == n else ws
                    assert np.array_equal(got, want), f"{'element' if k < total else 'scale'} row {k % total} (rceil={rceil})"
                    arena[a:a + width].fill_(SENT8)
        assert np.array_equal(shard.cpu().numpy().view(np.float32).view(np.uint32), cases(total, 256, 9).view(np.uint32))
    finally:
        plan.close()
        del arena
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 6. refusals, count == 0, rows in a gap
def test_refusals_leave_every_buffer_untouched():
    algo, side, total = t.SWING, 4, 8
    buckets, keys = unequal(total)
    shards = Shards(buckets, "compact")
    shards.fill([cases(*k) for k in keys])
    args = shards.args()
    s = stream()

    def refused(status, call):
        with pytest.raises(t.AllredError) as e:
            call()
        assert e.value.status == status, (e.value.status, status)

    def refused_everywhere(status, plan, lst):
        refused(status, lambda: plan.all_gather_shards_mxfp8(lst, stream=s))
        refused(status, lambda: plan.all_gather_shards_mxfp8(lst, rceil=True, stream=s))
        refused(status, lambda: plan.shards_mxfp8_launches(lst))

    for plan in (any_plan(algo, side, total, variant=t.LO), any_plan(algo, side, total, variant=t.MEM),
                 any_plan(algo, side, total, exec_mode=t.EXEC_STEPS)):
        refused_everywhere(_lib.ERR_UNSUPPORTED, plan, args)
        plan.close()
    p4 = t.Plan(t.SWING, t.BO, 2, 256 * 4, 4, t.EXEC_FUSED)   # no kernel form below 8 ranks
    a = args[0]
    refused_everywhere(_lib.ERR_UNSUPPORTED, p4, [(a[0], a[1], a[2], a[3], 256 * 4, a[5], 256)])
    p4.close()
    plan = any_plan(algo, side, total)
    rows, rs, scales, ss, n, shard, sst = args[1]
    blk = n // total
    rest = args[:1] + args[2:]
    part = (rows, rs, scales, ss, 8 * total * 3, shard, sst)   # not whole tiles: the whole list, wherever it stands
    refused_everywhere(_lib.ERR_UNSUPPORTED, plan, rest + [part])
    refused_everywhere(_lib.ERR_UNSUPPORTED, plan, [part] + rest)
    o = args[2]
    bad_lists = [
        rest + [(0, rs, scales, ss, n, shard, sst)],                    # NULL pointers
        rest + [(rows, rs, 0, ss, n, shard, sst)],
        rest + [(rows, rs, scales, ss, n, 0, sst)],
        rest + [(rows + 8, rs, scales, ss, n, shard, sst)],             # rows 8-byte aligned only
        rest + [(rows, rs, scales + 4, ss, n, shard, sst)],             # scales 4-byte aligned only
        rest + [(rows, rs, scales, ss, n, shard + 8, sst)],             # the shard 8-byte aligned only
        rest + [(rows, n - 16, scales, ss, n, shard, sst)],             # row_stride < n
        rest + [(rows, rs + 8, scales, ss, n, shard, sst)],             # row_stride % 16 != 0
        rest + [(rows, rs, scales, n // 32 - 8, n, shard, sst)],        # scale_stride < n / 32
        rest + [(rows, rs, scales, ss + 4, n, shard, sst)],             # scale_stride % 8 != 0
        rest + [(rows, rs, scales, ss, n, shard, blk - 4)],             # shard_stride < blk
        rest + [(rows, rs, scales, ss, n, shard, blk + 2)],             # shard_stride % 4 != 0
        rest + [(rows, rs, scales, ss, 0, shard, sst)],                 # an empty bucket
        rest + [(rows, rs, scales, ss, n + 8, shard, sst)],             # n % (8 total) != 0
        rest + [(rows, rs, rows, ss, n, shard, sst)],                   # scales on the bucket's own rows
        rest + [(rows, rs, rows + total * rs - 8, ss, n, shard, sst)],  # ... on the last 8 bytes of its row interval
        rest + [(rows, rs, o[0], ss, n, shard, sst)],                   # scales on another bucket's rows
        rest + [(rows, rs, o[2], ss, n, shard, sst)],                   # one scale buffer twice
        rest + [(o[0] + o[1], rs, scales, ss, n, shard, sst)],          # rows inside another bucket's rows
        rest + [(rows, rs, scales, ss, n, o[5], sst)],                  # one shard twice
        rest + [(rows, rs, scales, ss, n, rows, blk)],                  # the shard on the rows
        rest + [(rows, rs, shard + 4 * blk - 8, ss, n, shard, sst)],    # scales on the last 8 bytes of shard block 0
        rest + [(rows, rs, scales, ss, n, shard, 1 << 62)],             # address arithmetic that would overflow
        rest + [(rows, rs, scales, ss, n, shard, 1 << 63)],
        rest + [(rows, 1 << 62, scales, ss, n, shard, sst)],
        rest + [(rows, rs, scales, 1 << 62, n, shard, sst)],
    ]
    for bad in bad_lists:
        refused_everywhere(_lib.ERR_ARG, plan, bad)
    arr = (_lib.MxBucketF32 * len(args))(*args)
    lib = _lib.lib
    for flags in (2, 3, 0x100, -2):                                     # an unknown flag bit
        assert lib.allred_plan_all_gather_shards_mxfp8(plan._h, arr, len(args), flags, None) == _lib.ERR_ARG
        assert lib.allred_plan_all_gather_shards_mxfp8(plan._h, None, 0, flags, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8(plan._h, arr, -1, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8(plan._h, None, 2, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8(None, arr, len(args), 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8_launches(plan._h, arr, -1) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8_launches(plan._h, None, 2) == _lib.ERR_ARG
    # count == 0: OK, nothing launched
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp8([], stream=s)
        plan.all_gather_shards_mxfp8([], rceil=True, stream=s)
        assert lib.allred_plan_all_gather_shards_mxfp8(plan._h, None, 0, 1, None) == _lib.OK
    assert tr.count == 0 and plan.shards_mxfp8_launches([]) == 0
    # and the list itself is fine: the dry run accepts it without writing
    assert lib.allred_plan_all_gather_shards_mxfp8_launches(plan._h, arr, len(args)) == 1
    plan.close()
    for b in buckets:
        b.check(b.host, "written by a refused call")
    shards_unchanged(shards)


def test_rows_and_scales_inside_a_wide_strides_gap_are_accepted():
    """ONE buffer: 8 shard blocks of 256 floats at a stride of 256 + 4224 floats; the bucket's whole element-row
    interval (8 x 2048 bytes) and, right behind it, its scale-row interval (8 x 64 bytes) fill the gap behind
    block 0 exactly.  Accepted, and every byte of the buffer is what it must be."""
    algo, side, total = t.SWING, 4, 8
    n, blk = 256 * total, 256
    gap = total * n + total * (n // 32)
    sst = blk + gap // 4
    size = 4 * (total * sst + 64)
    x = cases(total, blk, 4)
    host = np.full(size, SENT8, dtype=np.uint8)
    for b in range(total):
        host[4 * b * sst:4 * (b * sst + blk)] = x[b].view(np.uint8)
    buf = to_dev8(host)
    rows, scales = buf.data_ptr() + 4 * blk, buf.data_ptr() + 4 * blk + total * n
    args = [(rows, n, scales, n // 32, n, buf.data_ptr(), sst)]
    plan = any_plan(algo, side, total)
    assert plan.shards_mxfp8_launches(args) == 1
    plan.all_gather_shards_mxfp8(args, rceil=True, stream=stream())
    torch.cuda.synchronize()
    we, ws = expected(total, blk, 4, True)
    want = host.copy()
    want[4 * blk:4 * blk + total * n] = np.tile(we, total)
    want[4 * blk + total * n:4 * blk + gap] = np.tile(ws, total)
    assert np.array_equal(buf.cpu().numpy(), want)
    # one byte-quantum off either way: on block 0's tail, or on block 1's head
    for bad in [(rows - 16, n, scales, n // 32, n, buf.data_ptr(), sst), (rows, n, scales + 8, n // 32, n, buf.data_ptr(), sst)]:
        with pytest.raises(t.AllredError) as e:
            plan.all_gather_shards_mxfp8([bad], stream=stream())
        assert e.value.status == _lib.ERR_ARG
    plan.close()
    assert np.array_equal(buf.cpu().numpy(), want)
