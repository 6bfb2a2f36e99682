"""allred_plan_adamw_all_gather_shards_mxfp8 / allred_plan_adamw_shards_mxfp8_launches
(k_adamw_ag_mxfp8): AdamW with parameter groups inside the MXFP8 all-gather's launch.

Expectations: tests/adamw_mx_ref.py — adamw_ref.step with eff(group_of[i]) of tests/adamw_groups_cases.py,
then mxfp8_ref.quantize of the new param plane (of p on a skipped step) — on the data of
tests/adamw_mx_cases.py, compared BIT FOR BIT: the planes fp32 as uint32, NaNs by class; element and scale
bytes exactly.  Identity buckets carry the 24 planted MX blocks of tests/mx_cases.py through the update
path, update buckets are tests/adamw_cases.py's; tests/test_adamw_mx_ref.py pins that an amax over fewer
than 32 elements, the old parameters or a bf16 in between change these bytes.

Buffers: every bucket's element rows and scale rows in buffers of their own with skew and a guard row =
sentinel (test_gpu_shards_mxfp8.MxBucket), the four fp32 planes sentinel-filled with a guard behind each —
compact, wide and flat (test_gpu_shards_f32.Shards) —, the hyper array, norm_sq and info in one small
sentinel-filled buffer (test_gpu_adamw_groups.SmallG).  WHOLE buffers are compared."""
import ctypes as C
import functools

import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_mx_cases as mc
import f32_norm
import f32_tree
import far_arena
import mxfp8_ref as ref
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_adamw_groups as groups  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_shards_mxfp8 as mxt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT8 = mxt.SENT8
stream = base.stream
SmallG = groups.SmallG
P_, G_, M_, V_ = range(4)
FLAGS = mc.FLAGS
flag_pairs = pytest.mark.parametrize("zero,rceil", FLAGS, ids=[f"zero{int(z)}-rceil{int(r)}" for z, r in FLAGS])


def tf(x):
    return "true" if x else "false"


def kernel(total, zero, rceil):
    return f"k_adamw_ag_mxfp8<{total}, {tf(zero)}, {tf(rceil)}>"


def mx_buckets(total, tiles):
    """element and scale rows in buffers of their own, every other bucket with stride skews"""
    return [mxt.MxBucket(total, 256 * total * k, skew=i % 2 == 1) for i, k in enumerate(tiles)]


class Planes(one.Planes):
    """the four fp32 planes of a list of MxBuckets: test_gpu_adamw_shards.Planes with this call's bucket tuple"""

    def args(self):
        out = []
        for i, b in enumerate(self.buckets):
            a = [self.s[k].arg(i) for k in range(4)]
            out.append(b.arg + tuple(x[-2] for x in a) + (a[0][-1],))
        return out


def check_all(buckets, planes, small, want, what):
    values, rows, info = want
    planes.check(values, what)
    for i, (b, (e, s)) in enumerate(zip(buckets, rows)):
        b.check(b.after(e, s), f"bucket {i} (n={b.n}): rows = mxfp8(p'): {what}")
    small.check(info, what)


@functools.lru_cache(maxsize=None)
def list_data(total, seed):
    return mc.make(total, seed)


@functools.lru_cache(maxsize=None)
def list_want(total, seed, zero, rceil):
    """the expectation of the LIST at (total, seed), computed once per flag pair"""
    return mc.expect(list_data(total, seed), mc.GROUP_OF, adamw_cases.norm_sq(total), total, zero, rceil)


# ------------------------------------------------------------------ 1. the step, every schedule, layout, grid and flag pair
@base.grids
@base.layouts
@base.sched
def test_step_and_mxfp8_all_gather(algo, side, total, layout, grid):
    """adamw_mx_cases.LIST — identity buckets of blk = 256 and 768 in group 1, update buckets of blk = 256 and 768
    in groups 0 and 2 — for all four flag pairs: p' m' v' (and g with zero_grad) bit for bit, every rank's
    element row and scale row = mxfp8(p'), gaps, guards, skew and the small buffer's sentinels unchanged;
    clipping by group 0's max_norm active; one launch.  At pipe_grid 5 every workgroup walks several tiles."""
    buckets = mx_buckets(total, mc.TILES)
    data = list_data(total, 10 * total)
    planes = Planes(buckets, layout, data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    plan = base.any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.adamw_shards_mxfp8_launches(planes.args()) == 1
        for zero, rceil in FLAGS:
            planes.restore()
            small.restore()
            with t.launch_trace() as tr:
                plan.adamw_all_gather_shards_mxfp8(planes.args(), mc.GROUP_OF, small.hyper, 3, small.norm_sq, small.info,
                                                   zero_grad=zero, rceil=rceil, stream=stream())
            assert tr.kernels == [kernel(total, zero, rceil)]
            if grid:
                assert tr.grids == [grid] and total * sum(mc.TILES) >= 3 * grid
            want = list_want(total, 10 * total, zero, rceil)
            assert want[2][1] < 1 and want[2][2] == 0   # clipping is active, the step is not skipped
            check_all(buckets, planes, small, want, f"zero_grad={zero}, rceil={rceil}")
    plan.close()


# ------------------------------------------------------------------ 2. the guarantee
GUARANTEE_LIST = ((1, "identity", 1), (3, "negative_v", 0), (2, "zero_den", 2), (3, "planes", 0), (1, "planes", 2))


@pytest.mark.parametrize("algo,side,total", [(t.SWING, 4, 8), (t.SWING, 8, 64)], ids=["swing-8", "swing-8x8"])
@flag_pairs
def test_planes_of_the_groups_call_rows_of_the_mxfp8_all_gather(algo, side, total, zero, rceil):
    """allred.h's guarantee: on the same inputs the four planes are bit for bit those
    allred_plan_adamw_all_gather_shards_f32_groups leaves (its bf16 rows go to buffers nobody compares), and the
    element and scale rows are bit for bit what allred_plan_all_gather_shards_mxfp8 writes from the param plane
    that call leaves.  p' is NaN in places (negative_v, zero_den): those blocks are 0xFF / 0x7F in both."""
    tiles = tuple(k for k, _, _ in GUARANTEE_LIST)
    group_of = tuple(g for _, _, g in GUARANTEE_LIST)
    buckets, second = mx_buckets(total, tiles), mx_buckets(total, tiles)
    rows16 = one.rows_buckets(total, tiles)
    data = mc.make(total, 200 + total, GUARANTEE_LIST)
    planes = Planes(buckets, "flat", data)
    nsq = adamw_cases.norm_sq(total)
    small, small2 = SmallG(gc.hyper_array(), nsq), SmallG(gc.hyper_array(), nsq)
    args = planes.args()
    plan = base.any_plan(algo, side, total)
    plan.adamw_all_gather_shards_mxfp8(args, group_of, small.hyper, 3, small.norm_sq, small.info, zero_grad=zero, rceil=rceil, stream=stream())
    check_all(buckets, planes, small, mc.expect(data, group_of, nsq, total, zero, rceil), "the numpy expectation")
    new = [g.copy() for s in planes.s for g in s.got()]
    new_rows = [b.got() for b in buckets]
    new_info = groups.info_words(small)
    planes.restore()
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32_groups([r.arg + a[5:] for r, a in zip(rows16, args)], group_of, small2.hyper, 3, small2.norm_sq,
                                                small2.info, zero_grad=zero, stream=stream())
        plan.all_gather_shards_mxfp8([b.arg + (a[5], a[9]) for b, a in zip(second, args)], rceil=rceil, stream=stream())
    assert tr.kernels == [f"k_adamw_ag_groups_f32<{total}, {tf(zero)}>", f"k_ag_group_mxfp8<{total}, {tf(rceil)}>"]
    old = [g.copy() for s in planes.s for g in s.got()]
    assert len(new) == len(old)
    for k, (a, b) in enumerate(zip(new, old)):
        assert f32_tree.same_f32(a.view(np.float32), b.view(np.float32)), f"plane buffer {k}"
    for i, (a, b) in enumerate(zip(new_rows, [b.got() for b in second])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"bucket {i}: rows and scales"
    assert np.array_equal(new_info, groups.info_words(small2))
    assert all((r[1][:total, :b.n // 32] == 0xFF).any() for r, b in zip(new_rows[:2], buckets))   # NaN blocks went through both
    assert not np.array_equal(new[0], planes.s[P_].host[0])   # something was computed
    plan.close()


# ------------------------------------------------------------------ 3. the call-wide values
@pytest.mark.parametrize("case", list(one.uniform_cases(64)))
def test_call_wide_values(case):
    """test_gpu_adamw_shards.uniform_cases with the case's set as group 0: norm_sq NULL (c == 1), +Inf max_norm,
    clipping, no clipping, N = +0, and N = +Inf / NaN — the skipped step: every group's state bit-equal to
    before, the rows the quantisation of p, grad zeroed only with the flag, info[2] = 1."""
    algo, side, total = t.SWING, 8, 64
    hyper0, nsq = one.uniform_cases(total)[case]
    grps = (hyper0, gc.GROUPS[1], gc.GROUPS[2])
    lst = ((1, "planes", 2), (2, "identity", 1), (1, "planes", 0))
    group_of = tuple(g for _, _, g in lst)
    buckets = mx_buckets(total, tuple(k for k, _, _ in lst))
    data = mc.make(total, 7, lst)
    planes = Planes(buckets, "wide", data)
    small = SmallG(gc.hyper_array(3, grps), nsq)
    plan = base.any_plan(algo, side, total)
    for zero, rceil in FLAGS:
        planes.restore()
        small.restore()
        plan.adamw_all_gather_shards_mxfp8(planes.args(), group_of, small.hyper, 3, small.norm_sq, small.info, zero_grad=zero,
                                           rceil=rceil, stream=stream())
        want = mc.expect(data, group_of, nsq, total, zero, rceil, grps)
        info = want[2]
        if case in ("N-inf", "N-nan"):
            assert info[2] == 1
            for d, v, (e, s) in zip(data, want[0], want[1]):
                assert all(np.array_equal(v[k].view(np.uint32), d[k].view(np.uint32)) for k in (P_, M_, V_))
                we, ws = ref.expected_rows(d[P_], rceil)
                assert np.array_equal(e, we) and np.array_equal(s, ws)
                assert (v[G_].view(np.uint32) == 0).all() if zero else np.array_equal(v[G_].view(np.uint32), d[G_].view(np.uint32))
        else:
            assert info[2] == 0 and (info[1] < 1) == (case == "clip") and (info[1] == 1) == (case != "clip")
        if case == "no-norm":
            assert info[0] == 0 and info[1] == 1
        check_all(buckets, planes, small, want, f"{case}, zero_grad={zero}, rceil={rceil}")
    plan.close()


# ------------------------------------------------------------------ 4. launches
@pytest.mark.parametrize("count,launches", [(32, 1), (33, 2), (65, 3)])
def test_32_buckets_per_launch_whatever_the_groups(count, launches):
    """one-tile buckets, bucket i in group i % 3 (group 1: identity buckets): launch boundaries at 32 and 64 fall on
    every group in turn; info is written once, by the first launch."""
    algo, side, total = t.SWING, 4, 8
    lst = tuple((1, "identity" if i % 3 == 1 else "planes", i % 3) for i in range(count))
    group_of = [g for _, _, g in lst]
    buckets = [mxt.MxBucket(total, 256 * total, skew=i % 3 == 0) for i in range(count)]
    data = mc.make(total, 100, lst)
    planes = Planes(buckets, "flat", data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    plan = base.any_plan(algo, side, total)
    assert plan.adamw_shards_mxfp8_launches(planes.args()) == launches
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_mxfp8(planes.args(), group_of, small.hyper, 3, small.norm_sq, small.info, zero_grad=True, rceil=True,
                                           stream=stream())
    assert tr.count == launches and tr.kernels == [kernel(total, True, True)] * launches
    check_all(buckets, planes, small, mc.expect(data, group_of, nsq, total, True, True), f"{count} buckets")
    plan.close()


# ------------------------------------------------------------------ 5. one capture, three steps
def test_one_capture_replayed_as_three_steps():
    """the hyper array travels through device memory: between replays all three sets (another lr per group and step,
    the step's bias corrections), norm_sq and the gradient planes are rewritten by stream-ordered copies on the
    capture's stream; three replays = three numpy steps, the rows the quantisation of each step's p'."""
    algo, side, total = t.SWING, 4, 16
    lst = ((1, "planes", 0), (3, "planes", 1), (2, "planes", 2), (3, "planes", 1))
    group_of = tuple(g for _, _, g in lst)
    buckets = mx_buckets(total, tuple(k for k, _, _ in lst))
    data = mc.make(total, 51, lst)
    planes = Planes(buckets, "flat", data)
    lrs = (1e-3, 3e-4, 2e-3)
    steps = [tuple(adamw_cases.hyper(step=k, lr=lrs[g] / k, betas=((0.9, 0.999), (0.8, 0.99), (0.95, 0.95))[g],
                                     eps=(1e-8, 1e-6, 1e-10)[g], weight_decay=(0.01, 0.0, 0.1)[g], max_norm=(1.0, 1e-3, float("inf"))[g])
                   for g in range(3)) for k in (1, 2, 3)]
    grads = [[adamw_cases.planes(60 + 10 * k + i, (b.total, b.blk))[G_] for i, b in enumerate(buckets)] for k in range(3)]
    nsqs = [adamw_cases.norm_sq(total, seed=k) for k in range(3)]
    small = SmallG(gc.hyper_array(3, steps[0]), nsqs[0])
    small_dev, grad_dev = [], []
    for k in range(3):
        small_dev.append(base.to_dev32(SmallG(gc.hyper_array(3, steps[k]), nsqs[k]).host))
        grad_dev.append([base.to_dev32(h) for h in planes.s[G_].expected(grads[k])])
    plan = base.any_plan(algo, side, total)
    args = planes.args()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # an eager call first: the capture loads no code
        plan.adamw_all_gather_shards_mxfp8(args, group_of, small.hyper, 3, small.norm_sq, small.info, rceil=True, stream=s)
    s.synchronize()
    planes.restore()
    small.restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        with t.launch_trace() as tr:
            plan.adamw_all_gather_shards_mxfp8(args, group_of, small.hyper, 3, small.norm_sq, small.info, rceil=True, stream=s)
    torch.cuda.synchronize()
    assert tr.kernels == [kernel(total, False, True)]
    planes.check(data, "a capture runs nothing")
    for b in buckets:
        b.check(b.host, "a capture runs nothing")
    state = data
    for k in range(3):
        with torch.cuda.stream(s):
            small.buf.copy_(small_dev[k], non_blocking=True)
            for d, src in zip(planes.s[G_].buf, grad_dev[k]):
                d.copy_(src, non_blocking=True)
            g.replay()
        s.synchronize()
        cur = [(st[P_], gi, st[M_], st[V_]) for st, gi in zip(state, grads[k])]
        want = mc.expect(cur, group_of, nsqs[k], total, False, True, steps[k])
        small.host = SmallG(gc.hyper_array(3, steps[k]), nsqs[k]).host
        check_all(buckets, planes, small, want, f"replay {k + 1}")
        state = want[0]
    del g
    plan.close()


# ------------------------------------------------------------------ 6. a side stream behind late inputs
def test_on_a_side_stream_behind_late_inputs():
    """every plane holds NaN bits and the small buffer the sentinel until, on the side stream and behind a few
    milliseconds of fills, the data arrives; the call is enqueued right behind it on that stream and only that
    stream is waited for"""
    algo, side, total = t.SWING, 4, 16
    buckets = mx_buckets(total, mc.TILES)
    data = list_data(total, 3)
    planes = Planes(buckets, "flat", data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    staged = [[base.to_dev32(h) for h in s.host] for s in planes.s]
    staged_small = base.to_dev32(small.host)
    scratch = torch.empty(1 << 28, dtype=torch.uint8, device=DEV)
    plan = base.any_plan(algo, side, total)
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        for b in buckets:
            b.restore()
        for pl in planes.s:
            for d in pl.buf:
                d.fill_(0x7FC00000)
        small.buf.fill_(0x7FC00000)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for i in range(16):
                scratch.fill_(i)
            for pl, st in zip(planes.s, staged):
                for d, h in zip(pl.buf, st):
                    d.copy_(h, non_blocking=True)
            small.buf.copy_(staged_small, non_blocking=True)
            plan.adamw_all_gather_shards_mxfp8(planes.args(), mc.GROUP_OF, small.hyper, 3, small.norm_sq, small.info, zero_grad=True,
                                               stream=s)
        s.synchronize()
        check_all(buckets, planes, small, list_want(total, 3, True, False), "on a side stream behind late inputs")
    del scratch
    plan.close()


# ------------------------------------------------------------------ 7. rows beyond 2^32 bytes
def test_far_element_rows_and_far_scale_rows():
    """test_gpu_shards_mxfp8's arena — allocated and not filled: a 4 GiB front pad, 64 element rows at a stride that
    puts the last row beyond 2^32 bytes, behind them 64 scale rows at the same stride — with one identity bucket of
    one tile per block, 8x8 Swing, pipe_grid 5.  Only a guard window around every payload row is initialised and
    compared: a row offset computed in 32 bits leaves the window's payload sentinel."""
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

    class Far:   # what Shards needs of a bucket
        pass
    fb = Far()
    fb.total, fb.n, fb.blk = total, n, 256
    fb.arg = (arena.data_ptr() + rows_at, stride, arena.data_ptr() + scales_at, stride, n)
    fb.restore = lambda: None
    lst = ((1, "identity", 1),)
    data = mc.make(total, 9, lst)
    planes = Planes([fb], "compact", data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(2), nsq)
    plan = base.any_plan(algo, side, total)
    try:
        with t.tuned(pipe_grid=5):
            for zero, rceil in ((False, False), (True, True)):
                planes.restore()
                small.restore()
                with t.launch_trace() as tr:
                    plan.adamw_all_gather_shards_mxfp8(planes.args(), (1,), small.hyper, 2, small.norm_sq, small.info, zero_grad=zero,
                                                       rceil=rceil, stream=stream())
                torch.cuda.synchronize()
                assert tr.kernels == [kernel(total, zero, rceil)]
                values, rows, info = mc.expect(data, (1,), nsq, total, zero, rceil)
                we, ws = rows[0]
                for k, (a, width) in enumerate(windows):
                    got = arena[a - G:a + width + G].cpu().numpy()
                    want = np.full(width + 2 * G, SENT8, dtype=np.uint8)
                    want[G:G + width] = we if width == n else ws
                    assert np.array_equal(got, want), f"{'element' if k < total else 'scale'} row {k % total} (rceil={rceil})"
                    arena[a:a + width].fill_(SENT8)
                planes.check(values, f"far rows, zero_grad={zero}")
                small.check(info, "far rows")
    finally:
        plan.close()
        del arena
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 8. the two-launch step end to end
@pytest.mark.parametrize("algo,side,total", [(t.SWING, 8, 64), (t.RECDUB, 4, 16)], ids=["swing-8x8", "recdub-4x4"])
def test_reduce_scatter_with_norm_then_adamw_mxfp8(algo, side, total):
    """the MXFP8 step in two launches: reduce_scatter_shards_f32_norm into the gradient planes, then the new call
    with its norm_sq and TWO groups, on hard_inputs.cancel, against the composed numpy expectation."""
    import test_gpu_shards_f32_norm as norm_base
    grads = base.unequal(algo, side, total, seed=11)          # their rows: the gradients, kept
    params = mx_buckets(total, base.UNEQUAL)                  # the parameter rows, written
    data = one.make_data(params, 41)
    planes = Planes(params, "flat", data)
    scale = 1.0 / total
    rs_args = [g.arg + (a[6], a[9]) for g, a in zip(grads, planes.args())]
    plan = base.any_plan(algo, side, total)
    norm = norm_base.Norm(plan, rs_args, total)
    grps = (adamw_cases.hyper(max_norm=0.25), gc.GROUPS[1])
    group_of = (1, 0, 0, 1)
    small = SmallG(gc.hyper_array(2, grps))
    with t.tuned(pipe_grid=5), t.launch_trace() as tr:
        plan.reduce_scatter_shards_f32_norm(rs_args, norm.sq_ptr, norm.ws_ptr, scale, stream=stream())
        plan.adamw_all_gather_shards_mxfp8(planes.args(), group_of, small.hyper, 2, norm.sq_ptr, small.info, zero_grad=True, rceil=True,
                                           stream=stream())
    assert tr.kernels == [f"k_tree_group_f32_norm<{total}, false>", kernel(total, True, True)]
    g = [f32_tree.scaled(b.sums, scale) for b in grads]
    nsq = f32_norm.expect_norm_sq(g)
    norm.check(nsq, "the reduce-scatter's norm")
    want = mc.expect([(d[P_], gi, d[M_], d[V_]) for d, gi in zip(data, g)], group_of, nsq, total, True, True, grps)
    assert want[2][1] < 1 and want[2][2] == 0
    check_all(params, planes, small, want, "the two-launch step")
    base.check_buckets(grads, [b.host for b in grads], "the gradient rows are only read")
    plan.close()


# ------------------------------------------------------------------ 9. refusals
def test_refusals_leave_every_buffer_untouched():
    algo, side, total = t.SWING, 4, 8
    buckets = mx_buckets(total, mc.TILES)
    data = list_data(total, 71)
    planes = Planes(buckets, "wide", data)
    small = SmallG(gc.hyper_array(), adamw_cases.norm_sq(total))
    args = planes.args()
    s = stream()
    lib = _lib.lib
    GROUP_OF = mc.GROUP_OF

    def status(plan, lst, group_of=GROUP_OF, hyper=small.hyper, ngroups=3, norm_sq=small.norm_sq, info=small.info, flags=0):
        arr, count = t.Plan._adamw_mx_buckets_f32(lst)
        grp = None if group_of is None else (C.c_uint8 * max(len(group_of), 1))(*group_of)
        return lib.allred_plan_adamw_all_gather_shards_mxfp8(plan._h if plan else None, arr, grp, count, hyper or None, ngroups,
                                                             norm_sq or None, info or None, flags, None)

    def refused(want, plan, lst, **kw):
        for flags in (0, 1, 2, 3):
            assert status(plan, lst, flags=flags, **kw) == want, (flags, kw)
        with pytest.raises(t.AllredError) as e:
            plan.adamw_all_gather_shards_mxfp8(lst, kw.get("group_of", GROUP_OF), kw.get("hyper", small.hyper), kw.get("ngroups", 3),
                                               kw.get("norm_sq", small.norm_sq), kw.get("info", small.info), stream=s)
        assert e.value.status == want

    def refused_dry(want, plan, lst):
        with pytest.raises(t.AllredError) as e:
            plan.adamw_shards_mxfp8_launches(lst)
        assert e.value.status == want

    plan = base.any_plan(algo, side, total)
    hy, sq, info = small.hyper, small.norm_sq, small.info
    rows, rs, scales, ss, n, pp, gp, mp, vp, sst = args[1]
    blk = n // total
    rest = args[:1] + args[2:]
    # --- the group rules
    for ng in (0, 9, -1, 256):
        refused(_lib.ERR_ARG, plan, args, ngroups=ng, group_of=(0, 0, 0, 0))
        refused(_lib.ERR_ARG, plan, args, ngroups=ng, group_of=None)
        assert status(plan, [], ngroups=ng, group_of=None) == _lib.ERR_ARG        # an empty list too
    for ng in (1, 2, 3):
        for where in range(4):                                                    # a group index equal to ngroups
            bad = [0, 0, 0, 0]
            bad[where] = ng
            refused(_lib.ERR_ARG, plan, args, ngroups=ng, group_of=tuple(bad))
    # --- hyper, norm_sq and info
    for d in (4, 8):
        refused(_lib.ERR_ARG, plan, args, hyper=hy + d)
        assert status(plan, [], hyper=hy + d) == _lib.ERR_ARG
    refused(_lib.ERR_ARG, plan, args, hyper=0)
    assert status(plan, [], hyper=0) == _lib.ERR_ARG
    refused(_lib.ERR_ARG, plan, args, info=hy + 64 + 16)                          # info inside the LAST group's 32 bytes
    refused(_lib.ERR_ARG, plan, args, norm_sq=hy + 92)                            # norm_sq on the last group's last float
    gap = pp + 4 * blk   # the 256-byte gap behind block 0 of bucket 1's param plane (wide layout)
    refused(_lib.ERR_ARG, plan, args, hyper=gap - 64)                             # the first two sets on block 0's tail
    refused(_lib.ERR_ARG, plan, args, hyper=gap + 256 - 64)                       # the third set alone on block 1's head
    refused(_lib.ERR_ARG, plan, args, hyper=rows + n - 48)                        # the second set on the last bytes of an element row
    refused(_lib.ERR_ARG, plan, args, hyper=scales + total * ss - 80)             # the third set on the last bytes of the scale rows
    pointer_cases = {   # refused whatever the list, an empty one included
        "norm_sq 2-byte aligned": dict(norm_sq=sq + 2), "info 8-byte aligned": dict(info=info + 8),
        "an unknown flag bit": dict(flags=4), "flags 7": dict(flags=7), "flags -2": dict(flags=-2), "flags 0x100": dict(flags=0x100),
        "info inside the first group": dict(info=hy + 16), "info on norm_sq": dict(info=sq + 16),
    }
    overlap_cases = {   # refused against this list
        "info on an element row": dict(info=rows + rs), "info on the last bytes of the scale rows": dict(info=scales + total * ss - 16),
        "hyper inside a plane block": dict(hyper=gp + 64), "norm_sq on a plane's last float": dict(norm_sq=vp + 4 * blk - 4),
        "info on the first bytes of a plane block": dict(info=mp + 4 * sst), "norm_sq on a scale row": dict(norm_sq=scales + 8),
    }
    for what, kw in pointer_cases.items():
        assert status(plan, args, **kw) == _lib.ERR_ARG and status(plan, [], **kw) == _lib.ERR_ARG, what
    for what, kw in overlap_cases.items():
        assert status(plan, args, **kw) == _lib.ERR_ARG, what
    # --- the plan
    for other in (base.any_plan(algo, side, total, variant=t.LO), base.any_plan(algo, side, total, variant=t.MEM),
                  base.any_plan(algo, side, total, exec_mode=t.EXEC_STEPS)):
        refused(_lib.ERR_UNSUPPORTED, other, args)
        refused_dry(_lib.ERR_UNSUPPORTED, other, args)
        other.close()
    p4 = t.Plan(t.SWING, t.BO, 2, 256 * 4, 4, t.EXEC_FUSED)   # no kernel form below 8 ranks
    a0 = args[0]
    small4 = [a0[:4] + (256 * 4,) + a0[5:9] + (256,)]
    refused(_lib.ERR_UNSUPPORTED, p4, small4, group_of=(1,))
    refused_dry(_lib.ERR_UNSUPPORTED, p4, small4)
    p4.close()
    part = (rows, rs, scales, ss, 8 * total * 3, pp, gp, mp, vp, sst)   # not whole tiles: the whole list, wherever it stands
    for lst in (rest + [part], [part] + rest):
        refused(_lib.ERR_UNSUPPORTED, plan, lst)
        refused_dry(_lib.ERR_UNSUPPORTED, plan, lst)
    # --- the list
    o = args[2]
    bad_lists = [
        rest + [(0, rs, scales, ss, n, pp, gp, mp, vp, sst)],                     # NULL pointers
        rest + [(rows, rs, 0, ss, n, pp, gp, mp, vp, sst)],
        rest + [(rows, rs, scales, ss, n, 0, gp, mp, vp, sst)], rest + [(rows, rs, scales, ss, n, pp, 0, mp, vp, sst)],
        rest + [(rows, rs, scales, ss, n, pp, gp, 0, vp, sst)], rest + [(rows, rs, scales, ss, n, pp, gp, mp, 0, sst)],
        rest + [(rows + 8, rs, scales, ss, n, pp, gp, mp, vp, sst)],              # rows 8-byte aligned only
        rest + [(rows, rs, scales + 4, ss, n, pp, gp, mp, vp, sst)],              # scales 4-byte aligned only
        rest + [(rows, rs, scales, ss, n, pp + 4, gp, mp, vp, sst)], rest + [(rows, rs, scales, ss, n, pp, gp + 8, mp, vp, sst)],
        rest + [(rows, rs, scales, ss, n, pp, gp, mp + 4, vp, sst)], rest + [(rows, rs, scales, ss, n, pp, gp, mp, vp + 8, sst)],
        rest + [(rows, n - 16, scales, ss, n, pp, gp, mp, vp, sst)],              # row_stride < n
        rest + [(rows, rs + 8, scales, ss, n, pp, gp, mp, vp, sst)],              # row_stride % 16 != 0
        rest + [(rows, rs, scales, n // 32 - 8, n, pp, gp, mp, vp, sst)],         # scale_stride < n / 32
        rest + [(rows, rs, scales, ss + 4, n, pp, gp, mp, vp, sst)],              # scale_stride % 8 != 0
        rest + [(rows, rs, scales, ss, n, pp, gp, mp, vp, blk - 4)],              # shard_stride < blk
        rest + [(rows, rs, scales, ss, n, pp, gp, mp, vp, blk + 2)],              # shard_stride % 4 != 0
        rest + [(rows, rs, scales, ss, 0, pp, gp, mp, vp, sst)],                  # an empty bucket
        rest + [(rows, rs, scales, ss, n + 8, pp, gp, mp, vp, sst)],              # n % (8 total) != 0
        rest + [(rows, rs, rows, ss, n, pp, gp, mp, vp, sst)],                    # scales on the bucket's own rows
        rest + [(rows, rs, o[0], ss, n, pp, gp, mp, vp, sst)],                    # scales on another bucket's rows
        rest + [(rows, rs, o[2], ss, n, pp, gp, mp, vp, sst)],                    # one scale buffer twice
        rest + [(o[0] + o[1], rs, scales, ss, n, pp, gp, mp, vp, sst)],           # rows inside another bucket's rows
        rest + [(rows, rs, scales, ss, n, pp, pp, mp, vp, sst)],                  # param == grad
        rest + [(rows, rs, scales, ss, n, pp, gp, mp, o[8], sst)],                # another bucket's exp_avg_sq
        rest + [(rows, rs, o[8] + 4 * (o[4] // total) - 8, ss, n, pp, gp, mp, vp, sst)],   # scales on the last 8 bytes of block 0 of bucket 2's exp_avg_sq
        rest + [(rows, rs, scales, ss, n, pp, gp, mp, rows, blk)],                # a plane on the rows
        rest + [(rows, rs, scales, ss, n, pp, gp, mp, vp, 1 << 62)],              # address arithmetic that would overflow
        rest + [(rows, rs, scales, ss, n, pp, gp, mp, vp, 1 << 63)],
        rest + [(rows, 1 << 62, scales, ss, n, pp, gp, mp, vp, sst)],
        rest + [(rows, rs, scales, 1 << 62, n, pp, gp, mp, vp, sst)],
    ]
    for bad in bad_lists:
        refused(_lib.ERR_ARG, plan, bad)
        refused_dry(_lib.ERR_ARG, plan, bad)
    assert status(None, args) == _lib.ERR_ARG
    arr, count = t.Plan._adamw_mx_buckets_f32(args)
    call = lib.allred_plan_adamw_all_gather_shards_mxfp8
    assert call(plan._h, arr, None, -1, hy, 3, None, None, 0, None) == _lib.ERR_ARG
    assert call(plan._h, None, None, 2, hy, 3, None, None, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_adamw_shards_mxfp8_launches(plan._h, arr, -1) == _lib.ERR_ARG
    assert lib.allred_plan_adamw_shards_mxfp8_launches(plan._h, None, 2) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        plan.adamw_all_gather_shards_mxfp8(args, (0, 1), hy, 3, sq, info, stream=s)   # two indices for four buckets
    # count == 0: OK after the pointer and ngroups checks, nothing launched, info not written
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_mxfp8([], None, hy, 3, sq, info, zero_grad=True, rceil=True, stream=s)
        plan.adamw_all_gather_shards_mxfp8([], [], hy, 8, sq, info, stream=s)
        assert status(plan, [], group_of=None, norm_sq=0, info=0, flags=3) == _lib.OK
    assert tr.count == 0 and plan.adamw_shards_mxfp8_launches([]) == 0
    # and the list itself is fine: the dry run accepts it without writing
    assert plan.adamw_shards_mxfp8_launches(args) == 1
    plan.close()
    planes.check(data, "written by a refused call")
    for b in buckets:
        b.check(b.host, "rows written by a refused call")
    small.check(None, "written by a refused call")


# ------------------------------------------------------------------ 10. everything in a gap
def test_rows_scales_and_the_small_buffers_fill_a_stride_gap_exactly():
    """ONE buffer holds the param plane — 8 blocks of 256 floats at a stride of 256 + 4260 floats — and, in the gap
    of 17040 bytes behind block 0, the bucket's element-row interval (8 x 2048), its scale-row interval (8 x 64),
    three hyper sets (96), norm_sq (32) and info (16), filling it exactly.  Accepted, and every byte of the buffer
    is what it must be; rows or scales one quantum off, or a fourth hyper set, are refused."""
    algo, side, total = t.SWING, 4, 8
    n, blk = 256 * total, 256
    gap = total * n + total * (n // 32) + 96 + 4 * total + 16
    assert gap == 17040
    sst = blk + gap // 4
    size = 4 * (total * sst + 64)
    nsq = adamw_cases.norm_sq(total)
    lst = ((1, "planes", 2),)
    data = mc.make(total, 4, lst)
    p = data[0][P_]
    host = np.full(size, SENT8, dtype=np.uint8)
    for b in range(total):
        host[4 * b * sst:4 * (b * sst + blk)] = p[b].view(np.uint8)
    rows_at = 4 * blk
    scales_at, hyper_at = rows_at + total * n, rows_at + total * n + total * (n // 32)
    norm_at, info_at = hyper_at + 96, hyper_at + 96 + 4 * total
    assert info_at + 16 == 4 * sst
    host[hyper_at:norm_at] = gc.hyper_array().reshape(-1).view(np.uint8)
    host[norm_at:info_at] = nsq.view(np.uint8)
    buf = mxt.to_dev8(host)
    at = buf.data_ptr()
    # every plane at ONE stride: the other three are buffers of their own at the same wide stride
    wide_host = []
    for k in (G_, M_, V_):
        w = np.full(total * sst, base.SENT32, dtype=np.uint32)
        for b in range(total):
            w[b * sst:b * sst + blk] = np.ascontiguousarray(data[0][k][b]).view(np.uint32)
        wide_host.append(w)
    wide = [base.to_dev32(w) for w in wide_host]
    args = [(at + rows_at, n, at + scales_at, n // 32, n, at) + tuple(w.data_ptr() for w in wide) + (sst,)]
    plan = base.any_plan(algo, side, total)
    assert plan.adamw_shards_mxfp8_launches(args) == 1
    for bad, kw in [([(at + rows_at - 16,) + args[0][1:]], {}), ([args[0][:2] + (at + scales_at + 8,) + args[0][3:]], {}),
                    (args, dict(ngroups=4)), (args, dict(info=at + info_at + 16)), (args, dict(norm_sq=at + norm_at - 4))]:
        with pytest.raises(t.AllredError) as e:
            plan.adamw_all_gather_shards_mxfp8(bad, (2,), at + hyper_at, kw.get("ngroups", 3), kw.get("norm_sq", at + norm_at),
                                               kw.get("info", at + info_at), stream=stream())
        assert e.value.status == _lib.ERR_ARG
    assert np.array_equal(buf.cpu().numpy(), host)
    for w, h in zip(wide, wide_host):
        assert np.array_equal(w.cpu().numpy().view(np.uint32), h)
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_mxfp8(args, (2,), at + hyper_at, 3, at + norm_at, at + info_at, rceil=True, stream=stream())
    torch.cuda.synchronize()
    assert tr.kernels == [kernel(total, False, True)]
    values, rowsw, info = mc.expect(data, (2,), nsq, total, False, True)
    want = host.copy()
    for b in range(total):
        want[4 * b * sst:4 * (b * sst + blk)] = values[0][P_][b].view(np.uint8)
    want[rows_at:scales_at] = np.tile(rowsw[0][0], total)
    want[scales_at:hyper_at] = np.tile(rowsw[0][1], total)
    want[info_at:info_at + 16] = info.view(np.uint8)
    got = buf.cpu().numpy()
    assert f32_tree.same_f32(got.view(np.float32), want.view(np.float32)) and np.array_equal(got[rows_at:hyper_at], want[rows_at:hyper_at])
    for w, k in zip(wide, (G_, M_, V_)):
        e = np.full(total * sst, base.SENT32, dtype=np.uint32)
        for b in range(total):
            e[b * sst:b * sst + blk] = np.ascontiguousarray(values[0][k][b]).view(np.uint32)
        assert f32_tree.same_f32(w.cpu().numpy().view(np.float32), e.view(np.float32)), one.NAMES[k]
    plan.close()


# ------------------------------------------------------------------ 11. the rows through the scaled MFMA
def test_rows_feed_the_scaled_mfma():
    """8 ranks, one identity bucket of blk = 512 (a rank row is a 16 x 256 matrix, two k-steps): rank 0's and the last
    rank's rows go to v_mfma_scale_f32_16x16x128_f8f6f4 through tests/mx_consumer.hip's helper where the call
    wrote them, one element at a time through one-hot B; the output equals t.mxfp8_dequantize of the expectation."""
    import test_gpu_mx_consumer as mfma
    algo, side, total = t.SWING, 4, 8
    lst = ((2, "identity", 1),)
    bk = mxt.MxBucket(total, 512 * total, skew=True)
    data = mc.make(total, 22, lst)
    planes = Planes([bk], "flat", data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(2), nsq)
    plan = base.any_plan(algo, side, total)
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_mxfp8(planes.args(), (1,), small.hyper, 2, small.norm_sq, small.info, stream=stream())
    assert tr.kernels == [kernel(total, False, False)]
    want_all = mc.expect(data, (1,), nsq, total, False, False)
    check_all([bk], planes, small, want_all, "the rows the MFMA is about to read")
    we, ws = want_all[1][0]
    k = bk.blk // 2
    want = ref.dequantize64(we, ws).reshape(16, k)
    with np.errstate(over="ignore"):
        assert np.array_equal(t.mxfp8_dequantize(we, ws).reshape(16, k), want.astype(np.float32), equal_nan=True)
    nan_rows = np.isnan(want).any(axis=1)
    assert nan_rows.any() and not nan_rows.all()
    for r in (0, total - 1):
        got = mfma.every_element(bk.buf[0].data_ptr() + r * bk.row_stride, k, bk.buf[1].data_ptr() + r * bk.scale_stride, k // 32, 16, k)
        assert np.isnan(got[nan_rows]).all() and not np.isnan(got[~nan_rows]).any()
        mfma.report(f"rank {r}", mfma.same_value(got[~nan_rows], want[~nan_rows], f"rank {r}'s row"))
    plan.close()
