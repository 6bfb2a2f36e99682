"""allred_plan_adamw_all_gather_shards_f32 / allred_plan_adamw_shards_f32_launches
(k_adamw_ag_group_f32): the clipped AdamW step on the fp32 planes inside the grouped all-gather's
launch.

Expectations come from tests/adamw_ref.py (numpy float32, one IEEE operation per operation of
allred.h, pinned against torch on the CPU in tests/test_adamw_ref.py) on the data of
tests/adamw_cases.py, and are compared BIT FOR BIT — fp32 as uint32, NaNs by class.  A fast-math
division, an fma, the epsilon on the wrong side or the norm added left to right fail here:
test_adamw_ref.py pins that these data tell them apart.

Buffers are test_gpu_shards_f32.py's: every bucket's rows in a buffer of their own with the skew
and a guard row = sentinel, every fp32 plane sentinel-filled with a guard behind it — compact,
wide (the gaps sentinel) and flat (FOUR rank-major flat buffers, one per plane) —, WHOLE buffers
compared.  hyper, norm_sq and info live in one small sentinel-filled buffer, compared whole too."""
import numpy as np
import pytest

import adamw_cases
import adamw_ref
import f32_norm
import f32_tree
import far_arena
import tenstorrentallreduce_amd as t
import test_gpu_shards_f32 as base
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENT32 = base.SENT32
stream = base.stream
P_, G_, M_, V_ = range(4)
NAMES = ("param", "grad", "exp_avg", "exp_avg_sq")


def rows_buckets(total, tiles_per_block, seed=5):
    """buckets whose rows hold soft data (all of it is overwritten); strides preferred_rank_stride(n) and n in turn"""
    return [base.Bucket(base.inputs("soft", total, 256 * total * k, seed), None, None if i % 2 == 0 else 256 * total * k)
            for i, k in enumerate(tiles_per_block)]


class Planes:
    """the four fp32 planes of a bucket list in one layout: four base.Shards"""

    def __init__(self, buckets, layout, data):
        self.buckets = buckets
        self.s = [base.Shards(buckets, layout) for _ in range(4)]
        self.data = data   # data[i] = (p, g, m, v), each (total, blk) float32
        for k in range(4):
            self.s[k].fill([d[k] for d in data])

    def args(self):
        out = []
        for i, b in enumerate(self.buckets):
            a = [self.s[k].arg(i) for k in range(4)]
            out.append(b.arg + tuple(x[3] for x in a) + (a[0][4],))
        return out

    def restore(self):
        for s in self.s:
            s.restore()
        for b in self.buckets:
            b.restore()

    def check(self, values, what):
        """values[i] = (p, g, m, v) expected in bucket i's blocks; everything else as the host mirror"""
        for k in range(4):
            self.s[k].check(self.s[k].expected([v[k] for v in values]), f"{NAMES[k]}: {what}")


class Small:
    """hyper (32 bytes), norm_sq (P floats) and info (16 bytes) in one sentinel-filled device buffer"""
    HYPER, NORM, INFO, WORDS = 16, 32, 112, 144

    def __init__(self, hyper, norm_sq=None):
        self.host = np.full(self.WORDS, SENT32, dtype=np.uint32)
        self.host[self.HYPER:self.HYPER + 8] = np.asarray(hyper, dtype=np.float32).view(np.uint32)
        if norm_sq is not None:
            self.host[self.NORM:self.NORM + len(norm_sq)] = np.asarray(norm_sq, dtype=np.float32).view(np.uint32)
        self.buf = base.to_dev32(self.host)
        at = self.buf.data_ptr()
        self.hyper, self.norm_sq, self.info = at + 4 * self.HYPER, (at + 4 * self.NORM if norm_sq is not None else None), at + 4 * self.INFO

    def restore(self):
        self.buf.copy_(base.to_dev32(self.host))

    def check(self, info, what):
        """info: the four float32 expected, or None for untouched"""
        torch.cuda.synchronize()
        want = self.host.copy()
        if info is not None:
            want[self.INFO:self.INFO + 4] = np.asarray(info, dtype=np.float32).view(np.uint32)
        got = self.buf.cpu().numpy().view(np.uint32)
        assert f32_tree.same_f32(got.view(np.float32), want.view(np.float32)), \
            f"hyper / norm_sq / info: {what}\n got {got[self.INFO:self.INFO + 4].view(np.float32)}\nwant {want[self.INFO:self.INFO + 4].view(np.float32)}"


def make_data(buckets, seed, maker=adamw_cases.planes):
    return [maker(seed + i, (b.total, b.blk)) for i, b in enumerate(buckets)]


def expect(data, hyper, norm_sq, total, zero):
    """per bucket the planes after the call, the rows' blocks, and the info words"""
    planes, rows, info = [], [], None
    for d in data:
        pl, r, info = adamw_ref.step(*d, hyper, norm_sq, total, zero)
        planes.append(pl)
        rows.append(r)
    return planes, rows, info


def check_all(buckets, planes, small, want, what):
    values, rows, info = want
    planes.check(values, what)
    base.check_buckets(buckets, [b.after_all_gather(r) for b, r in zip(buckets, rows)], f"rows = bf16_rne(p'): {what}", by_class=True)
    small.check(info, what)


# ------------------------------------------------------------------ 1. the step, every schedule, layout and grid
@base.grids
@base.layouts
@base.sched
def test_adamw_step_and_all_gather(algo, side, total, layout, grid):
    """p' m' v' (and g with zero_grad) bit for bit, every rank row = bf16_rne(p'), gaps, guards, skew and
    the small buffer's sentinels unchanged; clipping active, with and without zero_grad."""
    buckets = rows_buckets(total, base.UNEQUAL)
    data = make_data(buckets, 10 * total)
    planes = Planes(buckets, layout, data)
    hyper, nsq = adamw_cases.hyper(), adamw_cases.norm_sq(total)
    small = Small(hyper, nsq)
    plan = base.any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.adamw_shards_f32_launches(planes.args()) == 1
        for zero in (False, True):
            planes.restore()
            small.restore()
            with t.launch_trace() as tr:
                plan.adamw_all_gather_shards_f32(planes.args(), small.hyper, small.norm_sq, small.info, zero_grad=zero, stream=stream())
            assert tr.kernels == [f"k_adamw_ag_group_f32<{total}, {'true' if zero else 'false'}>"]
            want = expect(data, hyper, nsq, total, zero)
            assert want[2][1] < 1 and want[2][2] == 0   # clipping is active, the step is not skipped
            check_all(buckets, planes, small, want, f"zero_grad={zero}")
    plan.close()


# ------------------------------------------------------------------ 2. the uniform values
def uniform_cases(total):
    nsq = adamw_cases.norm_sq(total)
    inf, nan = nsq.copy(), nsq.copy()
    inf[total - 1] = np.inf
    nan[1] = np.nan
    return {
        "no-norm": (adamw_cases.hyper(), None),
        "max-norm-inf": (adamw_cases.hyper(max_norm=float("inf")), nsq),
        "clip": (adamw_cases.hyper(step=1, max_norm=0.5), nsq),
        "no-clip": (adamw_cases.hyper(max_norm=1e4), nsq),
        "N-zero": (adamw_cases.hyper(), np.zeros(total, dtype=np.float32)),
        "N-inf": (adamw_cases.hyper(), inf),
        "N-nan": (adamw_cases.hyper(), nan),
    }


@pytest.mark.parametrize("case", list(uniform_cases(64)))
def test_uniform_values(case):
    """8x8 Swing: norm_sq NULL, no clipping, clipping, N = +0, and N = +Inf / NaN — the skipped step: the
    state bit-equal to before, rows = bf16_rne(p), grad zeroed only with the flag, info[2] = 1."""
    algo, side, total = t.SWING, 8, 64
    hyper, nsq = uniform_cases(total)[case]
    buckets = rows_buckets(total, (1, 2))
    data = make_data(buckets, 7)
    planes = Planes(buckets, "wide", data)
    small = Small(hyper, nsq)
    plan = base.any_plan(algo, side, total)
    for zero in (False, True):
        planes.restore()
        small.restore()
        plan.adamw_all_gather_shards_f32(planes.args(), small.hyper, small.norm_sq, small.info, zero_grad=zero, stream=stream())
        want = expect(data, hyper, nsq, total, zero)
        info = want[2]
        if case in ("N-inf", "N-nan"):
            assert info[2] == 1
            for d, v, r in zip(data, want[0], want[1]):
                assert all(np.array_equal(v[k].view(np.uint32), d[k].view(np.uint32)) for k in (P_, M_, V_))
                assert np.array_equal(r, f32_tree.bf16_rne(d[P_]))
                assert (v[G_].view(np.uint32) == 0).all() if zero else np.array_equal(v[G_].view(np.uint32), d[G_].view(np.uint32))
        else:
            assert info[2] == 0 and (info[1] < 1) == (case == "clip") and (info[1] == 1) == (case != "clip")
        check_all(buckets, planes, small, want, f"{case}, zero_grad={zero}")
    plan.close()


@pytest.mark.parametrize("maker,hyper", [(adamw_cases.negative_v, adamw_cases.hyper(step=1)),
                                         (adamw_cases.zero_den, adamw_cases.hyper(step=7, eps=0.0))], ids=["negative-v", "eps0"])
def test_nan_and_zero_denominators(maker, hyper):
    """v < 0: sqrtf gives NaN, compared by class; eps = 0 with v' = 0: m' / 0 = +-Inf, 0 / 0 = NaN"""
    algo, side, total = t.SWING, 4, 16
    buckets = rows_buckets(total, (2, 1))
    data = make_data(buckets, 21, maker)
    planes = Planes(buckets, "compact", data)
    nsq = adamw_cases.norm_sq(total)
    small = Small(hyper, nsq)
    plan = base.any_plan(algo, side, total)
    plan.adamw_all_gather_shards_f32(planes.args(), small.hyper, small.norm_sq, small.info, stream=stream())
    want = expect(data, hyper, nsq, total, False)
    assert any(f32_tree.is_nan32(v[P_]).any() for v in want[0])
    check_all(buckets, planes, small, want, "non-finite results")
    plan.close()


# ------------------------------------------------------------------ 3. the rows are the all-gather of the new parameters
@pytest.mark.parametrize("grid", [0, 5], ids=["default-grid", "grid5"])
def test_rows_equal_the_all_gather_of_the_new_parameters(grid):
    algo, side, total = t.RECDUB, 4, 16
    buckets, second = rows_buckets(total, base.UNEQUAL), rows_buckets(total, base.UNEQUAL, seed=6)
    planes = Planes(buckets, "flat", make_data(buckets, 31))
    small = Small(adamw_cases.hyper(), adamw_cases.norm_sq(total))
    plan = base.any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        plan.adamw_all_gather_shards_f32(planes.args(), small.hyper, small.norm_sq, None, stream=stream())
        args2 = [b.arg + (a[3], a[7]) for b, a in zip(second, planes.args())]   # the new param plane into other rows
        plan.all_gather_shards_f32(args2, stream())
    for i, (a, b) in enumerate(zip(buckets, second)):
        ga, gb = a.got(), b.got()
        assert f32_tree.same_bf16(ga[:total, :a.n], gb[:total, :b.n]), f"bucket {i}"
        assert not np.array_equal(ga[:total, :a.n], a.host[:total, :a.n])
    plan.close()


# ------------------------------------------------------------------ 4. the two-launch step end to end
@pytest.mark.parametrize("algo,side,total", [(t.SWING, 8, 64), (t.RECDUB, 4, 16)], ids=["swing-8x8", "recdub-4x4"])
def test_reduce_scatter_with_norm_then_adamw(algo, side, total):
    """reduce_scatter_shards_f32_norm into the gradient planes, then the new call with its norm_sq, on
    hard_inputs.cancel, against the composed numpy expectation."""
    import test_gpu_shards_f32_norm as norm_base
    grads = base.unequal(algo, side, total, seed=11)          # their rows: the gradients, kept
    params = rows_buckets(total, base.UNEQUAL)                # the parameter rows, written
    data = make_data(params, 41)
    planes = Planes(params, "flat", data)
    scale = 1.0 / total
    rs_args = [g.arg + (a[4], a[7]) for g, a in zip(grads, planes.args())]
    plan = base.any_plan(algo, side, total)
    norm = norm_base.Norm(plan, rs_args, total)
    hyper = adamw_cases.hyper(max_norm=0.25)
    small = Small(hyper)
    with t.tuned(pipe_grid=5), t.launch_trace() as tr:
        plan.reduce_scatter_shards_f32_norm(rs_args, norm.sq_ptr, norm.ws_ptr, scale, stream=stream())
        plan.adamw_all_gather_shards_f32(planes.args(), small.hyper, norm.sq_ptr, small.info, zero_grad=True, stream=stream())
    assert tr.kernels == [f"k_tree_group_f32_norm<{total}, false>", f"k_adamw_ag_group_f32<{total}, true>"]
    g = [f32_tree.scaled(b.sums, scale) for b in grads]
    nsq = f32_norm.expect_norm_sq(g)
    norm.check(nsq, "the reduce-scatter's norm")
    want = expect([(d[P_], gi, d[M_], d[V_]) for d, gi in zip(data, g)], hyper, nsq, total, True)
    assert want[2][1] < 1 and want[2][2] == 0
    check_all(params, planes, small, want, "the two-launch step")
    base.check_buckets(grads, [b.host for b in grads], "the gradient rows are only read")
    plan.close()


# ------------------------------------------------------------------ 5. launches
@pytest.mark.parametrize("count,launches", [(32, 1), (33, 2), (65, 3)])
def test_32_buckets_per_launch(count, launches):
    algo, side, total = t.SWING, 4, 8
    assert _lib.ADAMW_GROUP_MAX == 32
    buckets = rows_buckets(total, (1,) * count)
    data = make_data(buckets, 100)
    planes = Planes(buckets, "flat", data)
    hyper, nsq = adamw_cases.hyper(), adamw_cases.norm_sq(total)
    small = Small(hyper, nsq)
    plan = base.any_plan(algo, side, total)
    assert plan.adamw_shards_f32_launches(planes.args()) == launches
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32(planes.args(), small.hyper, small.norm_sq, small.info, zero_grad=True, stream=stream())
    assert tr.count == launches and tr.kernels == [f"k_adamw_ag_group_f32<{total}, true>"] * launches
    check_all(buckets, planes, small, expect(data, hyper, nsq, total, True), f"{count} buckets")
    plan.close()


# ------------------------------------------------------------------ 6. one capture, three steps
def test_one_capture_replayed_as_three_steps():
    """hyper travels through device memory: the capture holds no step number.  hyper and the gradient
    planes are rewritten by stream-ordered copies between replays; three replays = three numpy steps."""
    algo, side, total = t.SWING, 4, 16
    buckets = rows_buckets(total, base.UNEQUAL)
    data = make_data(buckets, 51)
    planes = Planes(buckets, "flat", data)
    steps = [adamw_cases.hyper(step=k, lr=1e-3 / k) for k in (1, 2, 3)]
    grads = [[adamw_cases.planes(60 + 10 * k + i, (b.total, b.blk))[G_] for i, b in enumerate(buckets)] for k in range(3)]
    nsqs = [adamw_cases.norm_sq(total, seed=k) for k in range(3)]
    small = Small(steps[0], nsqs[0])
    # what the copies read: device images of the small buffer and of the gradient plane's buffers, per step
    small_dev, grad_dev = [], []
    for k in range(3):
        img = Small(steps[k], nsqs[k]).host
        small_dev.append(base.to_dev32(img))
        mirror = planes.s[G_].expected(grads[k])
        grad_dev.append([base.to_dev32(h) for h in mirror])
    plan = base.any_plan(algo, side, total)
    args = planes.args()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # an eager call first: the capture loads no code
        plan.adamw_all_gather_shards_f32(args, small.hyper, small.norm_sq, small.info, stream=s)
    s.synchronize()
    planes.restore()
    small.restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.adamw_all_gather_shards_f32(args, small.hyper, small.norm_sq, small.info, stream=s)
    torch.cuda.synchronize()
    planes.check(data, "a capture runs nothing")
    state = data
    for k in range(3):
        with torch.cuda.stream(s):
            small.buf.copy_(small_dev[k], non_blocking=True)
            for d, src in zip(planes.s[G_].buf, grad_dev[k]):
                d.copy_(src, non_blocking=True)
            g.replay()
        s.synchronize()
        cur = [(st[P_], gi, st[M_], st[V_]) for st, gi in zip(state, grads[k])]
        values, rows, info = expect(cur, steps[k], nsqs[k], total, False)
        small.host = Small(steps[k], nsqs[k]).host
        check_all(buckets, planes, small, (values, rows, info), f"replay {k + 1}")
        state = values
    del g
    plan.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_every_buffer_untouched():
    algo, side, total = t.SWING, 4, 8
    buckets = rows_buckets(total, base.UNEQUAL)
    data = make_data(buckets, 71)
    planes = Planes(buckets, "wide", data)
    small = Small(adamw_cases.hyper(), adamw_cases.norm_sq(total))
    args = planes.args()
    s = stream()
    lib = _lib.lib

    def status(plan, lst, hyper=small.hyper, norm_sq=small.norm_sq, info=small.info, flags=0):
        arr, count = t.Plan._adamw_buckets_f32(lst)
        return lib.allred_plan_adamw_all_gather_shards_f32(plan._h if plan else None, arr, count, hyper or None, norm_sq or None,
                                                           info or None, flags, None)

    def refused_list(want, plan, lst):
        assert status(plan, lst) == want and status(plan, lst, flags=1) == want
        assert lib.allred_plan_adamw_shards_f32_launches(plan._h, *t.Plan._adamw_buckets_f32(lst)) == want
        with pytest.raises(t.AllredError) as e:
            plan.adamw_all_gather_shards_f32(lst, small.hyper, small.norm_sq, small.info, stream=s)
        assert e.value.status == want
        with pytest.raises(t.AllredError):
            plan.adamw_shards_f32_launches(lst)

    for other in (base.any_plan(algo, side, total, variant=t.LO), base.any_plan(algo, side, total, variant=t.MEM),
                  base.any_plan(algo, side, total, exec_mode=t.EXEC_STEPS)):
        refused_list(_lib.ERR_UNSUPPORTED, other, args)
        other.close()
    p4 = t.Plan(t.SWING, t.BO, 2, 256 * 4, 4, t.EXEC_FUSED)
    refused_list(_lib.ERR_UNSUPPORTED, p4, [(args[0][0], args[0][1], 256 * 4) + args[0][3:7] + (256,)])
    p4.close()
    plan = base.any_plan(algo, side, total)
    ptr, stride, n, pp, gp, mp, vp, ss = args[1]
    blk = n // total
    rest = args[:1] + args[2:]
    part = (ptr, stride, 8 * total * 3, pp, gp, mp, vp, 24)
    refused_list(_lib.ERR_UNSUPPORTED, plan, rest + [part])
    refused_list(_lib.ERR_UNSUPPORTED, plan, [part] + rest)
    o = args[2]
    bad_lists = [
        rest + [(ptr, stride, n, 0, gp, mp, vp, ss)], rest + [(ptr, stride, n, pp, 0, mp, vp, ss)],     # a NULL plane
        rest + [(ptr, stride, n, pp, gp, 0, vp, ss)], rest + [(ptr, stride, n, pp, gp, mp, 0, ss)],
        rest + [(ptr, stride, n, pp + 4, gp, mp, vp, ss)], rest + [(ptr, stride, n, pp, gp + 8, mp, vp, ss)],   # not 16-byte aligned
        rest + [(ptr, stride, n, pp, gp, mp + 4, vp, ss)], rest + [(ptr, stride, n, pp, gp, mp, vp + 8, ss)],
        rest + [(ptr, stride, n, pp, gp, mp, vp, blk - 4)],       # shard_stride < blk
        rest + [(ptr, stride, n, pp, gp, mp, vp, blk + 2)],       # shard_stride % 4 != 0
        rest + [(ptr, stride, n, pp, gp, mp, vp, 1 << 62)],       # address arithmetic that would overflow
        rest + [(ptr, stride, n, pp, gp, mp, vp, 1 << 63)],
        rest + [(ptr, stride, n, pp, pp, mp, vp, ss)],            # param == grad
        rest + [(ptr, stride, n, pp, gp, mp, mp, ss)],            # the same plane named twice
        rest + [(ptr, stride, n, pp, gp, mp, o[5], ss)],          # another bucket's exp_avg
        rest + [(ptr, stride, n, pp, gp, mp, o[3] + 4 * (o[2] // total) - 16, blk)],   # on the last 16 bytes of a block of bucket 2's param
        rest + [(ptr, stride, n, pp, gp, mp, o[0] + 2 * o[1], blk)],                   # a plane block inside bucket 2's rows
        args + [(ptr + 2 * stride, stride, n, pp, gp, mp, vp, ss)],                    # inside bucket 1's rows
        rest + [(ptr, n - 8, n, pp, gp, mp, vp, ss)],             # stride < n
        rest + [(ptr + 2, stride, n, pp, gp, mp, vp, ss)],        # rows not 16-byte aligned
        rest + [(0, stride, n, pp, gp, mp, vp, ss)],              # a null bucket
        rest + [(ptr, stride, 0, pp, gp, mp, vp, ss)],            # an empty bucket
    ]
    for bad in bad_lists:
        refused_list(_lib.ERR_ARG, plan, bad)
    hy, sq, info = small.hyper, small.norm_sq, small.info
    gap = pp + 4 * blk   # the 256-byte gap behind block 0 of bucket 1's param plane (wide layout)
    pointer_cases = {   # refused whatever the list, an empty one included
        "hyper NULL": dict(hyper=0), "hyper 8-byte aligned": dict(hyper=hy + 8), "hyper 4-byte aligned": dict(hyper=hy + 4),
        "norm_sq 2-byte aligned": dict(norm_sq=sq + 2), "info 8-byte aligned": dict(info=info + 8),
        "an unknown flag bit": dict(flags=2), "flags 3": dict(flags=3), "flags -2": dict(flags=-2),
        "info inside hyper": dict(info=hy + 16), "norm_sq on hyper's last float": dict(norm_sq=hy + 28),
        "info on norm_sq": dict(info=sq + 16),
    }
    overlap_cases = {   # refused against this list
        "info on a row": dict(info=ptr + 2 * stride), "info on the last bytes of a row": dict(info=ptr + 2 * n - 16),
        "hyper inside a plane block": dict(hyper=gp + 64), "hyper on the last bytes of a plane block": dict(hyper=gap - 16),
        "hyper over the end of a gap": dict(hyper=gap + 256 - 16), "norm_sq on a plane's last float": dict(norm_sq=vp + 4 * blk - 4),
        "info on the first bytes of a plane block": dict(info=mp + 4 * ss),
    }
    if stride > n:
        overlap_cases["info in a row's skew"] = dict(info=ptr + 2 * n)
    for what, kw in pointer_cases.items():
        assert status(plan, args, **kw) == _lib.ERR_ARG and status(plan, [], **kw) == _lib.ERR_ARG, what
    for what, kw in overlap_cases.items():
        assert status(plan, args, **kw) == _lib.ERR_ARG, what
    assert status(None, args) == _lib.ERR_ARG
    arr, count = t.Plan._adamw_buckets_f32(args)
    assert lib.allred_plan_adamw_all_gather_shards_f32(plan._h, arr, -1, hy, None, None, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_adamw_all_gather_shards_f32(plan._h, None, 2, hy, None, None, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_adamw_shards_f32_launches(plan._h, arr, -1) == _lib.ERR_ARG
    # count == 0: OK after the pointer checks, nothing launched, info not written
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32([], hy, sq, info, zero_grad=True, stream=s)
        assert status(plan, [], norm_sq=0, info=0) == _lib.OK
    assert tr.count == 0 and plan.adamw_shards_f32_launches([]) == 0
    assert status(plan, [], hyper=0) == _lib.ERR_ARG
    # hyper, norm_sq and info in the gaps of the wide stride: accepted (the dry run: nothing is written)
    assert lib.allred_plan_adamw_shards_f32_launches(plan._h, arr, count) == 1
    plan.close()
    planes.check(data, "written by a refused call")
    base.check_buckets(buckets, [b.host for b in buckets], "rows written by a refused call")
    small.check(None, "written by a refused call")


def test_hyper_norm_sq_and_info_in_the_gaps_of_a_wide_stride():
    """accepted, and the call leaves the rest of every gap alone"""
    algo, side, total = t.SWING, 4, 8
    buckets = rows_buckets(total, (2, 1))
    data = make_data(buckets, 81)
    planes = Planes(buckets, "wide", data)
    hyper, nsq = adamw_cases.hyper(), adamw_cases.norm_sq(total)
    args = planes.args()
    blk = buckets[0].blk
    # block 0's gap of bucket 0's param plane: hyper at its head, info behind it, norm_sq at the tail
    mirror = planes.s[P_].host[0]
    at = blk
    mirror[at:at + 8] = hyper.view(np.uint32)
    mirror[at + 64 - total:at + 64] = nsq.view(np.uint32)
    planes.s[P_].restore()
    gap = args[0][3] + 4 * blk
    plan = base.any_plan(algo, side, total)
    plan.adamw_all_gather_shards_f32(args, gap, gap + 4 * (64 - total), gap + 32, stream=stream())
    values, rows, info = expect(data, hyper, nsq, total, False)
    mirror[at + 8:at + 12] = info.view(np.uint32)
    planes.check(values, "the three in a gap")
    base.check_buckets(buckets, [b.after_all_gather(r) for b, r in zip(buckets, rows)], "rows", by_class=True)
    plan.close()


# ------------------------------------------------------------------ rows and planes beyond 2^32 elements
@pytest.fixture(scope="module")
def far():
    f = far_arena.F32Far(planes=4)   # an allocation failure is an error of the test, not a skip
    yield f
    f.close()


def test_far_rows_and_four_far_planes_in_one_flat_buffer(far):
    """8x8 Swing, buckets of 1 and 3 tiles per block, the rank rows of the larger at the far bf16 stride and the four
    planes of both buckets at eight column offsets of ONE flat fp32 buffer of row stride
    F = roundup4(ceil(2^32 / 63)) + 64 floats (tests/far_arena.py): 63 F is beyond 2^32 floats.  The
    clipped step with zero_grad: p' g m' v' and every row bit for bit tests/adamw_ref.py's, every guard
    intact, the whole arena sentinel again."""
    algo, side, total = t.SWING, 8, 64
    shapes = [(total, 256 * k) for k in far_arena.F32_TILES]
    data = [adamw_cases.planes(80 + i, shape) for i, shape in enumerate(shapes)]
    for i, (rows, d) in enumerate(zip(far.rows, data)):
        rows.upload(base.inputs("soft", total, rows.set.width, 5))   # all of it is overwritten
        for k in range(4):
            far.planes[i][k].upload(d[k])
    args = [far.bucket(i) + tuple(far.planes[i][k].ptr for k in range(4)) + (far.stride_f32,) for i in range(len(data))]
    hyper, nsq = adamw_cases.hyper(), adamw_cases.norm_sq(total)
    small = Small(hyper, nsq)
    plan = base.any_plan(algo, side, total)
    try:
        with t.tuned(pipe_grid=5):
            assert plan.adamw_shards_f32_launches(args) == 1
            with t.launch_trace() as tr:
                plan.adamw_all_gather_shards_f32(args, small.hyper, small.norm_sq, small.info, zero_grad=True, stream=stream())
            torch.cuda.synchronize()
        assert tr.kernels == [f"k_adamw_ag_group_f32<{total}, true>"]
        values, rows16, info = expect(data, hyper, nsq, total, True)
        assert info[1] < 1 and info[2] == 0   # clipping is active, the step is not skipped
        for i in range(len(data)):
            for k in range(4):
                assert f32_tree.same_f32(far.planes[i][k].read().view(np.float32), values[i][k]), f"bucket {i} {NAMES[k]}"
            n = far.rows[i].set.width
            want = np.broadcast_to(np.ascontiguousarray(rows16[i]).reshape(-1), (total, n))
            assert f32_tree.same_bf16(far.rows[i].read(), want), f"bucket {i}: rows = bf16_rne(p')"
        small.check(info, "far rows, far planes")
    finally:
        plan.close()
        far.wipe()
    far.assert_sentinel()
