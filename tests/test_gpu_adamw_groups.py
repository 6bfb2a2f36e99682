"""allred_plan_adamw_all_gather_shards_f32_groups (k_adamw_ag_groups_f32): AdamW parameter groups —
a hyperparameter set chosen per bucket — inside the grouped all-gather's launch.

Expectations: tests/adamw_ref.py (numpy float32, one IEEE operation per operation of allred.h) with
eff(group_of[i]) of tests/adamw_groups_cases.py — group g's set with max_norm replaced by group 0's —
on the data of tests/adamw_cases.py, compared BIT FOR BIT, fp32 as uint32, NaNs by class.  The three
groups differ in every field; tests/test_adamw_groups_cases.py pins that taking any one field from
another group, or the group's own max_norm, changes these bits.

Buffers are tests/test_gpu_adamw_shards.py's: every bucket's rows in a buffer of their own with the
skew and a guard row = sentinel, the four fp32 planes sentinel-filled with a guard behind each —
compact, wide and flat —, WHOLE buffers compared.  The hyper array, norm_sq and info live in one
small sentinel-filled buffer, compared whole too."""
import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_ref
import f32_norm
import f32_tree
import far_arena
import tenstorrentallreduce_amd as t
import test_gpu_adamw_shards as one
import test_gpu_shards_f32 as base
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENT32 = base.SENT32
stream = base.stream
Planes, rows_buckets, make_data, check_all = one.Planes, one.rows_buckets, one.make_data, one.check_all
P_, G_, M_, V_ = range(4)
GROUP_OF = (0, 1, 2, 1)   # of the four buckets of base.UNEQUAL


def kernel(total, zero):
    return f"k_adamw_ag_groups_f32<{total}, {'true' if zero else 'false'}>"


class SmallG:
    """the hyper array (up to 8 x 32 bytes), norm_sq (P floats) and info (16 bytes) in one sentinel-filled
    device buffer; check() as test_gpu_adamw_shards.Small's"""
    HYPER, NORM, INFO, WORDS = 16, 96, 176, 208

    def __init__(self, hyper, norm_sq=None):
        hyper = np.asarray(hyper, dtype=np.float32).reshape(-1, 8)
        self.ngroups = hyper.shape[0]
        self.host = np.full(self.WORDS, SENT32, dtype=np.uint32)
        self.host[self.HYPER:self.HYPER + 8 * self.ngroups] = hyper.reshape(-1).view(np.uint32)
        if norm_sq is not None:
            self.host[self.NORM:self.NORM + len(norm_sq)] = np.asarray(norm_sq, dtype=np.float32).view(np.uint32)
        self.buf = base.to_dev32(self.host)
        at = self.buf.data_ptr()
        self.hyper, self.norm_sq, self.info = at + 4 * self.HYPER, (at + 4 * self.NORM if norm_sq is not None else None), at + 4 * self.INFO

    restore = one.Small.restore
    check = one.Small.check


def info_words(small):
    torch.cuda.synchronize()
    return small.buf.cpu().numpy().view(np.uint32)[small.INFO:small.INFO + 4].copy()


def snapshot(buckets, planes):
    """every plane buffer (uint32) and every row buffer (uint16), whole"""
    return [g.copy() for s in planes.s for g in s.got()] + [b.got().copy() for b in buckets]


def same(a, b):
    """bit-equal, NaNs by class"""
    assert a.dtype == b.dtype and a.shape == b.shape
    return f32_tree.same_f32(a.view(np.float32), b.view(np.float32)) if a.dtype == np.uint32 else f32_tree.same_bf16(a, b)


# ------------------------------------------------------------------ 1. the step, every schedule, layout and grid
@base.grids
@base.layouts
@base.sched
def test_groups_step_and_all_gather(algo, side, total, layout, grid):
    """four unequal buckets in groups (0, 1, 2, 1): p' m' v' (and g with zero_grad) bit for bit with each
    bucket's own group's values, every rank row = bf16_rne(p'), gaps, guards, skew and the small buffer's
    sentinels unchanged; clipping by group 0's max_norm active; one launch of the new kernel."""
    buckets = rows_buckets(total, base.UNEQUAL)
    data = make_data(buckets, 10 * total)
    planes = Planes(buckets, layout, data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    plan = base.any_plan(algo, side, total)
    with t.tuned(pipe_grid=grid):
        assert plan.adamw_shards_f32_launches(planes.args()) == 1
        for zero in (False, True):
            planes.restore()
            small.restore()
            with t.launch_trace() as tr:
                plan.adamw_all_gather_shards_f32_groups(planes.args(), GROUP_OF, small.hyper, 3, small.norm_sq, small.info,
                                                        zero_grad=zero, stream=stream())
            assert tr.kernels == [kernel(total, zero)]
            want = gc.expect(data, GROUP_OF, nsq, total, zero)
            assert want[2][1] < 1 and want[2][2] == 0   # clipping is active, the step is not skipped
            check_all(buckets, planes, small, want, f"zero_grad={zero}")
    plan.close()


# ------------------------------------------------------------------ 2. one call = one call per group
@pytest.mark.parametrize("algo,side,total", [(t.SWING, 4, 8), (t.SWING, 8, 64)], ids=["swing-8", "swing-8x8"])
@pytest.mark.parametrize("zero", [False, True], ids=["keep-grad", "zero-grad"])
def test_one_call_equals_one_existing_call_per_group(algo, side, total, zero):
    """allred.h's guarantee: the list through the new call once, and — on restored buffers — through
    allred_plan_adamw_all_gather_shards_f32 once per group on that group's sublist with eff(g): every
    plane buffer, every row buffer and info bit-equal."""
    buckets = rows_buckets(total, base.UNEQUAL)
    planes = Planes(buckets, "flat", make_data(buckets, 200 + total))
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    singles = [one.Small(gc.eff(g), nsq) for g in range(3)]
    args = planes.args()
    plan = base.any_plan(algo, side, total)
    plan.adamw_all_gather_shards_f32_groups(args, GROUP_OF, small.hyper, 3, small.norm_sq, small.info, zero_grad=zero, stream=stream())
    new, new_info = snapshot(buckets, planes), info_words(small)
    planes.restore()
    with t.launch_trace() as tr:
        for g in range(3):
            sub = [a for a, go in zip(args, GROUP_OF) if go == g]
            plan.adamw_all_gather_shards_f32(sub, singles[g].hyper, singles[g].norm_sq, singles[g].info, zero_grad=zero, stream=stream())
    assert tr.count == 3
    old = snapshot(buckets, planes)
    assert len(new) == len(old)
    for k, (a, b) in enumerate(zip(new, old)):
        assert same(a, b), f"buffer {k}"
    for g in range(3):
        assert np.array_equal(info_words(singles[g]), new_info), f"info of group {g}'s call"
    assert not np.array_equal(new[0], planes.s[P_].host[0])   # something was computed
    plan.close()


# ------------------------------------------------------------------ 3. one group
@pytest.mark.parametrize("group_of", [None, (0, 0, 0, 0)], ids=["group_of-NULL", "group_of-zeros"])
def test_one_group_is_the_existing_call(group_of):
    """ngroups == 1: bit-equal to allred_plan_adamw_all_gather_shards_f32 and to the numpy expectation,
    through the NEW kernel (the call has one form)."""
    algo, side, total = t.RECDUB, 4, 16
    buckets = rows_buckets(total, base.UNEQUAL)
    data = make_data(buckets, 300)
    planes = Planes(buckets, "wide", data)
    hyper, nsq = adamw_cases.hyper(), adamw_cases.norm_sq(total)
    small, single = SmallG(hyper, nsq), one.Small(hyper, nsq)
    plan = base.any_plan(algo, side, total)
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32_groups(planes.args(), group_of, small.hyper, 1, small.norm_sq, small.info, zero_grad=True, stream=stream())
    assert tr.kernels == [kernel(total, True)]
    check_all(buckets, planes, small, one.expect(data, hyper, nsq, total, True), "one group")
    new = snapshot(buckets, planes)
    planes.restore()
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32(planes.args(), single.hyper, single.norm_sq, single.info, zero_grad=True, stream=stream())
    assert tr.kernels == [f"k_adamw_ag_group_f32<{total}, true>"]
    for k, (a, b) in enumerate(zip(new, snapshot(buckets, planes))):
        assert same(a, b), f"buffer {k}"
    assert np.array_equal(info_words(small), info_words(single))
    plan.close()


# ------------------------------------------------------------------ 4. launches
@pytest.mark.parametrize("count,launches", [(32, 1), (33, 2), (65, 3)])
def test_32_buckets_per_launch_whatever_the_groups(count, launches):
    """one-tile buckets, bucket i in group i % 3: launch boundaries at 32 and 64 fall on every group in
    turn, so a group table indexed by the bucket's place in the LIST fails from bucket 32 on."""
    algo, side, total = t.SWING, 4, 8
    buckets = rows_buckets(total, (1,) * count)
    data = make_data(buckets, 100)
    planes = Planes(buckets, "flat", data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    group_of = [i % 3 for i in range(count)]
    plan = base.any_plan(algo, side, total)
    assert plan.adamw_shards_f32_launches(planes.args()) == launches
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32_groups(planes.args(), group_of, small.hyper, 3, small.norm_sq, small.info, zero_grad=True, stream=stream())
    assert tr.count == launches and tr.kernels == [kernel(total, True)] * launches
    check_all(buckets, planes, small, gc.expect(data, group_of, nsq, total, True), f"{count} buckets")
    plan.close()


# ------------------------------------------------------------------ 5. the call-wide values
@pytest.mark.parametrize("case", list(one.uniform_cases(64)))
def test_call_wide_values_with_three_groups(case):
    """test_gpu_adamw_shards.uniform_cases with the case's set as group 0 and two more groups: norm_sq
    NULL (c == 1), no clipping, clipping, N = +0, and N = +Inf / NaN — the skipped step: EVERY group's
    state bit-equal to before, rows = bf16_rne(p), grad zeroed only with the flag, info[2] = 1."""
    algo, side, total = t.SWING, 8, 64
    hyper0, nsq = one.uniform_cases(total)[case]
    groups = (hyper0, gc.GROUPS[1], gc.GROUPS[2])
    group_of = (2, 0, 1)
    buckets = rows_buckets(total, (1, 2, 1))
    data = make_data(buckets, 7)
    planes = Planes(buckets, "wide", data)
    small = SmallG(gc.hyper_array(3, groups), nsq)
    plan = base.any_plan(algo, side, total)
    for zero in (False, True):
        planes.restore()
        small.restore()
        plan.adamw_all_gather_shards_f32_groups(planes.args(), group_of, small.hyper, 3, small.norm_sq, small.info, zero_grad=zero, stream=stream())
        want = gc.expect(data, group_of, nsq, total, zero, groups)
        info = want[2]
        if case in ("N-inf", "N-nan"):
            assert info[2] == 1
            for d, v, r in zip(data, want[0], want[1]):
                assert all(np.array_equal(v[k].view(np.uint32), d[k].view(np.uint32)) for k in (P_, M_, V_))
                assert np.array_equal(r, f32_tree.bf16_rne(d[P_]))
                assert (v[G_].view(np.uint32) == 0).all() if zero else np.array_equal(v[G_].view(np.uint32), d[G_].view(np.uint32))
        else:
            assert info[2] == 0 and (info[1] < 1) == (case == "clip") and (info[1] == 1) == (case != "clip")
        if case == "no-norm":
            assert info[0] == 0 and info[1] == 1
        check_all(buckets, planes, small, want, f"{case}, zero_grad={zero}")
    plan.close()


# ------------------------------------------------------------------ 6. one capture, three steps
def test_one_capture_replayed_as_three_steps():
    """the whole hyper array travels through device memory: between replays all three sets (another lr
    per group and step, the step's bias corrections) and the gradient planes are rewritten by
    stream-ordered copies on the capture's side stream; three replays = three numpy steps."""
    algo, side, total = t.SWING, 4, 16
    buckets = rows_buckets(total, base.UNEQUAL)
    data = make_data(buckets, 51)
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
        plan.adamw_all_gather_shards_f32_groups(args, GROUP_OF, small.hyper, 3, small.norm_sq, small.info, stream=s)
    s.synchronize()
    planes.restore()
    small.restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.adamw_all_gather_shards_f32_groups(args, GROUP_OF, small.hyper, 3, small.norm_sq, small.info, stream=s)
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
        want = gc.expect(cur, GROUP_OF, nsqs[k], total, False, steps[k])
        small.host = SmallG(gc.hyper_array(3, steps[k]), nsqs[k]).host
        check_all(buckets, planes, small, want, f"replay {k + 1}")
        state = want[0]
    del g
    plan.close()


# ------------------------------------------------------------------ 7. the two-launch step end to end
@pytest.mark.parametrize("algo,side,total", [(t.SWING, 8, 64), (t.RECDUB, 4, 16)], ids=["swing-8x8", "recdub-4x4"])
def test_reduce_scatter_with_norm_then_adamw_groups(algo, side, total):
    """reduce_scatter_shards_f32_norm into the gradient planes, then the new call with its norm_sq and
    TWO groups, on hard_inputs.cancel, against the composed numpy expectation."""
    import test_gpu_shards_f32_norm as norm_base
    grads = base.unequal(algo, side, total, seed=11)          # their rows: the gradients, kept
    params = rows_buckets(total, base.UNEQUAL)                # the parameter rows, written
    data = make_data(params, 41)
    planes = Planes(params, "flat", data)
    scale = 1.0 / total
    rs_args = [g.arg + (a[4], a[7]) for g, a in zip(grads, planes.args())]
    plan = base.any_plan(algo, side, total)
    norm = norm_base.Norm(plan, rs_args, total)
    groups = (adamw_cases.hyper(max_norm=0.25), gc.GROUPS[1])
    group_of = (1, 0, 0, 1)
    small = SmallG(gc.hyper_array(2, groups))
    with t.tuned(pipe_grid=5), t.launch_trace() as tr:
        plan.reduce_scatter_shards_f32_norm(rs_args, norm.sq_ptr, norm.ws_ptr, scale, stream=stream())
        plan.adamw_all_gather_shards_f32_groups(planes.args(), group_of, small.hyper, 2, norm.sq_ptr, small.info, zero_grad=True, stream=stream())
    assert tr.kernels == [f"k_tree_group_f32_norm<{total}, false>", kernel(total, True)]
    g = [f32_tree.scaled(b.sums, scale) for b in grads]
    nsq = f32_norm.expect_norm_sq(g)
    norm.check(nsq, "the reduce-scatter's norm")
    want = gc.expect([(d[P_], gi, d[M_], d[V_]) for d, gi in zip(data, g)], group_of, nsq, total, True, groups)
    assert want[2][1] < 1 and want[2][2] == 0
    check_all(params, planes, small, want, "the two-launch step")
    base.check_buckets(grads, [b.host for b in grads], "the gradient rows are only read")
    plan.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_every_buffer_untouched():
    algo, side, total = t.SWING, 4, 8
    buckets = rows_buckets(total, base.UNEQUAL)
    data = make_data(buckets, 71)
    planes = Planes(buckets, "wide", data)
    small = SmallG(gc.hyper_array(), adamw_cases.norm_sq(total))
    args = planes.args()
    s = stream()
    lib = _lib.lib
    import ctypes as C

    def status(plan, lst, group_of=GROUP_OF, hyper=small.hyper, ngroups=3, norm_sq=small.norm_sq, info=small.info, flags=0):
        arr, count = t.Plan._adamw_buckets_f32(lst)
        groups = None if group_of is None else (C.c_uint8 * max(len(group_of), 1))(*group_of)
        return lib.allred_plan_adamw_all_gather_shards_f32_groups(plan._h if plan else None, arr, groups, count, hyper or None, ngroups,
                                                                  norm_sq or None, info or None, flags, None)

    def refused(want, plan, lst, **kw):
        assert status(plan, lst, **kw) == want and status(plan, lst, flags=1, **kw) == want
        with pytest.raises(t.AllredError) as e:
            plan.adamw_all_gather_shards_f32_groups(lst, kw.get("group_of", GROUP_OF), kw.get("hyper", small.hyper), kw.get("ngroups", 3),
                                                    kw.get("norm_sq", small.norm_sq), kw.get("info", small.info), stream=s)
        assert e.value.status == want

    plan = base.any_plan(algo, side, total)
    hy, sq, info = small.hyper, small.norm_sq, small.info
    ptr, stride, n, pp, gp, mp, vp, ss = args[1]
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
    refused(_lib.ERR_ARG, plan, args, group_of=(0, 1, 255, 1))
    # --- the hyper array
    for d in (4, 8):                                                              # misaligned
        refused(_lib.ERR_ARG, plan, args, hyper=hy + d)
        assert status(plan, [], hyper=hy + d) == _lib.ERR_ARG
    refused(_lib.ERR_ARG, plan, args, hyper=0)
    assert status(plan, [], hyper=0) == _lib.ERR_ARG
    refused(_lib.ERR_ARG, plan, args, info=hy + 64 + 16)                          # info inside the LAST group's 32 bytes
    refused(_lib.ERR_ARG, plan, args, info=hy + 64)
    assert status(plan, [], info=hy + 64 + 16) == _lib.ERR_ARG
    refused(_lib.ERR_ARG, plan, args, norm_sq=hy + 92)                            # norm_sq on the last group's last float
    gap = pp + 4 * blk   # the 256-byte gap behind block 0 of bucket 1's param plane (wide layout)
    # a plane block on the SECOND group's bytes and on nothing else that is checked: two sets, no norm_sq, no
    # info, exp_avg_sq's block 0 from hyper + 32 on — a rule that still assumed 32 bytes would accept it
    refused(_lib.ERR_ARG, plan, rest + [(ptr, stride, n, pp, gp, mp, hy + 32, blk)], ngroups=2, group_of=(0, 1, 0, 1), norm_sq=0, info=0)
    refused(_lib.ERR_ARG, plan, args, hyper=gap - 64)                             # the first two sets on block 0's tail
    refused(_lib.ERR_ARG, plan, args, hyper=gap + 256 - 64)                       # the third set alone on block 1's head
    refused(_lib.ERR_ARG, plan, args, hyper=gap + 256 - 48)                       # the second set's last 16 bytes on block 1's head
    refused(_lib.ERR_ARG, plan, args, hyper=ptr + 2 * n - 48)                     # the second group on the last bytes of a row
    # --- every refusal of the existing call, once
    for other in (base.any_plan(algo, side, total, variant=t.LO), base.any_plan(algo, side, total, variant=t.MEM),
                  base.any_plan(algo, side, total, exec_mode=t.EXEC_STEPS)):
        refused(_lib.ERR_UNSUPPORTED, other, args)
        other.close()
    p4 = t.Plan(t.SWING, t.BO, 2, 256 * 4, 4, t.EXEC_FUSED)
    refused(_lib.ERR_UNSUPPORTED, p4, [(args[0][0], args[0][1], 256 * 4) + args[0][3:7] + (256,)], group_of=(1,))
    p4.close()
    part = (ptr, stride, 8 * total * 3, pp, gp, mp, vp, 24)
    refused(_lib.ERR_UNSUPPORTED, plan, rest + [part])
    refused(_lib.ERR_UNSUPPORTED, plan, [part] + rest)
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
        rest + [(ptr, n - 8, n, pp, gp, mp, vp, ss)],             # stride < n
        rest + [(ptr + 2, stride, n, pp, gp, mp, vp, ss)],        # rows not 16-byte aligned
        rest + [(0, stride, n, pp, gp, mp, vp, ss)],              # a null bucket
        rest + [(ptr, stride, 0, pp, gp, mp, vp, ss)],            # an empty bucket
    ]
    for bad in bad_lists:
        refused(_lib.ERR_ARG, plan, bad)
    refused(_lib.ERR_ARG, plan, args + [(ptr + 2 * stride, stride, n, pp, gp, mp, vp, ss)], group_of=GROUP_OF + (0,))   # inside bucket 1's rows
    pointer_cases = {   # refused whatever the list, an empty one included
        "norm_sq 2-byte aligned": dict(norm_sq=sq + 2), "info 8-byte aligned": dict(info=info + 8),
        "an unknown flag bit": dict(flags=2), "flags 3": dict(flags=3), "flags -2": dict(flags=-2),
        "info inside the first group": dict(info=hy + 16), "info on norm_sq": dict(info=sq + 16),
    }
    overlap_cases = {   # refused against this list
        "info on a row": dict(info=ptr + 2 * stride), "info on the last bytes of a row": dict(info=ptr + 2 * n - 16),
        "hyper inside a plane block": dict(hyper=gp + 64), "norm_sq on a plane's last float": dict(norm_sq=vp + 4 * blk - 4),
        "info on the first bytes of a plane block": dict(info=mp + 4 * ss),
    }
    for what, kw in pointer_cases.items():
        assert status(plan, args, **kw) == _lib.ERR_ARG and status(plan, [], **kw) == _lib.ERR_ARG, what
    for what, kw in overlap_cases.items():
        assert status(plan, args, **kw) == _lib.ERR_ARG, what
    assert status(None, args) == _lib.ERR_ARG
    arr, count = t.Plan._adamw_buckets_f32(args)
    call = lib.allred_plan_adamw_all_gather_shards_f32_groups
    assert call(plan._h, arr, None, -1, hy, 3, None, None, 0, None) == _lib.ERR_ARG
    assert call(plan._h, None, None, 2, hy, 3, None, None, 0, None) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        plan.adamw_all_gather_shards_f32_groups(args, (0, 1), hy, 3, sq, info, stream=s)   # two indices for four buckets
    # count == 0: OK after the pointer and ngroups checks, nothing launched, info not written
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32_groups([], None, hy, 3, sq, info, zero_grad=True, stream=s)
        plan.adamw_all_gather_shards_f32_groups([], [], hy, 8, sq, info, stream=s)
        assert status(plan, [], group_of=None, norm_sq=0, info=0) == _lib.OK
    assert tr.count == 0
    plan.close()
    planes.check(data, "written by a refused call")
    base.check_buckets(buckets, [b.host for b in buckets], "rows written by a refused call")
    small.check(None, "written by a refused call")


# ------------------------------------------------------------------ 9. the array in a gap
def test_hyper_array_norm_sq_and_info_in_the_gaps_of_a_wide_stride():
    """three sets (96 bytes), info behind them and norm_sq at the tail of ONE 256-byte gap: accepted, right,
    and the call leaves the rest of every gap alone"""
    algo, side, total = t.SWING, 4, 8
    buckets = rows_buckets(total, (2, 1, 1))
    data = make_data(buckets, 81)
    planes = Planes(buckets, "wide", data)
    nsq = adamw_cases.norm_sq(total)
    group_of = (1, 2, 0)
    args = planes.args()
    blk = buckets[0].blk
    mirror = planes.s[P_].host[0]   # block 0's gap of bucket 0's param plane
    at = blk
    mirror[at:at + 24] = gc.hyper_array().reshape(-1).view(np.uint32)
    mirror[at + 64 - total:at + 64] = nsq.view(np.uint32)
    planes.s[P_].restore()
    gap = args[0][3] + 4 * blk
    plan = base.any_plan(algo, side, total)
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32_groups(args, group_of, gap, 3, gap + 4 * (64 - total), gap + 96, zero_grad=True, stream=stream())
    assert tr.kernels == [kernel(total, True)]
    values, rows, info = gc.expect(data, group_of, nsq, total, True)
    mirror[at + 24:at + 28] = info.view(np.uint32)
    planes.check(values, "the three in a gap")
    base.check_buckets(buckets, [b.after_all_gather(r) for b, r in zip(buckets, rows)], "rows", by_class=True)
    plan.close()


# ------------------------------------------------------------------ 10. rows and planes beyond 2^32 elements
@pytest.fixture(scope="module")
def far():
    f = far_arena.F32Far(planes=4)   # an allocation failure is an error of the test, not a skip
    yield f
    f.close()


def test_far_rows_and_four_far_planes_with_two_groups(far):
    """test_gpu_adamw_shards.test_far_rows_and_four_far_planes_in_one_flat_buffer's layout (8x8 Swing, the
    rank rows of the larger bucket at the far bf16 stride, the four planes of both at eight column
    offsets of ONE flat fp32 buffer whose 63rd row is beyond 2^32 floats), the two buckets in groups 1
    and 0, with zero_grad: every plane and row bit for bit, every guard intact, the arena sentinel again."""
    algo, side, total = t.SWING, 8, 64
    shapes = [(total, 256 * k) for k in far_arena.F32_TILES]
    assert len(shapes) == 2
    group_of = (1, 0)
    data = [adamw_cases.planes(80 + i, shape) for i, shape in enumerate(shapes)]
    for i, (rows, d) in enumerate(zip(far.rows, data)):
        rows.upload(base.inputs("soft", total, rows.set.width, 5))   # all of it is overwritten
        for k in range(4):
            far.planes[i][k].upload(d[k])
    args = [far.bucket(i) + tuple(far.planes[i][k].ptr for k in range(4)) + (far.stride_f32,) for i in range(len(data))]
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(2), nsq)
    plan = base.any_plan(algo, side, total)
    try:
        with t.tuned(pipe_grid=5):
            with t.launch_trace() as tr:
                plan.adamw_all_gather_shards_f32_groups(args, group_of, small.hyper, 2, small.norm_sq, small.info, zero_grad=True, stream=stream())
            torch.cuda.synchronize()
        assert tr.kernels == [kernel(total, True)]
        values, rows16, info = gc.expect(data, group_of, nsq, total, True)
        assert info[1] < 1 and info[2] == 0   # clipping is active, the step is not skipped
        for i in range(len(data)):
            for k in range(4):
                assert f32_tree.same_f32(far.planes[i][k].read().view(np.float32), values[i][k]), f"bucket {i} {one.NAMES[k]}"
            n = far.rows[i].set.width
            want = np.broadcast_to(np.ascontiguousarray(rows16[i]).reshape(-1), (total, n))
            assert f32_tree.same_bf16(far.rows[i].read(), want), f"bucket {i}: rows = bf16_rne(p')"
        small.check(info, "far rows, far planes")
    finally:
        plan.close()
        far.wipe()
    far.assert_sentinel()
