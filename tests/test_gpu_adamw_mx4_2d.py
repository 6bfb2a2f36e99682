"""allred_plan_adamw_all_gather_shards_mxfp4_2d (k_adamw_ag_mxfp4_2d), BIT FOR BIT on whole buffers (planes as uint32, NaNs by
class; bytes exactly) around sentinels: the planes against adamw_ref.step with eff(group), the four outputs against
mx4_2d_ref.expected of that p'.  A bucket is (cols, R, kind, group) as in test_gpu_adamw_mx2d; `identity` holds p =
mx4_2d_ref.hard_t (the planted MXFP4 blocks), g = m = v = 0 in group 1 (weight_decay = 0), so p' has p's bits and every planted
block reaches BOTH quantisers through the update path.  Buffers: test_gpu_shards_mxfp4_2d.Bucket2d, test_gpu_adamw_mx.Planes,
test_gpu_adamw_groups.SmallG."""
import ctypes as C
import functools

import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_ref
import f32_tree
import mx4_2d_ref as r2
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_adamw_groups as groups  # noqa: E402
import test_gpu_adamw_mx as amx  # noqa: E402
import test_gpu_adamw_mx2d as a2  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_shards_mxfp4_2d as m4  # noqa: E402

pytestmark = pytest.mark.gpu
stream, SmallG, Planes, tf, swap = base.stream, groups.SmallG, amx.Planes, a2.tf, a2.swap
P_, G_, M_, V_ = range(4)
G = _lib.ADAMW_MX4_2D_GROUP_MAX
SHAPES = {p: tuple((cols, R) for q, cols, R in r2.SHAPES if q == p) for p in (8, 16, 64)}   # mx4_2d_ref's, per rank count


def kernel(total, zero, rceil, rows=True):
    return f"k_adamw_ag_mxfp4_2d<{total}, {tf(zero)}, {tf(rceil)}, {tf(rows)}>"


@functools.lru_cache(maxsize=None)
def make_data(total, lst, seed):
    """data[i] = (p, g, m, v), each (total, R * cols) float32: test_gpu_adamw_mx2d.make_data with the MXFP4 planted blocks"""
    out = []
    for i, (cols, R, kind, _) in enumerate(lst):
        if kind == "identity":
            p = r2.hard_t(total, cols, R, seed + i).reshape(total, -1).copy()
            z = np.zeros_like(p)
            out.append((p, z, z.copy(), z.copy()))
        else:
            out.append(getattr(adamw_cases, kind)(seed + i, (total, R * cols)))
    return out


def quantised(p, total, entry, rceil):
    return r2.expected(np.ascontiguousarray(p).reshape(total * entry[1], entry[0]), total, rceil)


def expect(data, lst, total, nsq, zero, rceil, grps=gc.GROUPS):
    """per bucket the planes after the call and (rows, scales, t rows, t scales); the info words (group 0's)"""
    planes = [adamw_ref.step(*d, gc.eff(entry[3], grps), nsq, total, zero)[0] for d, entry in zip(data, lst)]
    outs = [quantised(pl[P_], total, entry, rceil) for pl, entry in zip(planes, lst)]
    u = adamw_ref.uniforms(grps[0], nsq, total)
    return planes, outs, np.array([u["N"], u["c"], 1.0 if u["skip"] else 0.0, 0.0], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def list_want(total, lst, seed, zero, rceil):
    return expect(make_data(total, lst, seed), lst, total, adamw_cases.norm_sq(total), zero, rceil)


def buckets_of(total, lst, rows=lambda i: True):
    return [m4.Bucket2d(total, cols, R, skew=i % 2 == 1, rows=rows(i)) for i, (cols, R, _, _) in enumerate(lst)]


def run(plan, planes, lst, small, zero=False, rceil=False, rows=True, **kw):
    args = planes.args() if rows else [(None, 0, None, 0) + a[4:] for a in planes.args()]
    plan.adamw_all_gather_shards_mxfp4_2d(args, [e[3] for e in lst], small.hyper, 3, small.norm_sq, small.info,
                                          zero_grad=zero, rceil=rceil, stream=kw.get("stream") or stream())


# ------------------------------------------------------------------ 1. against numpy
CASES = [(8, z, r, True) for z, r in amx.FLAGS] + [(16, True, False, True), (64, False, True, True), (8, True, True, False)]


@base.grids
@pytest.mark.parametrize("total,zero,rceil,rows", CASES, ids=[f"{p}-zero{int(z)}-rceil{int(r)}-rows{int(w)}" for p, z, r, w in CASES])
def test_step_and_both_orientations(total, zero, rceil, rows, grid):
    """every shape of mx4_2d_ref.SHAPES as an identity and as an update bucket, clipping active: p' m' v' (and g with zero_grad)
    bit for bit, every rank's four outputs = mxfp4(p') and mxfp4(p'^T), gaps, guards, skew and the small buffer's sentinels
    unchanged; one launch.  At pipe_grid 5 a workgroup takes many units: the peeled last square, the prefetch across units and
    both image rotations run.  rows = False: rows = scales = NULL in every bucket, and the row buffers keep their sentinels."""
    lst = a2.both_kinds(SHAPES[total])
    data = make_data(total, lst, 10 * total)
    want = list_want(total, lst, 10 * total, zero, rceil)
    assert want[2][1] < 1 and want[2][2] == 0   # clipping is active, the step is not skipped
    for d, entry, o in zip(data, lst, want[1]):   # on the reference alone: a kernel that quantised the old parameter fails
        if entry[2] != "identity":
            assert not np.array_equal(o[2], quantised(d[P_], total, entry, rceil)[2])
    buckets = buckets_of(total, lst)
    planes = Planes(buckets, "flat" if grid else "wide", data)
    small = SmallG(gc.hyper_array(), adamw_cases.norm_sq(total))
    plan = m4.plan_for(total)
    with t.tuned(pipe_grid=grid):
        assert plan.adamw_shards_mxfp4_2d_launches(planes.args()) == 1
        with t.launch_trace() as tr:
            run(plan, planes, lst, small, zero, rceil, rows)
    assert tr.kernels == [kernel(total, zero, rceil, rows)] and (not grid or tr.grids == [grid])
    if not rows:   # what the row buffers must hold is what they held
        held = [tuple(h[:b.total, :w] for h, w in zip(b.r.host, (b.n // 2, b.n // 32))) for b in buckets]
        want = (want[0], [h + o[2:] for h, o in zip(held, want[1])], want[2])
    a2.check_all(buckets, planes, small, want, f"zero_grad={zero}, rceil={rceil}, rows={rows}")
    plan.close()


# ------------------------------------------------------------------ 2. the guarantee and the skipped step, GPU against GPU
@pytest.mark.parametrize("skipped", [False, True], ids=["step", "skipped"])
@pytest.mark.parametrize("total,zero,rceil", [(8, False, True), (64, True, False)], ids=["swing-8", "swing-8x8"])
def test_planes_of_the_groups_call_outputs_of_the_2d_all_gather(total, zero, rceil, skipped):
    """allred.h's guarantee: the planes of adamw_all_gather_shards_f32_groups, the outputs of all_gather_shards_mxfp4_2d on the
    param plane it leaves.  skipped (an Inf in norm_sq): the planes keep their bits, the outputs are the quantisation of p,
    zero_grad still zeroes, info is what the groups call writes."""
    lst = a2.both_kinds(SHAPES[total][:3])
    data = make_data(total, lst, 200 + total)
    nsq = adamw_cases.norm_sq(total).copy()
    if skipped:
        nsq[total - 1] = np.inf
    buckets = buckets_of(total, lst)
    planes = Planes(buckets, "flat", data)
    small, small2 = SmallG(gc.hyper_array(), nsq), SmallG(gc.hyper_array(), nsq)
    plan = m4.plan_for(total)
    run(plan, planes, lst, small, zero, rceil)
    want = expect(data, lst, total, nsq, zero, rceil)
    a2.check_all(buckets, planes, small, want, "the numpy expectation")
    assert want[2][2] == (1 if skipped else 0)
    for d, v, entry, o in zip(data, want[0], lst, want[1]) if skipped else ():   # what the reference says of a skipped step
        assert all(np.array_equal(v[k].view(np.uint32), d[k].view(np.uint32)) for k in (P_, M_, V_))
        assert all(np.array_equal(a, b) for a, b in zip(o, quantised(d[P_], total, entry, rceil)))
    new = [g.copy() for s in planes.s for g in s.got()]
    new_out = [b.r.got() + b.c.got() for b in buckets]
    planes.restore()
    args = planes.args()
    rows16, second = one.rows_buckets(total, [e[0] * e[1] // 256 for e in lst]), buckets_of(total, lst)
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32_groups([r.arg + a[10:] for r, a in zip(rows16, args)], [e[3] for e in lst], small2.hyper, 3,
                                                small2.norm_sq, small2.info, zero_grad=zero, stream=stream())
        plan.all_gather_shards_mxfp4_2d([b.arg + (a[10], a[14]) for b, a in zip(second, args)], rceil=rceil, stream=stream())
    assert tr.kernels == [f"k_adamw_ag_groups_f32<{total}, {tf(zero)}>", m4.kernel(total, rceil)]
    old, old_out = [g for s in planes.s for g in s.got()], [b.r.got() + b.c.got() for b in second]
    for k, (a, b) in enumerate(zip(new, old)):
        assert f32_tree.same_f32(a.view(np.float32), b.view(np.float32)), f"plane buffer {k}"
    for i, (a, b) in enumerate(zip(new_out, old_out)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"bucket {i}: the four outputs"
    assert np.array_equal(groups.info_words(small), groups.info_words(small2))
    plan.close()


# ------------------------------------------------------------------ 3. launch boundaries
@pytest.mark.parametrize("count,launches", [(G, 1), (G + 1, 2), (2 * G + 1, 3)])
def test_16_buckets_per_launch_whatever_the_groups(count, launches):
    """mixed shapes, kinds and groups, every fourth bucket column-wise only: launch boundaries fall on every group in turn"""
    total = 8
    lst = tuple(SHAPES[8][i % 3] + (("identity", 1) if i % 3 == 1 else ("planes", i % 3)) for i in range(count))
    data = make_data(total, lst, 100)
    buckets = buckets_of(total, lst, rows=lambda i: i % 4 != 3)
    planes = Planes(buckets, "flat", data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    plan = m4.plan_for(total)
    assert plan.adamw_shards_mxfp4_2d_launches(planes.args()) == launches
    with t.launch_trace() as tr:
        run(plan, planes, lst, small, True, True)
    assert tr.count == launches and tr.kernels == [kernel(total, True, True)] * launches
    a2.check_all(buckets, planes, small, expect(data, lst, total, nsq, True, True), f"{count} buckets")
    plan.close()


# ------------------------------------------------------------------ 4. graph replay
def test_one_capture_replayed_as_three_steps():
    """between replays hyper, norm_sq and the gradient planes are rewritten by copies on the capture's stream: three numpy steps"""
    total = 16
    lst = tuple((cols, R, "planes", g) for (cols, R), g in zip(((64, 32), (96, 64), (32, 96), (128, 32)), (0, 1, 2, 1)))
    data = make_data(total, lst, 51)
    buckets = buckets_of(total, lst)
    planes = Planes(buckets, "flat", data)
    steps = [tuple(adamw_cases.hyper(step=k, lr=(1e-3, 3e-4, 2e-3)[g] / k, betas=((0.9, 0.999), (0.8, 0.99), (0.95, 0.95))[g],
                                     weight_decay=(0.01, 0.0, 0.1)[g]) for g in range(3)) for k in (1, 2, 3)]
    grads = [[adamw_cases.planes(60 + 10 * k + i, (b.total, b.blk))[G_] for i, b in enumerate(buckets)] for k in range(3)]
    nsqs = [adamw_cases.norm_sq(total, seed=k) for k in range(3)]
    small = SmallG(gc.hyper_array(3, steps[0]), nsqs[0])
    small_dev = [base.to_dev32(SmallG(gc.hyper_array(3, steps[k]), nsqs[k]).host) for k in range(3)]
    grad_dev = [[base.to_dev32(h) for h in planes.s[G_].expected(grads[k])] for k in range(3)]
    plan = m4.plan_for(total)
    # FOUR fresh streams, each of them used, the capture's the first: streams take the process's hardware queues (four by default)
    # in turn, and tests later in the same process pair a fresh stream with the default one and need the two on different
    # queues (test_gpu_peer's mutually waiting kernels).  With a whole turn taken here their streams land where they did before.
    s, *turn = [torch.cuda.Stream() for _ in range(4)]
    for x in turn:
        x.record_event()
    s.wait_stream(torch.cuda.current_stream())
    with t.tuned(pipe_grid=5):
        with torch.cuda.stream(s):   # an eager call first: the capture loads no code
            run(plan, planes, lst, small, rceil=True, stream=s)
        s.synchronize()
        planes.restore()
        small.restore()
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s), t.launch_trace() as tr:
            run(plan, planes, lst, small, rceil=True, stream=s)
    torch.cuda.synchronize()
    assert tr.kernels == [kernel(total, False, True)]
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
        want = expect(cur, lst, total, nsqs[k], False, True, steps[k])
        small.host = SmallG(gc.hyper_array(3, steps[k]), nsqs[k]).host
        a2.check_all(buckets, planes, small, want, f"replay {k + 1}")
        state = want[0]
    del g
    plan.close()


# ------------------------------------------------------------------ 5. refusals
REFUSALS = dict(a2.REFUSALS)   # the MXFP8 2D call's table without "scales NULL alone", and the halved payload's stride
del REFUSALS["scales NULL alone"]
REFUSALS["a t row stride of n / 2 - 16"] = (_lib.ERR_ARG, lambda a: dict(bucket=swap(a, 5, a[8] // 2 - 16)))


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_leave_every_buffer_untouched(what):
    total = 8
    lst = ((96, 64, "planes", 0), (32, 32, "planes", 2))
    data = make_data(total, lst, 71)
    buckets = buckets_of(total, lst)
    planes = Planes(buckets, "wide", data)
    small = SmallG(gc.hyper_array(), adamw_cases.norm_sq(total))
    args = planes.args()
    status, change = REFUSALS[what]
    kw = dict(group_of=(0, 2), ngroups=3, flags=0, bucket=args[1])
    kw.update(change(args[1]))
    arr, count = t.Plan._adamw_mx2d_buckets_f32([args[0], kw["bucket"]])
    plan = m4.plan_for(total)
    got = _lib.lib.allred_plan_adamw_all_gather_shards_mxfp4_2d(plan._h, arr, (C.c_uint8 * 2)(*kw["group_of"]), count, small.hyper,
                                                               kw["ngroups"], small.norm_sq, small.info, kw["flags"], None)
    assert got == status
    assert plan.adamw_shards_mxfp4_2d_launches(args) == 1   # the list itself is fine
    plan.close()
    planes.check(data, "written by a refused call")
    for b in buckets:
        b.check(None, "written by a refused call")
    small.check(None, "written by a refused call")
