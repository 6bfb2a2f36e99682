"""allred_plan_adamw_all_gather_shards_mxfp8_2d (k_adamw_ag_mxfp8_2d), BIT FOR BIT on whole buffers (planes as uint32, NaNs by
class; bytes exactly): the planes against adamw_ref.step with eff(group), the four outputs against mx2d_ref of that p'.
A bucket is (cols, R, kind, group): `identity` holds p = mx2d_ref.hard_t, g = m = v = 0 in group 1 (weight_decay = 0),
so p' has p's bits and every planted block reaches BOTH quantisers through the update path; the other kinds are
tests/adamw_cases.py's.  Buffers: test_gpu_shards_mxfp8_2d.Bucket2d, test_gpu_adamw_mx.Planes, test_gpu_adamw_groups.SmallG."""
import ctypes as C
import functools

import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_ref
import f32_tree
import mx2d_ref
import mxfp8_ref as ref
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_adamw_groups as groups  # noqa: E402
import test_gpu_adamw_mx as amx  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_shards_mxfp8 as mxt  # noqa: E402
import test_gpu_shards_mxfp8_2d as m2  # noqa: E402

pytestmark = pytest.mark.gpu
stream, SmallG, Planes, tf = base.stream, groups.SmallG, amx.Planes, m2.tf
P_, G_, M_, V_ = range(4)
G = _lib.ADAMW_MX2D_GROUP_MAX
# (cols, R): the four patch classes, one and three row groups, one, two and three column groups
SHAPES = ((32, 32), (96, 64), (64, 64), (128, 32), (96, 96))
SHAPES_64 = ((32, 32), (64, 128))
SCHEDULES = {8: (t.SWING, 4), 16: (t.SWING, 4), 64: (t.SWING, 8)}


def kernel(total, zero, rceil, rows=True):
    return f"k_adamw_ag_mxfp8_2d<{total}, {tf(zero)}, {tf(rceil)}, {tf(rows)}>"


def both_kinds(shapes):
    """every shape as an identity bucket (group 1) and as an update bucket (groups 0 and 2 in turn)"""
    return tuple(b for i, (cols, R) in enumerate(shapes) for b in ((cols, R, "identity", 1), (cols, R, "planes", 2 * (i % 2))))


@functools.lru_cache(maxsize=None)
def make_data(total, lst, seed, maker=None):
    """data[i] = (p, g, m, v), each (total, R * cols) float32"""
    out = []
    for i, (cols, R, kind, _) in enumerate(lst):
        if kind == "identity":
            p = mx2d_ref.blocks(mx2d_ref.hard_t(total, cols, R, seed + i), total).copy()
            z = np.zeros_like(p)
            out.append((p, z, z.copy(), z.copy()))
        else:
            out.append((maker or getattr(adamw_cases, kind))(seed + i, (total, R * cols)))
    return out


def quantised(p, total, lst_entry, rceil):
    W = np.ascontiguousarray(p).reshape(total * lst_entry[1], lst_entry[0])
    return mx2d_ref.expected_rows(W, total, rceil) + mx2d_ref.expected_t(W, rceil)


def expect(data, lst, total, nsq, zero, rceil, grps=gc.GROUPS):
    """per bucket the planes after the call and (rows, scales, t rows, t scales); the info words (group 0's)"""
    planes, outs = [], []
    for d, entry in zip(data, lst):
        pl, _, _ = adamw_ref.step(*d, gc.eff(entry[3], grps), nsq, total, zero)
        planes.append(pl)
        outs.append(quantised(pl[P_], total, entry, rceil))
    u = adamw_ref.uniforms(grps[0], nsq, total)
    return planes, outs, np.array([u["N"], u["c"], 1.0 if u["skip"] else 0.0, 0.0], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def list_want(total, lst, seed, zero, rceil):
    """the expectation of the list with adamw_cases.norm_sq, computed once per flag pair"""
    return expect(make_data(total, lst, seed), lst, total, adamw_cases.norm_sq(total), zero, rceil)


def buckets_of(total, lst, rows=True):
    return [m2.Bucket2d(total, cols, R, skew=i % 2 == 1, rows=rows) for i, (cols, R, _, _) in enumerate(lst)]


def check_all(buckets, planes, small, want, what):
    values, outs, info = want
    planes.check(values, what)
    for i, (b, o) in enumerate(zip(buckets, outs)):
        b.check(o, f"bucket {i} (cols={b.cols}, R={b.R}): {what}")
    small.check(info, what)


def run(plan, planes, lst, small, zero=False, rceil=False, rows=True):
    args = planes.args() if rows else [(None, 0, None, 0) + a[4:] for a in planes.args()]
    plan.adamw_all_gather_shards_mxfp8_2d(args, [e[3] for e in lst], small.hyper, 3, small.norm_sq, small.info,
                                          zero_grad=zero, rceil=rceil, stream=stream())


# ------------------------------------------------------------------ 1. against numpy, and 3. column-wise only
CASES = [(8, z, r, True) for z, r in amx.FLAGS] + [(16, False, True, True), (16, True, False, True), (64, True, True, True),
                                                   (64, False, False, True), (8, True, False, False)]


@base.grids
@pytest.mark.parametrize("total,zero,rceil,rows", CASES, ids=[f"{p}-zero{int(z)}-rceil{int(r)}-rows{int(w)}" for p, z, r, w in CASES])
def test_step_and_both_orientations(total, zero, rceil, rows, grid):
    """every shape as an identity and as an update bucket, clipping active: p' m' v' (and g with zero_grad) bit for
    bit, every rank's four outputs = mxfp8(p') and mxfp8(p'^T), gaps, guards, skew and the small buffer's sentinels
    unchanged; one launch.  At pipe_grid 5 a workgroup takes many units: the prefetch crosses units and both LDS
    images rotate.  rows = False: rows = scales = NULL in every bucket — ROWS = false in the trace, the t outputs the
    same, and the row buffers, allocated but not handed over, keep their sentinels."""
    lst = both_kinds(SHAPES_64 if total == 64 else SHAPES)
    data = make_data(total, lst, 10 * total)
    want = list_want(total, lst, 10 * total, zero, rceil)
    assert want[2][1] < 1 and want[2][2] == 0   # clipping is active, the step is not skipped
    for d, entry, o in zip(data, lst, want[1]):   # on the reference alone: a kernel that quantised the old parameter fails
        if entry[2] != "identity":
            assert not np.array_equal(o[2], quantised(d[P_], total, entry, rceil)[2])
    buckets = buckets_of(total, lst)
    planes = Planes(buckets, "flat" if grid else "wide", data)
    small = SmallG(gc.hyper_array(), adamw_cases.norm_sq(total))
    plan = base.any_plan(*SCHEDULES[total], total)
    with t.tuned(pipe_grid=grid):
        assert plan.adamw_shards_mxfp8_2d_launches(planes.args()) == 1
        with t.launch_trace() as tr:
            run(plan, planes, lst, small, zero, rceil, rows)
    assert tr.kernels == [kernel(total, zero, rceil, rows)] and (not grid or tr.grids == [grid])
    if not rows:   # what the row buffers must hold is what they held
        held = [tuple(h[:b.total, :w] for h, w in zip(b.r.host, (b.n, b.n // 32))) for b in buckets]
        want = (want[0], [h + o[2:] for h, o in zip(held, want[1])], want[2])
    check_all(buckets, planes, small, want, f"zero_grad={zero}, rceil={rceil}, rows={rows}")
    plan.close()


# ------------------------------------------------------------------ 2. the guarantee and 4. the skipped step, GPU against GPU
@pytest.mark.parametrize("skipped", [False, True], ids=["step", "skipped"])
@pytest.mark.parametrize("total,zero,rceil", [(8, False, True), (64, True, False)], ids=["swing-8", "swing-8x8"])
def test_planes_of_the_groups_call_outputs_of_the_2d_all_gather(total, zero, rceil, skipped):
    """allred.h's guarantee: the planes of adamw_all_gather_shards_f32_groups (its bf16 rows go to buffers nobody compares),
    the outputs of all_gather_shards_mxfp8_2d on the param plane it leaves.  skipped (an Inf in norm_sq): the planes keep
    their bits, the outputs are the quantisation of p, zero_grad still zeroes, info is what the groups call writes."""
    lst = both_kinds((SHAPES_64 if total == 64 else SHAPES)[:2])
    data = make_data(total, lst, 200 + total)
    nsq = adamw_cases.norm_sq(total).copy()
    if skipped:
        nsq[total - 1] = np.inf
    buckets = buckets_of(total, lst)
    planes = Planes(buckets, "flat", data)
    small, small2 = SmallG(gc.hyper_array(), nsq), SmallG(gc.hyper_array(), nsq)
    plan = base.any_plan(*SCHEDULES[total], total)
    run(plan, planes, lst, small, zero, rceil)
    want = expect(data, lst, total, nsq, zero, rceil)
    check_all(buckets, planes, small, want, "the numpy expectation")
    assert want[2][2] == (1 if skipped else 0)
    for d, v, entry, o in zip(data, want[0], lst, want[1]) if skipped else ():   # what the reference says of a skipped step
        assert all(np.array_equal(v[k].view(np.uint32), d[k].view(np.uint32)) for k in (P_, M_, V_))
        assert all(np.array_equal(a, b) for a, b in zip(o, quantised(d[P_], total, entry, rceil)))
        assert (v[G_].view(np.uint32) == 0).all() if zero else np.array_equal(v[G_].view(np.uint32), d[G_].view(np.uint32))
    new = [g.copy() for s in planes.s for g in s.got()]
    new_out = [b.r.got() + b.c.got() for b in buckets]
    planes.restore()
    args = planes.args()
    rows16, second = one.rows_buckets(total, [e[0] * e[1] // 256 for e in lst]), buckets_of(total, lst)
    with t.launch_trace() as tr:
        plan.adamw_all_gather_shards_f32_groups([r.arg + a[10:] for r, a in zip(rows16, args)], [e[3] for e in lst], small2.hyper, 3,
                                                small2.norm_sq, small2.info, zero_grad=zero, stream=stream())
        plan.all_gather_shards_mxfp8_2d([b.arg + (a[10], a[14]) for b, a in zip(second, args)], rceil=rceil, stream=stream())
    assert tr.kernels == [f"k_adamw_ag_groups_f32<{total}, {tf(zero)}>", m2.kernel(total, rceil)]
    old, old_out = [g for s in planes.s for g in s.got()], [b.r.got() + b.c.got() for b in second]
    for k, (a, b) in enumerate(zip(new, old)):
        assert f32_tree.same_f32(a.view(np.float32), b.view(np.float32)), f"plane buffer {k}"
    for i, (a, b) in enumerate(zip(new_out, old_out)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"bucket {i}: the four outputs"
    assert np.array_equal(groups.info_words(small), groups.info_words(small2))
    plan.close()


@pytest.mark.parametrize("count,launches", [(G, 1), (G + 1, 2), (2 * G + 1, 3)])
def test_16_buckets_per_launch_whatever_the_groups(count, launches):
    """mixed shapes, kinds and groups, every fourth bucket column-wise only: launch boundaries fall on every group in turn;
    info holds the call's four words (every launch would store the same: that launch 0 alone gets the pointer is the
    launcher's code, not something a value can show)"""
    total = 8
    lst = tuple(SHAPES[i % 3] + (("identity", 1) if i % 3 == 1 else ("planes", i % 3)) for i in range(count))
    data = make_data(total, lst, 100)
    buckets = [m2.Bucket2d(total, cols, R, skew=i % 3 == 0, rows=i % 4 != 3) for i, (cols, R, _, _) in enumerate(lst)]
    planes = Planes(buckets, "flat", data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    plan = base.any_plan(*SCHEDULES[total], total)
    assert plan.adamw_shards_mxfp8_2d_launches(planes.args()) == launches
    with t.launch_trace() as tr:
        run(plan, planes, lst, small, True, True)
    assert tr.count == launches and tr.kernels == [kernel(total, True, True)] * launches
    check_all(buckets, planes, small, expect(data, lst, total, nsq, True, True), f"{count} buckets")
    plan.close()


def test_one_capture_replayed_as_three_steps():
    """between replays hyper, norm_sq and the gradient planes are rewritten by copies on the capture's stream: three numpy steps"""
    total = 16
    lst = tuple((cols, R, "planes", g) for (cols, R), g in zip(SHAPES[:4], (0, 1, 2, 1)))
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
    plan = base.any_plan(*SCHEDULES[total], total)
    args, group_of = planes.args(), [e[3] for e in lst]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def call():
        plan.adamw_all_gather_shards_mxfp8_2d(args, group_of, small.hyper, 3, small.norm_sq, small.info, rceil=True, stream=s)
    with t.tuned(pipe_grid=5):
        with torch.cuda.stream(s):   # an eager call first: the capture loads no code
            call()
        s.synchronize()
        planes.restore()
        small.restore()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s), t.launch_trace() as tr:
            call()
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
        check_all(buckets, planes, small, want, f"replay {k + 1}")
        state = want[0]
    del g
    plan.close()


# ------------------------------------------------------------------ 6. refusals
def swap(a, k, v):
    return a[:k] + (v,) + a[k + 1:]


REFUSALS = {   # name: (status, what it changes: of bucket 1's tuple `a` or of the call's keywords)
    "a bad flag bit": (_lib.ERR_ARG, lambda a: dict(flags=4)),
    "ngroups 0": (_lib.ERR_ARG, lambda a: dict(ngroups=0)),
    "ngroups 9": (_lib.ERR_ARG, lambda a: dict(ngroups=9)),
    "a group index equal to ngroups": (_lib.ERR_ARG, lambda a: dict(group_of=(0, 3))),
    "rows NULL alone": (_lib.ERR_ARG, lambda a: dict(bucket=swap(a, 0, None))),
    "scales NULL alone": (_lib.ERR_ARG, lambda a: dict(bucket=swap(a, 2, None))),
    "a NULL plane": (_lib.ERR_ARG, lambda a: dict(bucket=swap(a, 11, None))),
    "cols % 32 != 0": (_lib.ERR_UNSUPPORTED, lambda a: dict(bucket=swap(a, 9, 16))),
    "nrows % (32 total) != 0": (_lib.ERR_UNSUPPORTED, lambda a: dict(bucket=swap(a, 9, 2 * a[9]))),
}   # the one-quantum overlap of the t rows with a plane block: the stride-gap test below, where nothing else can overlap


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
    plan = base.any_plan(*SCHEDULES[total], total)
    got = _lib.lib.allred_plan_adamw_all_gather_shards_mxfp8_2d(plan._h, arr, (C.c_uint8 * 2)(*kw["group_of"]), count, small.hyper,
                                                               kw["ngroups"], small.norm_sq, small.info, kw["flags"], None)
    assert got == status
    assert plan.adamw_shards_mxfp8_2d_launches(args) == 1   # the list itself is fine
    plan.close()
    planes.check(data, "written by a refused call")
    for b in buckets:
        b.check(None, "written by a refused call")
    small.check(None, "written by a refused call")


def test_a_stride_gap_filled_exactly_and_one_quantum_overlaps():
    """ONE buffer holds the param plane — 8 blocks of 1024 floats at a wide stride — and, in the gap behind block 0, the
    bucket's four output intervals, three hyper sets, norm_sq and info, filling it exactly: accepted, every byte what it
    must be.  Refused, with nothing written: the rows moved 16 bytes back — exactly one quantum of ONE output interval on
    block 0's tail, no other overlap —, the same for the t rows (rows = scales = NULL, the t rows where the rows stood),
    and a fourth hyper set (on norm_sq)."""
    total, cols, R = 8, 32, 32
    lst = ((cols, R, "planes", 2),)
    n, blk = total * R * cols, R * cols
    at = [int(x) for x in np.cumsum((4 * blk, total * n, total * n // 32, total * n, total * n // 32, 96, 4 * total, 16))]
    sst = at[-1] // 4   # rows, scales, t rows, t scales, hyper, norm_sq, info at at[0 .. 6]; the gap ends at at[7]
    nsq = adamw_cases.norm_sq(total)
    data = make_data(total, lst, 4)

    def image(k, values):
        """plane k of the bucket at the wide stride, the sentinel in every gap"""
        h = np.full((total, sst), base.SENT32, dtype=np.uint32)
        h[:, :blk] = values[0][k].view(np.uint32)
        return h.reshape(-1)
    host = image(P_, data).view(np.uint8).copy()
    host[at[4]:at[5]] = gc.hyper_array().reshape(-1).view(np.uint8)
    host[at[5]:at[6]] = nsq.view(np.uint8)
    bufs = [mxt.to_dev8(host)] + [base.to_dev32(image(k, data)) for k in (G_, M_, V_)]   # every plane at ONE stride
    ptr = bufs[0].data_ptr()
    out = (ptr + at[0], n, ptr + at[1], n // 32, ptr + at[2], n, ptr + at[3], n // 32)
    rest = (n, cols, ptr) + tuple(b.data_ptr() for b in bufs[1:]) + (sst,)
    small = (ptr + at[5], ptr + at[6])
    plan = base.any_plan(*SCHEDULES[total], total)
    assert plan.adamw_shards_mxfp8_2d_launches([out + rest]) == 1
    for o, ngroups in (((ptr + at[0] - 16,) + out[1:], 3), ((None, 0, None, 0, ptr + at[0] - 16) + out[5:], 3), (out, 4)):
        with pytest.raises(t.AllredError) as e:
            plan.adamw_all_gather_shards_mxfp8_2d([o + rest], (2,), ptr + at[4], ngroups, *small, stream=stream())
        assert e.value.status == _lib.ERR_ARG
    assert plan.adamw_shards_mxfp8_2d_launches([(None, 0, None, 0, ptr + at[0]) + out[5:] + rest]) == 1   # 16 bytes on: accepted
    assert np.array_equal(bufs[0].cpu().numpy(), host)
    assert all(np.array_equal(b.cpu().numpy().view(np.uint32), image(k, data)) for b, k in zip(bufs[1:], (G_, M_, V_)))
    plan.adamw_all_gather_shards_mxfp8_2d([out + rest], (2,), ptr + at[4], 3, *small, rceil=True, stream=stream())
    torch.cuda.synchronize()
    values, outs, info = expect(data, lst, total, nsq, False, True)
    want = host.copy()
    want.view(np.uint32).reshape(total, sst)[:, :blk] = values[0][P_].view(np.uint32)
    for k in range(4):
        want[at[k]:at[k + 1]] = np.tile(outs[0][k], total)
    want[at[6]:at[7]] = info.view(np.uint8)
    got = bufs[0].cpu().numpy()
    assert f32_tree.same_f32(got.view(np.float32), want.view(np.float32)) and np.array_equal(got[at[0]:at[4]], want[at[0]:at[4]])
    for b, k in zip(bufs[1:], (G_, M_, V_)):
        assert f32_tree.same_f32(b.cpu().numpy().view(np.float32), image(k, values).view(np.float32)), one.NAMES[k]
    plan.close()


def test_t_rows_feed_the_scaled_mfma():
    """a rank's t row of an update bucket of 32 columns is the 32 x 256 matrix p'^T in MX rows: rank 0's and the last rank's
    go through tests/mx_consumer.hip's helper where the call wrote them, and the MFMA reads them as p'^T dequantised"""
    import test_gpu_mx_consumer as mfma
    total, cols, R = 8, 32, 32
    lst = ((cols, R, "planes", 0),)
    nrows = total * R
    data = make_data(total, lst, 22)
    bk = m2.Bucket2d(total, cols, R, skew=True)
    planes = Planes([bk], "flat", data)
    nsq = adamw_cases.norm_sq(total)
    small = SmallG(gc.hyper_array(), nsq)
    plan = base.any_plan(*SCHEDULES[total], total)
    run(plan, planes, lst, small)
    want_all = expect(data, lst, total, nsq, False, False)
    check_all([bk], planes, small, want_all, "the rows the MFMA is about to read")
    we, ws = want_all[1][0][2:]
    want = ref.dequantize64(we, ws).reshape(cols, nrows)
    nan_rows = np.isnan(want).any(axis=1)
    assert not nan_rows.all()
    for r in (0, total - 1):
        got = mfma.every_element(bk.c.buf[0].data_ptr() + r * bk.c.row_stride, nrows, bk.c.buf[1].data_ptr() + r * bk.c.scale_stride,
                                 nrows // 32, cols, nrows)
        assert np.isnan(got[nan_rows]).all() and not np.isnan(got[~nan_rows]).any()
        mfma.report(f"rank {r}", mfma.same_value(got[~nan_rows], want[~nan_rows], f"rank {r}'s t row"))
    plan.close()
