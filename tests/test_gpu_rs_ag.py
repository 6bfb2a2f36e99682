"""Reduce-scatter and all-gather on a virtual-rank plan (allred_plan_reduce_scatter /
allred_plan_all_gather), fused and steps form, against the CPU oracle.

The arithmetic is deterministic and the add order is specified (block b = tree b of
the schedule, every add rounded to bf16), so every comparison is BIT-EXACT: the
expected reduce-scatter value is block b of the oracle's BO allreduce of the same
inputs, the all-gather is a pure 16-bit copy, and the two in sequence are
Plan.execute.  In-place cases lay the rows out at preferred_rank_stride with a
sentinel in the stride skew and one guard row behind the last rank: whatever a call
must not touch is compared with its input bits.

Shapes, the smallest that reach each kernel: blocks of 3 vectors (several blocks per
wave: the register form, per-lane owner rows), blocks of 2 whole tiles (8+ ranks: one
tile per workgroup through LDS), and 64 x 327,680 (1280 tiles on at most 512
workgroups: the persistent form, 2 or 3 tiles per workgroup)."""
import functools

import numpy as np
import pytest

import oracle
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5A5

GRIDS = [(1, 1), (2, 2), (2, 4), (4, 8), (4, 16), (8, 64)]
SCHEDULES = [(algo, side, total) for side, total in GRIDS for algo in (t.SWING, t.RECDUB)]
SCHEDULES += [(algo, 1, total) for total in (8, 64) for algo in (t.SWING_1D, t.RECDUB_1D)]
CASES = [(a, s, p, 8 * p * 3) for a, s, p in SCHEDULES] + [(a, s, p, 256 * p * 2) for a, s, p in SCHEDULES]
CASES += [(t.SWING, 8, 64, 327680), (t.RECDUB, 8, 64, 327680)]
IDS = [f"algo{a}-{s}x{p}-n{n}" for a, s, p, n in CASES]
case = pytest.mark.parametrize("algo,side,total,n", CASES, ids=IDS)


@functools.lru_cache(maxsize=None)
def reference(algo, side, total, n):
    """(inputs, oracle BO allreduce of them), both (total, n) uint16, computed once and read-only."""
    rng = np.random.default_rng(1000 * total + 10 * algo + n % 97)
    data = rng.integers(0x3F80, 0x42C8, (total, n)).astype(np.uint16)
    want = [r.copy() for r in data]
    oracle.allreduce("bo", algo, side, want, total)
    want = np.stack(want)
    data.flags.writeable = False
    want.flags.writeable = False
    return data, want


def raw_bits(total, n, seed):
    """arbitrary 16-bit patterns: NaN payloads, infinities, denormals"""
    return np.random.default_rng(seed).integers(0, 0x10000, (total, n)).astype(np.uint16)


def rows(data):
    """(host image, device buffer, stride): rows at preferred_rank_stride, the skew and a guard row = SENT"""
    total, n = data.shape
    stride = t.preferred_rank_stride(n)
    host = np.full((total + 1, stride), SENT, dtype=np.uint16)
    host[:total, :n] = data
    return host, to_dev(host), stride


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV)


def from_dev(buf):
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint16)


def owner_blocks(a, total, n):
    """block b of row b, for every b: (total, blk)"""
    blk = n // total
    return np.stack([a[b, b * blk:(b + 1) * blk] for b in range(total)])


def put_owner_blocks(dst, src, total, n):
    blk = n // total
    for b in range(total):
        dst[b, b * blk:(b + 1) * blk] = src[b, b * blk:(b + 1) * blk]


def stream():
    return torch.cuda.current_stream()


# ------------------------------------------------------------------ reduce-scatter
@case
def test_fused_reduce_scatter_in_place(algo, side, total, n):
    """Block b of rank b = the oracle's block b; every other element of the buffer —
    the other blocks, the skew, the guard row — keeps its input bits."""
    data, want = reference(algo, side, total, n)
    host, buf, stride = rows(data)
    plan = t.Plan(algo, t.BO, side, n, total, t.EXEC_FUSED)
    plan.reduce_scatter(buf.data_ptr(), stride, stream=stream())
    got = from_dev(buf)
    plan.close()
    expect = host.copy()
    put_owner_blocks(expect, want, total, n)
    assert np.array_equal(owner_blocks(got, total, n), owner_blocks(want, total, n))
    assert np.array_equal(got, expect)


@case
def test_steps_reduce_scatter_in_place(algo, side, total, n):
    """The reference's reduce-scatter loop alone: owner blocks = the oracle (the other
    blocks hold partial sums, unspecified); skew and guard row untouched."""
    data, want = reference(algo, side, total, n)
    host, buf, stride = rows(data)
    plan = t.Plan(algo, t.BO, side, n, total, t.EXEC_STEPS)
    plan.reduce_scatter(buf.data_ptr(), stride, stream=stream())
    got = from_dev(buf)
    plan.close()
    assert np.array_equal(owner_blocks(got, total, n), owner_blocks(want, total, n))
    assert (got[:total, n:] == SENT).all() and (got[total] == SENT).all()


@case
def test_fused_reduce_scatter_out_of_place(algo, side, total, n):
    """out rows (stride blk + 8) = the oracle's blocks, the gaps untouched, ranks unchanged bit for bit."""
    data, want = reference(algo, side, total, n)
    host, buf, stride = rows(data)
    blk = n // total
    out = to_dev(np.full((total + 1, blk + 8), SENT, dtype=np.uint16))
    plan = t.Plan(algo, t.BO, side, n, total, t.EXEC_FUSED)
    plan.reduce_scatter(buf.data_ptr(), stride, out.data_ptr(), blk + 8, stream=stream())
    got_out, got = from_dev(out), from_dev(buf)
    plan.close()
    assert np.array_equal(got_out[:total, :blk], owner_blocks(want, total, n))
    assert (got_out[:total, blk:] == SENT).all() and (got_out[total] == SENT).all()
    assert np.array_equal(got, host)


@pytest.mark.parametrize("form", [1, 2, 3], ids=["register", "one-tile", "persistent"])
@pytest.mark.parametrize("side,total", [(4, 8), (4, 16), (8, 32), (8, 64)])
def test_fused_reduce_scatter_forms_agree(side, total, form):
    """The tune key fused_form forces each kernel form on a whole-tile bucket (3 tiles per
    block, so the persistent form's workgroups straddle nothing): the register form with
    uniform waves, one tile per workgroup, and the persistent form at 8 / 16 / 32 / 64
    ranks — the same bits in place and out of place."""
    n = 256 * total * 3
    blk = n // total
    data, want = reference(t.SWING, side, total, n)
    host, buf, stride = rows(data)
    out = to_dev(np.full((total, blk), SENT, dtype=np.uint16))
    plan = t.Plan(t.SWING, t.BO, side, n, total, t.EXEC_FUSED)
    with t.tuned(fused_form=form):
        plan.reduce_scatter(buf.data_ptr(), stride, out.data_ptr(), blk, stream=stream())
        plan.reduce_scatter(buf.data_ptr(), stride, stream=stream())
    got, got_out = from_dev(buf), from_dev(out)
    plan.close()
    expect = host.copy()
    put_owner_blocks(expect, want, total, n)
    assert np.array_equal(got_out, owner_blocks(want, total, n))
    assert np.array_equal(got, expect)


# ------------------------------------------------------------------ all-gather
@pytest.mark.parametrize("exec_mode", [t.EXEC_FUSED, t.EXEC_STEPS], ids=["fused", "steps"])
@case
def test_all_gather_in_place(algo, side, total, n, exec_mode):
    """Every rank's block b = rank b's input block b, all 16 bits (NaN and inf patterns
    included); skew and guard row untouched."""
    data = raw_bits(total, n, seed=total + n + algo)
    host, buf, stride = rows(data)
    plan = t.Plan(algo, t.BO, side, n, total, exec_mode)
    plan.all_gather(buf.data_ptr(), stride, stream=stream())
    got = from_dev(buf)
    plan.close()
    expect = host.copy()
    expect[:total, :n] = owner_blocks(data, total, n).reshape(-1)[None, :]
    assert np.array_equal(got, expect)


@case
def test_fused_all_gather_out_of_place(algo, side, total, n):
    """Block b read from in + b * in_stride: every rank row = the in rows in order; in unchanged."""
    blk = n // total
    src = raw_bits(total + 1, blk + 8, seed=3 * total + n + algo)
    host, buf, stride = rows(raw_bits(total, n, seed=5 * total + n + algo))
    din = to_dev(src)
    plan = t.Plan(algo, t.BO, side, n, total, t.EXEC_FUSED)
    plan.all_gather(buf.data_ptr(), stride, din.data_ptr(), blk + 8, stream=stream())
    got, got_in = from_dev(buf), from_dev(din)
    plan.close()
    expect = host.copy()
    expect[:total, :n] = src[:total, :blk].reshape(-1)[None, :]
    assert np.array_equal(got, expect)
    assert np.array_equal(got_in, src)


# ------------------------------------------------------------------ composition
@pytest.mark.parametrize("rs_exec,ag_exec", [(t.EXEC_FUSED, t.EXEC_FUSED), (t.EXEC_STEPS, t.EXEC_STEPS),
                                             (t.EXEC_FUSED, t.EXEC_STEPS), (t.EXEC_STEPS, t.EXEC_FUSED)],
                         ids=["fused-fused", "steps-steps", "fused-steps", "steps-fused"])
@case
def test_reduce_scatter_then_all_gather_is_the_allreduce(algo, side, total, n, rs_exec, ag_exec):
    data, want = reference(algo, side, total, n)
    host, buf, stride = rows(data)
    whole = buf.clone()
    plans = {e: t.Plan(algo, t.BO, side, n, total, e) for e in {rs_exec, ag_exec, t.EXEC_FUSED}}
    plans[rs_exec].reduce_scatter(buf.data_ptr(), stride, stream=stream())
    plans[ag_exec].all_gather(buf.data_ptr(), stride, stream=stream())
    plans[t.EXEC_FUSED].execute(whole.data_ptr(), stride, None, stream())
    got, ref = from_dev(buf), from_dev(whole)
    for p in plans.values():
        p.close()
    assert np.array_equal(got, ref)
    assert np.array_equal(got[:total, :n], want)
    assert (got[:total, n:] == SENT).all() and (got[total] == SENT).all()


# ------------------------------------------------------------------ argument checks
def test_argument_checks_refuse_before_any_launch():
    algo, side, total = t.SWING, 4, 8
    n = 256 * total * 2
    blk = n // total
    data, _ = reference(algo, side, total, n)
    host, buf, stride = rows(data)
    side_host = np.full((total, blk + 8), SENT, dtype=np.uint16)
    side_buf = to_dev(side_host)
    s = stream()

    def refused(status, call):
        with pytest.raises(t.AllredError) as e:
            call()
        assert e.value.status == status, (e.value.status, status)

    for variant in (t.LO, t.MEM):
        plan = t.Plan(algo, variant, side, n, total, t.EXEC_FUSED)
        refused(t._lib.ERR_UNSUPPORTED, lambda: plan.reduce_scatter(buf.data_ptr(), stride, stream=s))
        refused(t._lib.ERR_UNSUPPORTED, lambda: plan.all_gather(buf.data_ptr(), stride, stream=s))
        plan.close()
    steps = t.Plan(algo, t.BO, side, n, total, t.EXEC_STEPS)
    refused(t._lib.ERR_UNSUPPORTED,
            lambda: steps.reduce_scatter(buf.data_ptr(), stride, side_buf.data_ptr(), blk + 8, stream=s))
    refused(t._lib.ERR_UNSUPPORTED,
            lambda: steps.all_gather(buf.data_ptr(), stride, side_buf.data_ptr(), blk + 8, stream=s))
    fused = t.Plan(algo, t.BO, side, n, total, t.EXEC_FUSED)
    for plan in (steps, fused):
        refused(t._lib.ERR_ARG, lambda: plan.reduce_scatter(buf.data_ptr(), n - 8, stream=s))
        refused(t._lib.ERR_ARG, lambda: plan.all_gather(buf.data_ptr(), n - 8, stream=s))
    for fn in (fused.reduce_scatter, fused.all_gather):
        refused(t._lib.ERR_ARG, lambda: fn(buf.data_ptr(), stride, side_buf.data_ptr() + 2, blk + 8, stream=s))
        refused(t._lib.ERR_ARG, lambda: fn(buf.data_ptr(), stride, side_buf.data_ptr(), blk - 8, stream=s))
        refused(t._lib.ERR_ARG, lambda: fn(buf.data_ptr(), stride, side_buf.data_ptr(), blk + 4, stream=s))
        # the side buffer inside the rank rows, and ending inside them
        refused(t._lib.ERR_ARG, lambda: fn(buf.data_ptr(), stride, buf.data_ptr() + 2 * stride, blk, stream=s))
        refused(t._lib.ERR_ARG,
                lambda: fn(buf.data_ptr() + 2 * stride, stride, buf.data_ptr(), stride, stream=s))
    steps.close()
    fused.close()
    assert np.array_equal(from_dev(buf), host)
    assert np.array_equal(from_dev(side_buf), side_host)


# ------------------------------------------------------------------ the RCCL path on one GPU
def test_single_rank_rccl_reduce_scatter_and_all_gather():
    """A one-rank communicator: rank 0 owns its one block and the program has no steps —
    both calls return OK and leave the bucket's bits unchanged."""
    comm = t.Comm(t.Comm.unique_id(), 1, 0, 0)
    n = 8 * 64 * 4
    data = raw_bits(1, n, seed=7)[0]
    buf = to_dev(data)
    desc = t.dist_desc(t.SWING, t.BO, 1, 1, n)
    ws = torch.empty(t.dist_workspace_bytes(desc), dtype=torch.uint8, device=DEV)
    t.dist_reduce_scatter(comm, desc, buf.data_ptr(), ws.data_ptr(), stream())
    t.dist_all_gather(comm, desc, buf.data_ptr(), ws.data_ptr(), stream())
    assert np.array_equal(from_dev(buf), data)
    for bad in (t.dist_desc(t.SWING, t.LO, 1, 1, n), t.dist_desc(t.SWING, t.MEM, 1, 1, n),
                t.dist_desc(t.SWING, t.BO, 1, 1, n, channels=2),
                t.dist_desc(t.SWING, t.BO, 1, 1, n, local_ranks=4, local_side=2)):
        for fn in (t.dist_reduce_scatter, t.dist_all_gather):
            with pytest.raises(t.AllredError) as e:
                fn(comm, bad, buf.data_ptr(), ws.data_ptr(), stream())
            assert e.value.status == t._lib.ERR_UNSUPPORTED
    comm.close()
