"""The 2D MXFP4 all-gather with stochastically rounded, optionally rotated column-wise rows
(allred_plan_all_gather_shards_mxfp4_2d_sr and its _launches twin; k_ag_group_mxfp4_2d_sr), BIT FOR BIT, whole buffers
around sentinel skews and guard rows, on test_gpu_shards_mxfp4_2d's buckets.  The t rows are held against
t.mxfp4_sr_quantize on W^T flattened — the 1D SR call's host rule —, the rows against the RNE call's expectation."""
import functools

import numpy as np
import pytest

import mx4_2d_ref as r2
import mxfp4_rht_ref as rht
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_shards_f32 as f32t  # noqa: E402
import test_gpu_shards_mxfp4_2d as m4  # noqa: E402  (its buckets, matrices and RNE expectation)
import test_gpu_shards_mxfp4_sr as sr1  # noqa: E402  (the state, MASK, SEED, MODES)
import test_gpu_shards_mxfp8 as mx8  # noqa: E402

pytestmark = pytest.mark.gpu
Shards, stream, state, MASK = f32t.Shards, f32t.stream, sr1.state, sr1.MASK
G = _lib.MX4_2D_SR_GROUP_MAX
# one column square; partial 128-column strips with strips across block ends at R = 160; R = 32: every strip crosses
# block ends; every P instantiation
SHAPES = ((8, 32, 32), (8, 160, 160), (16, 64, 32), (32, 32, 96), (64, 32, 32))


def cancel_t(total, cols, R, seed):
    """(nrows, cols) float32 whose transpose, flattened, is rht.cancel_shard: the cancelling pairs lie down the columns"""
    return np.ascontiguousarray(rht.cancel_shard(1, total * R * cols, seed).reshape(cols, total * R).T)


@functools.lru_cache(maxsize=None)
def matrix(kind, total, cols, R, seed):
    return cancel_t(total, cols, R, seed) if kind == "cancel_t" else m4.matrix(kind, total, cols, R, seed)


@functools.lru_cache(maxsize=None)
def expected(kind, key, index, step, rceil, mask):
    """(rows, scales, t rows, t scales) of bucket `index` of the list"""
    W = matrix(kind, *key)
    return r2.expected(W, key[0], rceil)[:2] + t.mxfp4_sr_quantize(W.T.reshape(-1), sr1.SEED, step, index, rceil=rceil, sign_mask=mask)


def kernel(total, rceil, rows, mask):
    return f"k_ag_group_mxfp4_2d_sr<{total}, {m4.m2.tf(rceil)}, {m4.m2.tf(rows)}, {m4.m2.tf(mask is not None)}>"


def fill(shards, kind, keys):
    shards.fill([matrix(kind, *k).reshape(k[0], -1) for k in keys])


def check_all(buckets, kind, keys, step, rceil, mask, what):
    for i, (b, k) in enumerate(zip(buckets, keys)):
        b.check(expected(kind, k, i, step, rceil, mask), f"bucket {i} (cols={b.cols}, R={b.R}, {kind}, step={step}, rceil={rceil}, mask={mask}): {what}")


# ------------------------------------------------------------------ 1. every rank's four outputs
@pytest.mark.parametrize("grid", [0, 5], ids=["default-grid", "grid5"])
@pytest.mark.parametrize("rows", [True, False], ids=["rows", "t-only"])
@pytest.mark.parametrize("total,cols,R", SHAPES)
def test_rows_are_rne_and_t_rows_are_the_sr_call_on_the_transpose(total, cols, R, rows, grid):
    buckets, keys = m4.make(total, [(cols, R)], rows=lambda i: rows)
    shards = Shards(buckets, "wide")
    plan, sr = m4.plan_for(total), state(3)
    with t.tuned(pipe_grid=grid):
        for kind in ("hard_t", "cancel_t"):
            fill(shards, kind, keys)
            for rceil, mask in sr1.MODES:
                if kind == "cancel_t" and mask is None:
                    continue   # the cancelling pairs are there for the rotation's stage and operand order
                buckets[0].restore()
                with t.launch_trace() as tr:
                    plan.all_gather_shards_mxfp4_2d_sr(shards.args(), sr.data_ptr(), sign_mask=mask, rceil=rceil, stream=stream())
                assert tr.kernels == [kernel(total, rceil, rows, mask)] and (not grid or tr.grids == [min(grid, m4.units(total, cols, R))])
                check_all(buckets, kind, keys, 3, rceil, mask, "rows = mxfp4(W), t rows = mxfp4_sr(W^T)")
            mx8.shards_unchanged(shards)
    e = expected("hard_t", keys[0], 0, 3, True, None)
    assert not np.array_equal(e[2], m4.expected("hard_t", *keys[0], True)[2]), "the t rows are not RNE's"
    plan.close()


# ------------------------------------------------------------------ 2. the counter's bucket word
def test_the_bucket_index_is_the_lists_not_the_launchs():
    """G + 1 one-square buckets, two launches: bucket G holds bucket 0's matrix and is the second launch's first"""
    total = 8
    buckets = [m4.Bucket2d(total, 32, 32, skew=i % 3 == 0, rows=i % 2 == 0) for i in range(G + 1)]
    keys = [(total, 32, 32, i % 4) for i in range(G + 1)]
    shards = Shards(buckets, "flat")
    fill(shards, "hard_t", keys)
    plan, sr = m4.plan_for(total), state(1)
    assert [plan.shards_mxfp4_2d_sr_launches(shards.args()[:k]) for k in (0, G, G + 1)] == [0, 1, 2]
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp4_2d_sr(shards.args(), sr.data_ptr(), sign_mask=MASK, rceil=True, stream=stream())
    assert tr.kernels == [kernel(total, True, True, MASK)] * 2
    check_all(buckets, "hard_t", keys, 1, True, MASK, f"{G + 1} buckets in 2 launches")
    assert keys[G] == keys[0] and not np.array_equal(expected("hard_t", keys[0], 0, 1, True, MASK)[2], expected("hard_t", keys[0], G, 1, True, MASK)[2])
    plan.close()


# ------------------------------------------------------------------ 3. graph replay follows the state
def test_captured_once_replayed_twice_with_step_rewritten_in_device_memory():
    total, rceil = 16, False
    buckets, keys = m4.make(total, [(64, 32), (96, 64), (32, 96)], rows=lambda i: i != 1, seed=3)
    shards = Shards(buckets, "wide")
    fill(shards, "hard_t", keys)
    args, sr = shards.args(), state(10)
    plan = m4.plan_for(total)
    s = torch.cuda.Stream()
    with t.tuned(pipe_grid=5):
        with torch.cuda.stream(s):   # an eager call first: nothing is loaded inside the capture
            plan.all_gather_shards_mxfp4_2d_sr(args, sr.data_ptr(), sign_mask=MASK, rceil=rceil, stream=s)
        s.synchronize()
        check_all(buckets, "hard_t", keys, 10, rceil, MASK, "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s), t.launch_trace() as tr:
            plan.all_gather_shards_mxfp4_2d_sr(args, sr.data_ptr(), sign_mask=MASK, rceil=rceil, stream=s)
    torch.cuda.synchronize()
    assert tr.kernels == [kernel(total, rceil, True, MASK)] and len(tr.kernels) == plan.shards_mxfp4_2d_sr_launches(args)
    got = []
    for step in (11, 12):
        sr[2] = step
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        check_all(buckets, "hard_t", keys, step, rceil, MASK, f"replay at step {step}")
        got.append(buckets[0].c.got()[0].copy())
    assert not np.array_equal(got[0], got[1])
    mx8.shards_unchanged(shards)
    del g
    plan.close()


# ------------------------------------------------------------------ 4. refusals
def test_a_refused_list_leaves_every_buffer_untouched():
    total = 8
    buckets, keys = m4.make(total, [(32, 32), (64, 32)])
    shards = Shards(buckets, "compact")
    fill(shards, "hard_t", keys)
    args, sr = shards.args(), state(0)
    plan = m4.plan_for(total)
    arr, count = plan._mx2d_buckets_f32(args)
    inside = buckets[1].c.buf[1].data_ptr() + buckets[1].c.scale_stride + 8   # rank 1's t scale row of bucket 1
    ARG, call = _lib.ERR_ARG, _lib.lib.allred_plan_all_gather_shards_mxfp4_2d_sr
    for flags, ptr in ((0, None), (0, sr.data_ptr() + 4), (0, inside), (_lib.MX_SR_ROTATE, inside - 8), (4, sr.data_ptr())):
        assert call(plan._h, arr, count, flags, 0, ptr, None) == ARG, (flags, ptr)
    narrow, _ = plan._mx2d_buckets_f32([a[:9] + (16,) + a[10:] for a in args])   # cols = 16
    assert call(plan._h, narrow, count, 0, 0, sr.data_ptr(), None) == _lib.ERR_UNSUPPORTED
    assert _lib.lib.allred_plan_all_gather_shards_mxfp4_2d_sr_launches(plan._h, narrow, count) == _lib.ERR_UNSUPPORTED
    assert _lib.lib.allred_plan_all_gather_shards_mxfp4_2d(plan._h, arr, count, _lib.MX_SR_ROTATE, None) == ARG
    plan.close()
    torch.cuda.synchronize()
    for b in buckets:
        b.check(None, "written by a refused call")
    mx8.shards_unchanged(shards)
