"""The stochastically rounded MXFP4 all-gather (allred_plan_all_gather_shards_mxfp4_sr; k_ag_group_mxfp4_sr) against
t.mxfp4_sr_quantize, BIT FOR BIT, on test_gpu_shards_mxfp4's buffers: WHOLE buffers around sentinels, on
mx4_cases.shard's planted blocks (NaN, +-Inf, signed zeros, fp32 denormals, and the largest finite value, which
overflows under the rotation).  The state lives in device memory; a captured call follows its `step`."""
import functools

import numpy as np
import pytest

import mx4_cases
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_shards_f32 as f32t  # noqa: E402  (its Shards, schedules and parametrisations)
import test_gpu_shards_mxfp4 as mx4  # noqa: E402  (its buckets and list)
import test_gpu_shards_mxfp8 as mx8  # noqa: E402

pytestmark = pytest.mark.gpu
MASK, SEED = 0x9E3779B9, 0xC0FFEE0123456789
MODES = [(rceil, mask) for rceil in (False, True) for mask in (None, MASK)]


def state(step, seed=SEED):
    """allred_mx_sr_state in device memory: seed (two words), step, reserved (non-zero: it is ignored)"""
    return torch.from_numpy(np.array([seed & 0xFFFFFFFF, seed >> 32, step, 0xDEAD], dtype=np.uint32).view(np.int32)).to(f32t.DEV)


@functools.lru_cache(maxsize=None)
def expected(key, index, step, rceil, mask):
    """the rows of bucket `index` of the list: the gathered row is the shard's blocks end to end"""
    return t.mxfp4_sr_quantize(mx4.cases(*key).reshape(-1), SEED, step, index, rceil=rceil, sign_mask=mask)


def check_all(buckets, keys, step, rceil, mask, what):
    for i, (b, key) in enumerate(zip(buckets, keys)):
        b.check(b.after(*expected(key, i, step, rceil, mask)), f"bucket {i} (n={b.n}, step={step}, rceil={rceil}, mask={mask}): {what}")


def kernel(total, rceil, mask):
    return f"k_ag_group_mxfp4_sr<{total}, {'true' if rceil else 'false'}, {'false' if mask is None else 'true'}>"


@f32t.grids
@f32t.sched
def test_every_row_receives_the_sr_quantised_shard(algo, side, total, grid):
    """every P and the 1-D plan, 1 / 3 / 2 / 5 tiles per block (the peeled and the odd last tile), both scale rules,
    rotated or not; one launch"""
    buckets, keys = mx4.unequal(total)
    shards = mx4.filled(buckets, keys, "compact" if grid else "wide")
    plan, sr = f32t.any_plan(algo, side, total), state(3)
    with t.tuned(pipe_grid=grid):
        for rceil, mask in MODES:
            for b in buckets:
                b.restore()
            with t.launch_trace() as tr:
                plan.all_gather_shards_mxfp4_sr(shards.args(), sr.data_ptr(), sign_mask=mask, rceil=rceil, stream=f32t.stream())
            assert tr.kernels == [kernel(total, rceil, mask)]
            check_all(buckets, keys, 3, rceil, mask, "block b of every row = sr(shard block b)")
        mx8.shards_unchanged(shards)
    # the rounding is not RNE's, and the rotation's overflow block is there
    assert not np.array_equal(expected(keys[0], 0, 3, True, None)[0], mx4.expected(*keys[0], True)[0])
    assert (expected(keys[0], 0, 3, False, MASK)[1] == 0xFF).sum() > (expected(keys[0], 0, 3, False, None)[1] == 0xFF).sum()
    plan.close()


def test_the_bucket_index_is_the_lists_not_the_launchs():
    """33 one-tile buckets, two launches: bucket 32 holds bucket 0's data and is the second launch's first"""
    total, count = 8, 33
    buckets = [mx4.Mx4Bucket(total, 256 * total, skew=i % 3 == 0) for i in range(count)]
    keys = [(total, 256, i % 4) for i in range(count)]
    shards = mx4.filled(buckets, keys, "flat")
    plan, sr = f32t.any_plan(t.SWING, 4, total), state(1)
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp4_sr(shards.args(), sr.data_ptr(), rceil=True, stream=f32t.stream())
    assert tr.kernels == [kernel(total, True, None)] * 2
    check_all(buckets, keys, 1, True, None, "33 buckets in 2 launches")
    assert keys[32] == keys[0] and not np.array_equal(expected(keys[0], 0, 1, True, None)[0], expected(keys[0], 32, 1, True, None)[0])
    plan.close()


def test_captured_once_replayed_twice_with_step_rewritten_in_device_memory():
    total, rceil = 16, True
    buckets, keys = mx4.unequal(total, seed=3)
    shards = mx4.filled(buckets, keys, "wide")
    args, sr = shards.args(), state(10)
    plan = f32t.any_plan(t.SWING, 4, total)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):   # an eager call first: nothing is loaded inside the capture
        plan.all_gather_shards_mxfp4_sr(args, sr.data_ptr(), sign_mask=MASK, rceil=rceil, stream=s)
    s.synchronize()
    check_all(buckets, keys, 10, rceil, MASK, "eager")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.all_gather_shards_mxfp4_sr(args, sr.data_ptr(), sign_mask=MASK, rceil=rceil, stream=s)
    torch.cuda.synchronize()
    rows = []
    for step in (11, 12):
        sr[2] = step
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        check_all(buckets, keys, step, rceil, MASK, f"replay at step {step}")
        rows.append(buckets[0].got()[0].copy())
    assert not np.array_equal(rows[0], rows[1])
    mx8.shards_unchanged(shards)
    del g
    plan.close()


def test_a_refused_list_leaves_every_buffer_untouched():
    """sr NULL, misaligned, or inside a scale row; a flag bit beyond RCEIL | ROTATE; the older calls refuse ROTATE"""
    total = 8
    buckets, keys = mx4.unequal(total)
    shards = mx4.filled(buckets, keys, "compact")
    args, sr = shards.args(), state(0)
    plan = f32t.any_plan(t.SWING, 4, total)
    arr, count = plan._mx_buckets_f32(args)
    inside = buckets[2].buf[1].data_ptr() + buckets[2].scale_stride + 8   # rank 1's scale row of bucket 2
    for flags, ptr in ((0, None), (0, sr.data_ptr() + 4), (0, inside), (_lib.MX_SR_ROTATE, inside - 8), (4, sr.data_ptr())):
        assert _lib.lib.allred_plan_all_gather_shards_mxfp4_sr(plan._h, arr, count, flags, 0, ptr, None) == _lib.ERR_ARG, (flags, ptr)
    assert _lib.lib.allred_plan_all_gather_shards_mxfp4(plan._h, arr, count, _lib.MX_SR_ROTATE, None) == _lib.ERR_ARG
    assert _lib.lib.allred_plan_all_gather_shards_mxfp4_rht(plan._h, arr, count, _lib.MX_SR_ROTATE, 0, None) == _lib.ERR_ARG
    plan.close()
    torch.cuda.synchronize()
    for b in buckets:
        b.check(b.host, "written by a refused call")
    mx8.shards_unchanged(shards)
