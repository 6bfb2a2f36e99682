"""The rotated MXFP4 all-gather (allred_plan_all_gather_shards_mxfp4_rht; k_ag_group_mxfp4_rht) against
tests/mxfp4_rht_ref.py, BIT FOR BIT, on test_gpu_shards_mxfp4's buffers: WHOLE buffers around sentinels.  Two data
sets, both needed: mx4_cases.shard (NaN, +-Inf, denormals, and the largest finite value, whose butterfly overflows: a
0xFF block) and mxfp4_rht_ref.cancel_shard, on which — unlike on random data — a wrong stage order, operand order or
sign bit changes nibbles."""
import functools

import numpy as np
import pytest

import mx4_cases
import mxfp4_rht_ref as ref
import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

torch = pytest.importorskip("torch")
import test_gpu_shards_f32 as f32t  # noqa: E402  (its Shards, schedules and parametrisations)
import test_gpu_shards_mxfp4 as mx4  # noqa: E402  (its buckets and list)
import test_gpu_shards_mxfp8 as mx8  # noqa: E402

pytestmark = pytest.mark.gpu
MASKS = (0, 0xFFFFFFFF, 0x9E3779B9)
DATA = {"hard": mx4_cases.shard, "cancel": ref.cancel_shard}


@functools.lru_cache(maxsize=None)
def cases(kind, total, blk, seed):
    return DATA[kind](total, blk, seed)


@functools.lru_cache(maxsize=None)
def expected(key, mask, rceil):
    return ref.expected_rows(cases(*key), mask, rceil)


def keys_of(kind, keys):
    return [(kind,) + k for k in keys]


def check_all(buckets, keys, mask, rceil, what):
    for i, (b, key) in enumerate(zip(buckets, keys)):
        b.check(b.after(*expected(key, mask, rceil)), f"bucket {i} (n={b.n}, mask={mask:#x}, rceil={rceil}): {what}")


def kernel(total, rceil):
    return f"k_ag_group_mxfp4_rht<{total}, {'true' if rceil else 'false'}>"


@f32t.grids
@pytest.mark.parametrize("kind,layout", [("hard", "compact"), ("cancel", "wide")])
@f32t.sched
def test_every_row_receives_the_rotated_quantised_shard(algo, side, total, kind, layout, grid):
    """every P and the 1-D plan, 1 / 3 / 2 / 5 tiles per block, both scale rules, three masks; one launch"""
    buckets, keys = mx4.unequal(total)
    keys = keys_of(kind, keys)
    shards = f32t.Shards(buckets, layout)
    shards.fill([cases(*k) for k in keys])
    plan = f32t.any_plan(algo, side, total)
    if kind == "hard":   # the largest finite value overflows in the butterfly: more 0xFF blocks than NaN and Inf inputs
        assert (expected(keys[0], 0, False)[1] == 0xFF).sum() > (mx4.expected(*keys[0][1:], False)[1] == 0xFF).sum()
    with t.tuned(pipe_grid=grid):
        for rceil in (False, True):
            for mask in MASKS:
                for b in buckets:
                    b.restore()
                with t.launch_trace() as tr:
                    plan.all_gather_shards_mxfp4_rht(shards.args(), mask, rceil=rceil, stream=f32t.stream())
                assert tr.kernels == [kernel(total, rceil)]
                check_all(buckets, keys, mask, rceil, "block b of every row = mxfp4(rotated shard block b)")
        mx8.shards_unchanged(shards)
    plan.close()


def test_captured_once_replayed_twice_on_rewritten_shards():
    """the tables and the mask travel by value: one capture on a side stream, two replays, the shards rewritten in between"""
    total, mask, rceil = 16, MASKS[2], True
    buckets, keys = mx4.unequal(total, seed=3)
    shards = f32t.Shards(buckets, "wide")
    shards.fill([cases("cancel", *k) for k in keys])
    args = shards.args()
    plan = f32t.any_plan(t.SWING, 4, total)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):   # an eager call first: nothing is loaded inside the capture
        plan.all_gather_shards_mxfp4_rht(args, mask, rceil=rceil, stream=s)
    s.synchronize()
    check_all(buckets, keys_of("cancel", keys), mask, rceil, "eager")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.all_gather_shards_mxfp4_rht(args, mask, rceil=rceil, stream=s)
    torch.cuda.synchronize()
    for kind in ("hard", "cancel"):
        ks = keys_of(kind, keys)
        shards.fill([cases(*k) for k in ks])
        for b in buckets:
            b.restore()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        check_all(buckets, ks, mask, rceil, f"replay on {kind}")
        mx8.shards_unchanged(shards)
    del g
    plan.close()


def test_a_refused_list_leaves_every_buffer_untouched():
    """the MXFP4 call's checks: a row stride below n / 2 and an unknown flag bit are refused, nothing is written"""
    total = 8
    buckets, keys = mx4.unequal(total)
    shards = f32t.Shards(buckets, "compact")
    shards.fill([cases("hard", *k) for k in keys])
    args = shards.args()
    rows, rs, scales, ss, n, shard, sst = args[-1]
    plan = f32t.any_plan(t.SWING, 4, total)
    with pytest.raises(t.AllredError) as e:
        plan.all_gather_shards_mxfp4_rht(args[:-1] + [(rows, n // 2 - 16, scales, ss, n, shard, sst)], MASKS[2], stream=f32t.stream())
    assert e.value.status == _lib.ERR_ARG
    arr, count = plan._mx_buckets_f32(args)
    assert _lib.lib.allred_plan_all_gather_shards_mxfp4_rht(plan._h, arr, count, 2, 0, None) == _lib.ERR_ARG
    plan.close()
    for b in buckets:
        b.check(b.host, "written by a refused call")
    mx8.shards_unchanged(shards)
