"""The data of the norm tests, shared by the GPU file (tests/test_gpu_shards_f32_norm.py) and by the
CPU file that pins that these data tell a wrong order of operations from the right one
(tests/test_f32_norm.py).  Plain module: numpy and the library's host-side schedule only.

A case is a list of buckets; stored(case, ...) gives, per bucket, the (P, blk) float32 values the
call must store — tests/f32_tree.py's tree sums times scale, plus the old shard — and the expected
norm_sq is tests/f32_norm.py's over those.
"""
import functools

import numpy as np

import f32_tree
import hard_inputs
import tenstorrentallreduce_amd as t

SIDE = {8: 4, 16: 4, 32: 8, 64: 8}
SCHEDULES = [(algo, SIDE[total], total) for total in (8, 16, 32, 64) for algo in (t.SWING, t.RECDUB)]
SCHEDULES.append((t.SWING_1D, 1, 8))
SCHEDULE_IDS = [f"algo{a}-{s}x{p}" for a, s, p in SCHEDULES]
UNEQUAL = (1, 3, 2, 5)                      # tiles per block of the unequal list: 11 partials per rank
SCALES = lambda total: (1.0, 1.0 / total, 0.1)   # noqa: E731
STRIDED = (8, (5,) * 16)                    # P = 8, sixteen buckets of 5 tiles per block: 80 partials per rank, past 64
CHAIN_COUNTS = (64, 65, 130)                # buckets of one tile per block at P = 8: one, two and three launches


@functools.lru_cache(maxsize=None)
def tree_order(algo, side, total):
    return tuple(tuple(row) for row in t.schedule(algo, side, total)["tree_order"])


@functools.lru_cache(maxsize=None)
def sums(kind, algo, side, total, n, seed):
    """(inputs (total, n) uint16, their per-block fp32 tree sums (total, blk)), computed once, read-only"""
    data = getattr(hard_inputs, kind)(total, n, seed)
    data.flags.writeable = False
    s = f32_tree.tree_sums(data, tree_order(algo, side, total))
    s.flags.writeable = False
    return data, s


def bucket_list(algo, side, total, tiles, kind="cancel", seed=0):
    """[(data, sums)] for buckets of tiles[i] tiles per block"""
    return [sums(kind, algo, side, total, 256 * total * k, 100 * seed + i) for i, k in enumerate(tiles)]


def stored(buckets, scale, old=None):
    """what the call stores: per bucket sums * scale, then old[i] + that"""
    return [f32_tree.scaled(s, scale, None if old is None else old[i]) for i, (_, s) in enumerate(buckets)]


def random_floats(rng, shape, lo_exp=100, hi_exp=150):
    """finite float32 of both signs whose squares are finite: magnitudes 2^(lo_exp - 127) .. 2^(hi_exp - 126)"""
    bits = (rng.integers(0, 2, shape, dtype=np.uint32) << 31) | (rng.integers(lo_exp, hi_exp, shape, dtype=np.uint32) << 23) \
        | rng.integers(0, 1 << 23, shape, dtype=np.uint32)
    return bits.view(np.float32)
