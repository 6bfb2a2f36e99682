"""tests/f32_norm.py — the expectation of allred_plan_reduce_scatter_shards_f32_norm — on the CPU:
its rules on small known answers, and that the DATA of the GPU tests (tests/f32_norm_cases.py)
discriminate: on the exact values of every GPU case that claims to check the order of operations,
each plausible wrong order changes at least one rank's norm_sq bit pattern.  A GPU test that
passes on such data has therefore computed the stated order and none of these."""
import numpy as np
import pytest

import f32_norm
import f32_norm_cases as cases
import f32_tree

ALTERNATIVES = {
    "a left-to-right sum of the tile": dict(partial=f32_norm.tile_partials_sequential),
    "an fma chain inside the lane": dict(partial=f32_norm.tile_partials_fma),
    "the c levels before the q level": dict(partial=f32_norm.tile_partials_c_first),
    "a plain sequential sum of the partials": dict(combine=f32_norm.launch_sum_sequential),
}


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


COMBINE = ("a plain sequential sum of the partials",)   # what a list of many partials per rank is there for


def assert_discriminates(values, what, names=tuple(ALTERNATIVES)):
    want = f32_norm.expect_norm_sq(values)
    assert np.isfinite(want).all() and (want > 0).all(), what
    for name in names:
        alt = ALTERNATIVES[name]
        other = f32_norm.expect_norm_sq(values, **alt)
        assert (bits(other) != bits(want)).any(), f"{what}: {name} gives the same norm_sq in every rank"


# ------------------------------------------------------------------ the rules themselves
def test_tile_partial_is_the_balanced_tree_in_element_order():
    x = np.zeros(256, dtype=np.float32)
    x[0], x[1], x[2] = 4096.0, 1.0, 1.0          # 2^24 + 1 rounds to 2^24 (tie to even): the pair (x0, x1) loses the 1
    assert f32_norm.tile_partial(x) == np.float32(2.0 ** 24)             # (2^24 + 1) + (1 + 0) = 2^24 + 1 -> 2^24 (tie to even)
    x[3] = 1.0
    assert f32_norm.tile_partial(x) == np.float32(2.0 ** 24 + 2)         # (2^24 + 1 -> 2^24) + (1 + 1)
    assert f32_norm.tile_partials_sequential(x)[0] == np.float32(2.0 ** 24)   # left to right every 1 is lost
    # the lane's four first, then q, then c: elements 4 (2 c + q) .. + 3 are lane (q, c)'s
    rng = np.random.default_rng(0)
    x = rng.standard_normal(256).astype(np.float32)
    sq = x * x
    lane = (sq[0::4] + sq[1::4]) + (sq[2::4] + sq[3::4])                 # group g = 2 c + q
    level_q = lane[0::2] + lane[1::2]                                    # q = 0 and 1 of every c
    assert bits(f32_norm.tile_partial(x)) == bits(f32_norm.tree(level_q))
    assert x.dtype == np.float32 and f32_norm.tile_partial(x).dtype == np.float32


def test_launch_sum_is_strided_then_a_tree_and_the_padding_is_exact():
    rng = np.random.default_rng(1)
    for L in (0, 1, 2, 11, 16, 63, 64, 65, 80, 128, 130, 200):
        s = (rng.standard_normal(L).astype(np.float32)) ** 2
        a = np.zeros(64, dtype=np.float32)
        for i, v in enumerate(s):
            a[i % 64] = np.float32(a[i % 64] + v)
        assert bits(f32_norm.launch_sum(s)) == bits(f32_norm.tree(a)), L
        if 0 < L <= 64:
            # padding to the next power of two is all the 64-wide tree does to a short list: x + 0 = x exactly
            p2 = 1 << (L - 1).bit_length()
            short = np.zeros(p2, dtype=np.float32)
            short[:L] = s
            assert bits(f32_norm.launch_sum(s)) == bits(f32_norm.tree(short)), L
    assert bits(f32_norm.launch_sum(np.zeros(0, dtype=np.float32))) == 0   # +0.0f, not -0


def test_the_chain_over_launches_is_left_to_right():
    rng = np.random.default_rng(2)
    blocks = [rng.standard_normal((8, 256)).astype(np.float32) * np.float32(3.0 ** (i % 7)) for i in range(130)]
    got = f32_norm.expect_norm_sq(blocks)
    for b in range(8):
        r = [f32_norm.launch_sum(np.concatenate([f32_norm.tile_partials(v[b]) for v in blocks[k:k + 64]])) for k in (0, 64, 128)]
        assert bits(got[b]) == bits(np.float32(np.float32(r[0] + r[1]) + r[2]))
    assert not np.array_equal(bits(got), bits(f32_norm.expect_norm_sq(blocks[64:] + blocks[:64])))


def test_nonfinite_values_reach_their_rank_only():
    rng = np.random.default_rng(3)
    blocks = [rng.standard_normal((8, 512)).astype(np.float32) for _ in range(3)]
    clean = f32_norm.expect_norm_sq(blocks)
    for planted, check in ((np.nan, np.isnan), (np.inf, np.isposinf), (-np.inf, np.isposinf)):
        dirty = [v.copy() for v in blocks]
        dirty[1][5, 300] = planted
        got = f32_norm.expect_norm_sq(dirty)
        assert check(got[5])
        keep = np.arange(8) != 5
        assert np.array_equal(bits(got[keep]), bits(clean[keep]))


# ------------------------------------------------------------------ the GPU tests' data discriminate
@pytest.mark.parametrize("algo,side,total", cases.SCHEDULES, ids=cases.SCHEDULE_IDS)
def test_unequal_cancel_lists_discriminate(algo, side, total):
    """test_gpu_shards_f32_norm.py's main case: hard_inputs.cancel, (1, 3, 2, 5) tiles per block, and ONE case
    runs all three scales.  The three wrong ADD orders show at every scale.  An fma shows only where a square
    is inexact, and cancel's sums carry few mantissa bits (what survives next to +-B): at scale 1 and 1 / P
    (the same mantissas) most squares are exact, so the fma is pinned per case — some scale of it must show
    it, which 0.1, whose products fill the mantissa, does where the others do not."""
    buckets = cases.bucket_list(algo, side, total, cases.UNEQUAL)
    fma_seen = False
    for scale in cases.SCALES(total):
        values = cases.stored(buckets, scale)
        want = f32_norm.expect_norm_sq(values)
        assert np.isfinite(want).all() and (want > 0).all()
        for name, alt in ALTERNATIVES.items():
            differs = (bits(f32_norm.expect_norm_sq(values, **alt)) != bits(want)).any()
            if "fma" in name:
                fma_seen = fma_seen or differs
            else:
                assert differs, f"scale {scale}: {name} gives the same norm_sq in every rank"
    assert fma_seen, "no scale of this case tells an fma chain from separate multiplies and adds"


@pytest.mark.parametrize("algo,side,total", cases.SCHEDULES, ids=cases.SCHEDULE_IDS)
def test_accumulated_lists_follow_the_stored_value(algo, side, total):
    """accumulate once and twice: the norm is that of old + v, not of v, and the data tell them apart.  These
    lists claim nothing about the order: old spans 2^-27 .. 2^24, and a few large squares hide every low bit."""
    first = cases.bucket_list(algo, side, total, cases.UNEQUAL, seed=1)
    second = cases.bucket_list(algo, side, total, cases.UNEQUAL, seed=2)
    rng = np.random.default_rng(total)
    old = [cases.random_floats(rng, s.shape) for _, s in first]
    scale = 1.0 / total
    once = cases.stored(first, scale, old)
    twice = cases.stored(second, scale, once)
    alone = f32_norm.expect_norm_sq(cases.stored(first, scale))
    assert (bits(alone) != bits(f32_norm.expect_norm_sq(once))).all(), "the norm of v alone equals the norm of old + v"
    assert (bits(f32_norm.expect_norm_sq(once)) != bits(f32_norm.expect_norm_sq(twice))).any()


def test_the_strided_list_discriminates():
    """80 partials per rank: lanes 0 .. 15 add two.  It claims the order in which the PARTIALS are combined — one
    ulp of one of 80 partials rarely reaches their sum, so the tile's own order is the unequal lists' to pin."""
    total, tiles = cases.STRIDED
    buckets = cases.bucket_list(cases.t.SWING, 4, total, tiles, seed=5)
    values = cases.stored(buckets, 0.1)
    assert_discriminates(values, "sixteen buckets of 5 tiles per block", COMBINE)
    # ... and the strided rule is not a plain tree over the 80 partials padded to 128
    want = f32_norm.expect_norm_sq(values)

    def padded_tree(partials):
        p = np.zeros(128, dtype=np.float32)
        p[:partials.size] = partials
        return f32_norm.tree(p)
    assert (bits(f32_norm.expect_norm_sq(values, combine=padded_tree)) != bits(want)).any()


@pytest.mark.parametrize("count", cases.CHAIN_COUNTS)
def test_the_multi_launch_lists_discriminate(count):
    buckets = cases.bucket_list(cases.t.SWING, 4, 8, (1,) * count, seed=6)
    values = cases.stored(buckets, 0.1)
    assert_discriminates(values, f"{count} buckets", COMBINE)   # as the strided list: the combination, and the chain
    if count > 64:
        # one launch over the whole list (no chain) is another number
        want = f32_norm.expect_norm_sq(values)
        whole = np.array([f32_norm.launch_sum(f32_norm.rank_partials(values, b)) for b in range(8)], dtype=np.float32)
        assert (bits(whole) != bits(want)).any()


def test_same_f32_is_what_the_gpu_file_compares_with():
    assert f32_tree.same_f32(np.float32([np.nan, 1.0]), np.float32([-np.nan, 1.0]))
    assert not f32_tree.same_f32(np.float32([np.inf]), np.float32([np.nan]))
