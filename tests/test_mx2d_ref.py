"""What tests/mx2d_ref.py's data tells, on the CPU: the conditions under which a wrong column-wise kernel cannot
pass tests/test_gpu_shards_mxfp8_2d.py.  Held at mx2d_ref.SHAPES: (P, cols, R) = (8, 32, 32), (8, 96, 64), (64, 32, 32),
(16, 160, 32), and the shapes of several row groups per shard block, each at one of its rank counts.

1. hard_t's planted blocks lie down the columns: its transpose, flattened, is mx_cases.shard.
2. A column scale taken from rows 0 .. 15 of a block alone (half a reduction) changes the bytes of blocks of at
   least 10 of the 24 planted kinds.
3. The transposed ROW-WISE bytes in place of the t rows (the scales of other groups of 32) differ in blocks of at
   least 22 kinds.  NOT at R = 96 with P = 8, 32 or 64, where a row of W holds one planted kind only: there the five
   kinds whose scale the clamp fixes cannot differ, and exactly the other 19 must.
4. Under the floor rule fewer than 1 % of the elements saturate; under RCEIL none.
5. A transposed copy with i and j swapped in the address differs from the expectation at every (non-square) shape.
"""
import numpy as np
import pytest

import mx2d_ref
import mx_cases
import mxfp8_ref as ref

shapes = pytest.mark.parametrize("total,cols,R", mx2d_ref.SHAPES, ids=[f"P{p}-{c}x{r}" for p, c, r in mx2d_ref.SHAPES])
SEED = 3
# the planted kinds whose amax lies below 2^-118: under the floor rule X is clamped at -127, as for any block of smaller values
CLAMPED = {i for i, (_, amax, _, _) in enumerate(mx_cases.BLOCKS) if (amax & 0x7FFFFFFF) >> 23 <= 8}


def kinds_differing(a, b, nrows, cols):
    """the planted kinds with a block whose 32 bytes differ between two (cols, nrows) byte matrices"""
    differ = (a != b).reshape(cols, nrows // 32, 32).any(axis=-1)
    return set(mx2d_ref.planted_kind(nrows, cols)[differ].tolist())


@shapes
def test_the_planted_blocks_lie_down_the_columns(total, cols, R):
    W = mx2d_ref.hard_t(total, cols, R, SEED)
    nrows = total * R
    assert W.shape == (nrows, cols) and W.flags.c_contiguous
    assert np.array_equal(W.T.reshape(-1).view(np.uint32), mx_cases.shard(1, nrows * cols, SEED).reshape(-1).view(np.uint32))
    # every planted kind is there, and the row-wise data is mx_cases.shard as the call's blocks
    assert set(mx2d_ref.planted_kind(nrows, cols).reshape(-1).tolist()) == set(range(mx_cases.NBLOCKS))
    V = mx2d_ref.hard_rows(total, cols, R, SEED)
    assert np.array_equal(mx2d_ref.blocks(V, total).view(np.uint32), mx_cases.shard(total, R * cols, SEED).view(np.uint32))
    e, s = mx2d_ref.expected_t(W)
    assert e.shape == (nrows * cols,) and s.shape == (nrows * cols // 32,)
    we, ws = ref.expected_rows(mx_cases.shard(1, nrows * cols, SEED))
    assert np.array_equal(e, we) and np.array_equal(s, ws)


@shapes
def test_half_a_column_reduction_shows(total, cols, R):
    W = mx2d_ref.hard_t(total, cols, R, SEED)
    nrows = total * R
    wt = np.ascontiguousarray(W.T)
    e, _ = ref.quantize(wt)
    bits = wt.view(np.uint32) & np.uint32(0x7FFFFFFF)
    A16 = bits.reshape(cols, nrows // 32, 32)[:, :, :16].max(axis=-1)
    e16, _ = ref.quantize_with(wt, ref.scale_exponent(A16, False), ref.is_special(A16))
    assert len(kinds_differing(e16, e, nrows, cols)) >= 10


@shapes
def test_transposed_row_wise_bytes_are_not_the_t_rows(total, cols, R):
    W = mx2d_ref.hard_t(total, cols, R, SEED)
    nrows = total * R
    e, _ = ref.quantize(np.ascontiguousarray(W.T))
    er, _ = ref.quantize(W)                      # MX blocks along cols
    differ = kinds_differing(np.ascontiguousarray(er.T), e, nrows, cols)
    if (nrows // 32) % mx_cases.NBLOCKS:
        assert len(differ) >= 22
    else:
        # R = 96 at P = 8, 32, 64: a column is a whole number of 24-block cycles, so a ROW of W holds one position
        # of one planted kind in every column, and a row-wise block meets no other kind.  The kinds whose scale
        # the clamp at 2^-127 fixes then quantise alike both ways; every other kind differs.
        assert differ == set(range(mx_cases.NBLOCKS)) - CLAMPED and len(CLAMPED) == 5


@shapes
def test_saturation_under_both_rules(total, cols, R):
    wt = np.ascontiguousarray(mx2d_ref.hard_t(total, cols, R, SEED).T)
    A = ref.block_amax_bits(wt)
    special = ref.is_special(A)
    floor = ref.saturated(wt, ref.scale_exponent(A, False), special)
    print(f"saturating under the floor rule: {floor.mean():.4%}")   # 0.89 % .. 0.91 % at the four shapes
    assert 0 < floor.mean() < 0.01
    assert not ref.saturated(wt, ref.scale_exponent(A, True), special).any()
    # the row-wise data read down its columns (what the t rows of hard_rows hold) saturates nowhere under RCEIL either
    vt = np.ascontiguousarray(mx2d_ref.hard_rows(total, cols, R, SEED).T)
    A = ref.block_amax_bits(vt)
    assert not ref.saturated(vt, ref.scale_exponent(A, True), ref.is_special(A)).any()


@shapes
def test_i_and_j_swapped_in_the_address_shows(total, cols, R):
    W = mx2d_ref.hard_t(total, cols, R, SEED)
    nrows = total * R
    assert nrows != cols
    e, s = mx2d_ref.expected_t(W)
    swapped = np.ascontiguousarray(e.reshape(cols, nrows).T).reshape(-1)   # byte (i, j) at i * cols + j
    assert not np.array_equal(swapped, e)
    swapped_s = np.ascontiguousarray(s.reshape(cols, nrows // 32).T).reshape(-1)
    assert not np.array_equal(swapped_s, s)
