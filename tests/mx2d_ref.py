"""The numpy expectation of allred_plan_all_gather_shards_mxfp8_2d and its hard data (helper, no tests).

A bucket is one row-major matrix W[nrows][cols], nrows = total * R, in `total` shard blocks of R rows.
Row-wise the call writes mxfp8_ref.expected_rows of the blocks; column-wise it writes the linear MX rows of
W^T: mxfp8_ref.quantize(W.T), flattened — the same rule, the 32 elements taken down a column.

hard_t is the matrix whose TRANSPOSE, flattened, is mx_cases.shard(1, n, seed): all 24 planted blocks lie
along columns, where only the column-wise reduction meets them whole.  hard_rows is mx_cases.shard itself,
reshaped: the planted blocks lie along rows."""
import numpy as np

import mx2d_cases
import mx_cases
import mxfp8_ref as ref

# (P, cols, R) the data conditions are held at: four of one row group per block, then the shapes of several
SHAPES = ((8, 32, 32), (8, 96, 64), (64, 32, 32), (16, 160, 32),
          (8, 32, 96), (32, 96, 96), (16, 96, 128), (8, 128, 96), (8, 192, 128), (64, 96, 96), (64, 64, 128))


def hard_t(total, cols, R, seed):
    """(nrows, cols) float32, nrows = total * R"""
    nrows = total * R
    wt = mx_cases.shard(1, nrows * cols, seed).reshape(cols, nrows)
    return np.ascontiguousarray(wt.T)


def hard_rows(total, cols, R, seed):
    """(nrows, cols) float32: mx_cases.shard(total, R * cols, seed) as the matrix its blocks form"""
    return np.ascontiguousarray(mx_cases.shard(total, R * cols, seed).reshape(total * R, cols))


def blocks(W, total):
    """(total, blk) float32: the matrix as the shard blocks of the call"""
    return np.ascontiguousarray(W).reshape(total, -1)


def expected_t(W, rceil=False):
    """(the t element row (n,), the t scale row (n / 32,)): what EVERY rank's t rows receive"""
    e, s = ref.quantize(np.ascontiguousarray(np.asarray(W, dtype=np.float32).T), rceil)
    return e.reshape(-1), s.reshape(-1)


def expected_rows(W, total, rceil=False):
    return ref.expected_rows(blocks(W, total), rceil)


MUTANTS = ("src_ignores_row_group", "out_ignores_row_group", "row_group_shift_lgw", "row_and_column_group_swapped")
WALK_FILL = 0xA5   # what walk leaves in a byte that no unit writes


def walk(W, total, rceil, lg_side, mutant=None):
    """k_ag_group_mxfp8_2d's PLACEMENT, emulated: every unit (block, rem) of the bucket W in the order the kernel's
    cursor takes them, the five offsets from a restatement of csrc/mx2d_span.hpp's mx2d_unit_at, the patch read
    from the shard blocks at `src`, its row blocks and its column blocks quantised with mxfp8_ref, the bytes
    written at `row`, `rscale`, `t` and `tscale` the way the kernel's store loops address them.  Returns
    (rows, scales, t rows, t scales) of one rank, WALK_FILL where nothing was written.

    mutant: one deliberate mistake in the restated offsets (MUTANTS).  The first three are mistakes in the
    row-group terms; the last, row group and column group taken for each other behind the split, is a control
    that needs no second row group to show.  A mutant's address outside its buffer reads zeros or writes
    nothing."""
    assert mutant is None or mutant in MUTANTS
    W = np.ascontiguousarray(W, dtype=np.float32)
    nrows, cols = W.shape
    R = nrows // total
    lgh, lgw, rgs, cgs = mx2d_cases.shape_class(cols, R, lg_side)
    H, Wd = 32 << lgh, 32 << lgw
    shard_stride = R * cols
    shard = blocks(W, total).reshape(-1)
    block, rem = (a.reshape(-1) for a in np.meshgrid(np.arange(total, dtype=np.int64), np.arange(rgs * cgs, dtype=np.int64), indexing="ij"))
    # mx2d_unit_at
    rg, cg = rem // cgs, rem % cgs
    if mutant == "row_and_column_group_swapped":
        rg, cg = cg, rg
    shift = 5 + (lgw if mutant == "row_group_shift_lgw" else lgh)
    in_block = 0 if mutant == "src_ignores_row_group" else (rg << shift) * cols
    j0 = cg << (5 + lgw)
    i0 = block * R + (0 if mutant == "out_ignores_row_group" else rg << shift)
    src = block * shard_stride + in_block + j0
    row = i0 * cols + j0
    rscale = row >> 5
    t = j0 * nrows + i0
    tscale = t >> 5
    # the patches: (units, H, Wd)
    i, j = np.arange(H, dtype=np.int64)[None, :, None], np.arange(Wd, dtype=np.int64)[None, None, :]
    at = src[:, None, None] + i * cols + j
    inside = at < shard.size
    patch = np.where(inside, shard[np.where(inside, at, 0)], np.float32(0))
    re, rs = ref.quantize(patch, rceil)                                            # (units, H, Wd), (units, H, Wd / 32)
    te, ts = ref.quantize(np.ascontiguousarray(patch.transpose(0, 2, 1)), rceil)   # (units, Wd, H), (units, Wd, H / 32)
    n = nrows * cols

    def place(size, where, values):
        out = np.full(size, WALK_FILL, dtype=np.uint8)
        ok = where < size
        out[where[ok]] = values[ok]
        return out

    kw, kh = np.arange(Wd // 32, dtype=np.int64)[None, None, :], np.arange(H // 32, dtype=np.int64)[None, None, :]
    jt, it = np.arange(Wd, dtype=np.int64)[None, :, None], np.arange(H, dtype=np.int64)[None, None, :]
    return (place(n, row[:, None, None] + i * cols + j, re),
            place(n // 32, rscale[:, None, None] + i * (cols // 32) + kw, rs),
            place(n, t[:, None, None] + jt * nrows + it, te),
            place(n // 32, tscale[:, None, None] + jt * (nrows // 32) + kh, ts))


def planted_kind(nrows, cols):
    """(cols, nrows / 32) int: the index into mx_cases.BLOCKS of every column block of hard_t"""
    return (np.arange(cols * (nrows // 32)) % mx_cases.NBLOCKS).reshape(cols, nrows // 32)
