"""The numpy expectation of allred_plan_all_gather_shards_mxfp8_2d and its hard data (helper, no tests).

A bucket is one row-major matrix W[nrows][cols], nrows = total * R, in `total` shard blocks of R rows.
Row-wise the call writes mxfp8_ref.expected_rows of the blocks; column-wise it writes the linear MX rows of
W^T: mxfp8_ref.quantize(W.T), flattened — the same rule, the 32 elements taken down a column.

hard_t is the matrix whose TRANSPOSE, flattened, is mx_cases.shard(1, n, seed): all 24 planted blocks lie
along columns, where only the column-wise reduction meets them whole.  hard_rows is mx_cases.shard itself,
reshaped: the planted blocks lie along rows."""
import numpy as np

import mx_cases
import mxfp8_ref as ref

SHAPES = ((8, 32, 32), (8, 96, 64), (64, 32, 32), (16, 160, 32))   # (P, cols, R) the data conditions are held at


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


def planted_kind(nrows, cols):
    """(cols, nrows / 32) int: the index into mx_cases.BLOCKS of every column block of hard_t"""
    return (np.arange(cols * (nrows // 32)) % mx_cases.NBLOCKS).reshape(cols, nrows // 32)
