"""The numpy expectation of allred_plan_all_gather_shards_mxfp4_2d, its hard data and its shapes (helper, no tests):
tests/mx2d_ref.py with tests/mxfp4_ref.py's rule and tests/mx4_cases.py's 17 planted blocks."""
import numpy as np

import mx4_cases
import mxfp4_ref as ref

# (P, cols, R): the smallest shapes at which each term of the unit arithmetic is live at S = 4 and at S = 8
SHAPES = ((8, 32, 32), (8, 96, 64), (8, 64, 96), (8, 128, 128), (8, 160, 160), (16, 64, 32), (32, 32, 96), (64, 32, 32), (64, 64, 96))


def hard_t(total, cols, R, seed):
    """(nrows, cols) float32 whose transpose, flattened, is mx4_cases.shard(1, n, seed): the planted blocks lie down the columns"""
    nrows = total * R
    return np.ascontiguousarray(mx4_cases.shard(1, nrows * cols, seed).reshape(cols, nrows).T)


def hard_rows(total, cols, R, seed):
    """(nrows, cols) float32: the planted blocks lie along the rows"""
    return np.ascontiguousarray(mx4_cases.shard(total, R * cols, seed).reshape(total * R, cols))


def expected(W, total, rceil=False):
    """(rows (n / 2,), scales (n / 32,), t rows (n / 2,), t scales (n / 32,)): what EVERY rank receives"""
    W = np.ascontiguousarray(W, dtype=np.float32)
    te, ts = ref.quantize(np.ascontiguousarray(W.T), rceil)
    return ref.expected_rows(W.reshape(total, -1), rceil) + (te.reshape(-1), ts.reshape(-1))
