"""t.hadamard32 — allred.h's rotation on the host — against the float64 product with the explicit +-1 matrix, and
against tests/mxfp4_rht_ref.py's index-by-index form bit for bit (the GPU tests' expectation).
The bound: output k is 2^-2.5 sum_i +-x_i through five float32 additions and one multiply, each with relative error
2^-24, plus the rounding of the constant: seven factors (1 + 2^-24), so within 7 * 2^-24 * 2^-2.5 * sum |x_i|."""
import numpy as np
import pytest

import f32_tree
import mxfp4_rht_ref as ref
import tenstorrentallreduce_amd as t

MASKS = [0, 0xFFFFFFFF, 0x9E3779B9]
POP = np.array([[bin(i & k).count("1") for i in range(32)] for k in range(32)])
H = np.where(POP & 1, -1.0, 1.0)   # H[k, i] = (-1)^popcount(i & k)
U = 7 * 2.0 ** -24 * 2.0 ** -2.5


@pytest.mark.parametrize("mask", MASKS)
def test_forward_and_inverse_against_the_float64_matrix(mask):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((4096, 32)) * np.exp2(rng.integers(-20, 20, (4096, 1)))).astype(np.float32)
    x64 = x.astype(np.float64)
    s = np.where(mask >> np.arange(32) & 1, -1.0, 1.0)
    bound = U * np.abs(x64).sum(axis=1, keepdims=True)
    y = t.hadamard32(x, mask)
    assert y.dtype == np.float32 and y.shape == x.shape
    worst = (np.abs(y - 2.0 ** -2.5 * (x64 * s) @ H.T) / bound).max()
    print(f"mask {mask:#x}: forward error {worst:.3f} of the bound")
    assert worst <= 1.0
    assert f32_tree.same_f32(y, ref.rotate(x, mask))
    # the same bound applied twice: to the inverse's own seven roundings on ITS input y, and to the forward error of
    # y, which the inverse carries to an output as 2^-2.5 times a signed sum over the 32 values of the block
    back = t.hadamard32(y, mask, inverse=True)
    bound2 = U * np.abs(y.astype(np.float64)).sum(axis=1, keepdims=True) + 2.0 ** -2.5 * 32 * bound
    worst = (np.abs(back - x64) / bound2).max()
    print(f"mask {mask:#x}: round-trip error {worst:.3f} of the bound applied twice")
    assert worst <= 1.0


def test_shapes_and_special_values():
    with pytest.raises(ValueError):
        t.hadamard32(np.zeros(48, dtype=np.float32), 0)
    x = np.ones((2, 3, 64), dtype=np.float32)
    x[0, 0, 0], x[0, 0, 1], x[1, 2, 33], x[0, 1, 5] = np.float32(3.4028235e38), np.float32(1e38), np.nan, -0.0
    y = t.hadamard32(x, 1)
    assert y.shape == x.shape and f32_tree.same_f32(y, ref.rotate(x, 1))
    assert np.isinf(y[0, 0, :32]).any() and np.isnan(y[1, 2, 32:]).all() and not np.isnan(y[1, 2, :32]).any()
