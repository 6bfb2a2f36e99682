"""The numpy expectation of allred_plan_all_gather_shards_mxfp4 (helper, no tests), written from the
semantics include/allred.h states.  The amax, the special blocks, 2^-X and the ONE float32 multiply are
tests/mxfp8_ref.py's; new here are the scale exponent (emax of e2m1 is 2, RCEIL turns at mantissa
0x400000), the saturating round-to-nearest-even onto the eight e2m1 magnitudes, and the nibble packing."""
import numpy as np

from mxfp8_ref import block_amax_bits, is_special, pow2, scaled  # noqa: F401  (re-exported for the tests)

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
NAN_SCALE = 0xFF


def scale_exponent(A, rceil):
    """X of a finite block, clamped below at -127 (int32); meaningless where is_special(A)"""
    X = (A >> 23).astype(np.int32) - 127 - 2
    if rceil:
        X = X + ((A & np.uint32(0x7FFFFF)) > np.uint32(0x400000)).astype(np.int32)
    return np.maximum(X, -127)


def e2m1_nibbles(y):
    """y float32 -> uint8 codes 0 .. 15: the nearest of E2M1 to |y| (|y| > 6: 6), a tie to the even code, bit 3 the
    sign bit of y, kept on a zero result.  The midpoints are exact in float64, so the compares are."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    sign = ((y.view(np.uint32) >> 31) << 3).astype(np.uint8)
    mag = np.abs(y.astype(np.float64))
    mid = (E2M1[:-1] + E2M1[1:]) / 2                       # between codes k and k + 1: goes up when above, or on it with k odd
    up = (mag[..., None] > mid) | ((mag[..., None] == mid) & (np.arange(7) % 2 == 1))
    return up.sum(axis=-1).astype(np.uint8) | sign


def pack(nibbles):
    """(..., 2 k) codes -> (..., k) bytes: element 2 i in bits 3:0 of byte i, element 2 i + 1 in bits 7:4"""
    n = np.asarray(nibbles, dtype=np.uint8)
    return n[..., 0::2] | (n[..., 1::2] << 4)


def quantize(x, rceil=False):
    """the call's rule: x (..., 32 k) float32 -> (element bytes (..., 16 k) uint8, scale bytes (..., k) uint8)"""
    A = block_amax_bits(x)
    X, special = scale_exponent(A, rceil), is_special(A)
    nib = np.where(np.repeat(special, 32, axis=-1), np.uint8(0), e2m1_nibbles(scaled(x, X)))
    return pack(nib), np.where(special, NAN_SCALE, X + 127).astype(np.uint8)


def dequantize64(elems, scales):
    """float64, exact: e2m1(nibble) * 2^(scale - 127); NaN under a 0xFF scale"""
    e, s = np.asarray(elems, dtype=np.uint8), np.asarray(scales, dtype=np.uint8)
    nib = np.stack([e & 0xF, e >> 4], axis=-1).reshape(e.shape[:-1] + (-1,))
    val = np.where(nib & 8, -E2M1[nib & 7], E2M1[nib & 7])
    return val * np.repeat(np.where(s == NAN_SCALE, np.nan, np.exp2(s.astype(np.float64) - 127.0)), 32, axis=-1)


def expected_rows(blocks, rceil=False):
    """blocks: (total, blk) float32, a bucket's shard blocks -> (the element row (n / 2,), the scale row (n / 32,)):
    what EVERY rank's rows receive"""
    e, s = quantize(np.ascontiguousarray(blocks, dtype=np.float32), rceil)
    return e.reshape(-1), s.reshape(-1)
