"""The numpy expectation of allred_plan_all_gather_shards_mxfp8 (helper, no tests), written from the
semantics include/allred.h states: per aligned group of 32 floats the integer amax A of the abs bit
patterns, the E8M0 scale byte from A's exponent (floor rule, or RCEIL), ONE float32 multiply by
2^-X, and a saturating IEEE round-to-nearest-even to e4m3fn.  Everything is a function of bits.

The pieces are separate so that tests/test_mxfp8_ref.py can put a wrong rule in place of a right one:
block_amax_bits -> scale_exponent -> scaled -> e4m3_bytes."""
import numpy as np

E4M3_MAX = 448.0
NAN_BYTE, NAN_SCALE = 0x7F, 0xFF


def block_amax_bits(x, group=32):
    """x: (..., 32 k) float32 -> (..., 32 k / group) uint32: the largest bits & 0x7fffffff of each group, as integers"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return bits.reshape(bits.shape[:-1] + (-1, group)).max(axis=-1)


def is_special(A):
    """a NaN or +-Inf in the block"""
    return A >= np.uint32(0x7F800000)


def scale_exponent(A, rceil):
    """X of a finite block, clamped below at -127 (int32); meaningless where is_special(A)"""
    X = (A >> 23).astype(np.int32) - 127 - 8
    if rceil:
        X = X + ((A & np.uint32(0x7FFFFF)) > np.uint32(0x600000)).astype(np.int32)
    return np.maximum(X, -127)


def pow2(k):
    """2^k as float32 from its bit pattern, k in [-126, 127]"""
    return ((np.asarray(k, dtype=np.int32) + 127).astype(np.uint32) << 23).view(np.float32)


def scaled(x, X):
    """y = x * 2^-X per group of 32: one float32 multiply, denormals kept.  x: (..., 32 k), X: (..., k)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x.reshape(X.shape + (32,)) * pow2(-X)[..., None]).reshape(x.shape)


def e4m3_bytes(y, truncate=False):
    """y float32 -> uint8 e4m3fn: RNE (truncate: toward zero), subnormals multiples of 2^-9, |y| > 448 ->
    +-448, the sign always kept; a NaN gives the NaN byte with its sign."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    sign = ((y.view(np.uint32) >> 31) << 7).astype(np.uint8)
    mag = np.abs(y.astype(np.float64))
    nan = np.isnan(mag)
    mag = np.where(nan, 0.0, np.minimum(mag, E4M3_MAX))          # +Inf saturates like any |y| > 448
    _, ex = np.frexp(mag)                                        # mag = m 2^ex, m in [0.5, 1)
    quantum = np.exp2((np.maximum(ex - 1, -6) - 3).astype(np.float64))   # the spacing at mag: 2^(e - 3), 2^-9 below 2^-6
    steps = mag / quantum                                        # exact: a power-of-two scaling
    q = np.floor(steps) if truncate else np.rint(steps)          # np.rint: half to even
    val = q * quantum                                            # <= 448; may have reached the next binade
    _, ex2 = np.frexp(val)
    e = np.maximum(ex2 - 1, -6)
    normal = val >= 2.0 ** -6
    man = np.where(normal, val / np.exp2(e.astype(np.float64)) * 8 - 8, val * 2.0 ** 9)
    byte = np.where(normal, (e + 7) << 3, 0).astype(np.int64) | man.astype(np.int64)
    byte = np.where(nan, 0x7F, byte)
    return byte.astype(np.uint8) | sign


def e4m3_value(b):
    """uint8 -> float64 (NaN for 0x7F / 0xFF)"""
    b = np.asarray(b, dtype=np.uint8)
    exp, man = ((b >> 3) & 0xF).astype(np.int32), (b & 7).astype(np.float64)
    mag = np.where(exp == 0, man * 2.0 ** -9, (1.0 + man / 8.0) * np.exp2((exp - 7).astype(np.float64)))
    mag = np.where((b & 0x7F) == 0x7F, np.nan, mag)
    return np.where(b & 0x80, -mag, mag)


def quantize_with(x, X, special, truncate=False):
    """x (..., 32 k) float32 with per-block X and special (..., k) -> (element bytes (..., 32 k), scale bytes (..., k))"""
    elems = e4m3_bytes(scaled(x, X), truncate)
    elems = np.where(np.repeat(special, 32, axis=-1), np.uint8(NAN_BYTE), elems)
    scales = np.where(special, NAN_SCALE, X + 127).astype(np.uint8)
    return elems, scales


def quantize(x, rceil=False):
    """the call's rule: x (..., 32 k) float32 -> (element bytes (..., 32 k) uint8, scale bytes (..., k) uint8)"""
    A = block_amax_bits(x)
    return quantize_with(x, scale_exponent(A, rceil), is_special(A))


def dequantize64(elems, scales):
    """float64, exact: e4m3(byte) * 2^(scale - 127); NaN under a 0xFF scale"""
    s = np.asarray(scales, dtype=np.uint8)
    scale = np.where(s == NAN_SCALE, np.nan, np.exp2(s.astype(np.float64) - 127.0))
    return e4m3_value(elems) * np.repeat(scale, 32, axis=-1)


def saturated(x, X, special):
    """per element: |x * 2^-X| > 448 in a finite block"""
    with np.errstate(invalid="ignore"):
        return (np.abs(scaled(x, X).astype(np.float64)) > E4M3_MAX) & ~np.repeat(special, 32, axis=-1)


def expected_rows(blocks, rceil=False):
    """blocks: (total, blk) float32, a bucket's shard blocks -> (the element row (n,), the scale row (n / 32,)):
    what EVERY rank's rows receive"""
    e, s = quantize(np.ascontiguousarray(blocks, dtype=np.float32), rceil)
    return e.reshape(-1), s.reshape(-1)
