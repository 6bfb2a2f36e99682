"""Hard data for the MXFP8 all-gather (helper, no tests): 24 planted MX blocks of 32 floats — three
256-float tiles' worth — tiled over a shard.  Every block has ONE planted amax (its bits, position and
sign chosen), optional planted elements, and seeded filler of magnitude 2^-6 .. 2^-2 of the amax:
never the amax, spread over several e4m3 binades, and at least two binades below it, so a scale taken
from 8 or 16 elements differs from the block's.  tests/test_mxfp8_ref.py asserts what each block tells.

BLOCKS[i] = (name, amax bits (sign included), amax position, {position: bits} of further planted elements)."""
import numpy as np

P2_8 = 0x43800000     # 256.0: E = 8, X = 0 under both rules, so y = x and the planted elements ARE the e4m3 inputs


def f32(v):
    return int(np.float32(v).view(np.uint32))


def neg(bits):
    return bits | 0x80000000


BLOCKS = [
    # tile 0: where the scale rule turns
    ("mantissa 0x600000 exactly", 0x3FE00000, 5, {}),
    ("one ulp above 0x600000", 0x3FE00001, 17, {}),
    ("one ulp below 0x600000, in the last lane of the quad", 0x3FDFFFFF, 31, {}),
    ("amax 448", 0x43E00000, 0, {}),
    ("amax -448 x 2^-20", neg(f32(448.0 * 2.0 ** -20)), 9, {}),
    ("amax denormal", 0x00000123, 12, {}),
    ("amax 2^-126", 0x00800000, 3, {}),
    ("amax the largest finite fp32", 0x7F7FFFFF, 30, {}),
    # tile 1: zeros, non-finite values, e4m3 ties
    ("all zero, -0 among them", 0x80000000, 0, {i: (0x80000000 if i % 3 == 0 else 0) for i in range(32)}),
    ("one +Inf", 0x7F800000, 11, {}),
    ("one NaN", 0x7FC00001, 22, {}),
    ("-Inf next to finite values", 0xFF800000, 7, {6: f32(3.0), 8: f32(-2.5)}),
    ("e4m3 ties, normal range", P2_8, 1,
     {2: f32(1.0625), 3: f32(1.1875), 4: f32(17.0), 5: f32(19.0), 6: f32(232.0), 7: f32(248.0),
      8: f32(-1.0625), 9: f32(-1.1875), 10: f32(-17.0), 11: f32(-19.0), 12: f32(-232.0), 13: f32(-248.0),
      14: f32(1.0625 + 2.0 ** -20), 15: f32(1.0625 - 2.0 ** -20), 16: f32(2.0 ** -6 + 2.0 ** -10), 17: f32(2.0 ** -6 + 3 * 2.0 ** -10)}),
    ("e4m3 ties, subnormal range", P2_8, 30,
     {0: f32(2.0 ** -10), 1: f32(3 * 2.0 ** -10), 2: f32(5 * 2.0 ** -10), 3: f32(7 * 2.0 ** -10), 4: f32(13 * 2.0 ** -10),
      5: f32(15 * 2.0 ** -10), 6: f32(-(2.0 ** -10)), 7: f32(-3 * 2.0 ** -10), 8: f32(-15 * 2.0 ** -10),
      9: f32(2.0 ** -10 + 2.0 ** -30), 10: f32(-(2.0 ** -10) - 2.0 ** -30), 11: f32(3 * 2.0 ** -10 - 2.0 ** -30)}),
    ("elements that round to +-0", P2_8, 16,
     {0: f32(2.0 ** -11), 1: f32(-(2.0 ** -11)), 2: f32(2.0 ** -30), 3: f32(-(2.0 ** -30)), 4: f32(1e-30), 5: f32(-1e-30),
      6: 0x00000001, 7: 0x80000001, 8: 0x80000000, 9: 0x007FFFFF, 10: 0x807FFFFF, 11: f32(-(2.0 ** -10))}),
    ("amax negative, mantissa 0x700000, in the last lane", neg(0x40F00000), 31, {}),
    # tile 2: the ends of the exponent range, and a bf16-rounded amax
    ("amax 448 x 2^100", f32(448.0 * 2.0 ** 100), 2, {}),
    ("amax 448 x 2^-130", 0x02E00000, 20, {}),
    ("mantissa 0x600000 where the clamp binds", 0x00E00000, 13, {}),
    ("amax just below 2: its bf16 rounding reaches the next binade", 0x3FFFFF00, 26, {}),
    ("amax one ulp above 0x600000, negative", neg(0x41E00001), 8, {}),
    ("amax the largest finite fp32, negative", 0xFF7FFFFF, 16, {}),
    ("a NaN and an Inf", 0x7FC00000, 4, {19: 0xFF800000}),
    ("mantissa above 0x600000 at E = 127", 0x7F600001, 27, {}),
]
NBLOCKS = len(BLOCKS)
assert NBLOCKS == 24


def block(i, rng):
    """BLOCKS[i] as 32 uint32 bit patterns, the filler from rng"""
    _, amax, pos, planted = BLOCKS[i]
    a = np.uint32(amax & 0x7FFFFFFF).view(np.float32)
    ref = np.float64(a) if np.isfinite(a) else 1.0           # non-finite blocks: filler around 1
    mag = ref * np.exp2(rng.uniform(-6.0, -2.0, 32))
    sign = rng.integers(0, 2, 32) * 2.0 - 1.0
    with np.errstate(under="ignore"):
        out = (mag * sign).astype(np.float32).view(np.uint32).copy()   # a denormal amax: smaller denormals, zeros
    for p, bits in planted.items():
        out[p] = bits
    out[pos] = amax
    return out


def tile_blocks(seed):
    """(24, 32) uint32: every planted block once"""
    rng = np.random.default_rng(seed)
    return np.stack([block(i, rng) for i in range(NBLOCKS)])


def shard(total, blk, seed):
    """(total, blk) float32, blk % 256 == 0: MX block m of the flattened shard is planted block m % 24 with
    fresh filler, so every planted block meets every position of a tile and block ends of the shard"""
    assert blk % 256 == 0
    nb = total * blk // 32
    rng = np.random.default_rng(seed)
    out = np.stack([block(m % NBLOCKS, rng) for m in range(nb)])
    return out.reshape(total, blk).view(np.float32)
