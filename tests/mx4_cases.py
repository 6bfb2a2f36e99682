"""Hard data for the MXFP4 all-gather (helper, no tests): 17 planted MX blocks in the shape of tests/mx_cases.py's
BLOCKS — (name, amax bits, amax position, {position: bits} of further planted elements), mx_cases' filler two to six
binades below the amax — cycled over a shard.  17 is odd: every block meets every tile position and both lanes of
the kernel's lane pair.  tests/test_mxfp4_ref.py asserts what they tell."""
import numpy as np

from mx_cases import f32, neg

SIX = 0x40C00000      # 6.0: X = 0 under both rules, so y = x and the planted elements ARE the e2m1 inputs
ULP = 2.0 ** -23

BLOCKS = [
    # tile 0: where the scale rule turns, and the amax range
    ("mantissa 0x400000 exactly", 0x3FC00000, 5, {}),
    ("one ulp above 0x400000", 0x3FC00001, 17, {}),
    ("one ulp below 0x400000, in the odd lane of the pair", 0x3FBFFFFF, 31, {}),
    ("amax 6", SIX, 0, {}),
    ("amax -6 x 2^-20", neg(f32(6.0 * 2.0 ** -20)), 9, {}),
    ("amax denormal", 0x00000123, 12, {}),
    ("amax 2^-126", 0x00800000, 3, {}),
    ("amax the largest finite fp32", 0x7F7FFFFF, 30, {}),
    # tile 1: zeros, non-finite values, the top exponent, e2m1 ties
    ("all zero, -0 among them", 0x80000000, 0, {i: (0x80000000 if i % 3 == 0 else 0) for i in range(32)}),
    ("one +Inf", 0x7F800000, 11, {}),
    ("one NaN", 0x7FC00001, 22, {}),
    ("-Inf next to finite values", 0xFF800000, 7, {6: f32(3.0), 8: f32(-2.5)}),
    ("mantissa above 0x400000 at E = 127", 0x7F600001, 27, {}),
    ("e2m1 ties and their neighbours", SIX, 1,
     {2: f32(0.25), 3: f32(-0.25), 4: f32(0.25 + ULP / 4), 5: f32(0.25 - ULP / 8), 6: f32(0.75), 7: f32(1.25), 8: f32(1.75),
      9: f32(2.5), 10: f32(3.5), 11: f32(5.0), 12: f32(5.0 + 4 * ULP), 13: f32(-5.0), 14: f32(2.0 ** -30), 15: f32(-(2.0 ** -30)),
      16: 0x00000001, 17: 0x80000001}),
    ("amax negative, mantissa 0x500000, in the odd lane", neg(0x40D00000), 31, {}),
    ("mantissa above 0x400000 where the clamp binds", 0x00C00001, 13, {}),
    ("amax one ulp above 0x400000, negative", neg(0x41C00001), 8, {}),
]
NBLOCKS, TIES = len(BLOCKS), 13
# the tie block under either rule: elements 1 .. 17 as nibbles (6 -> 7, then the planted ones); bytes 1 .. 8 of the block
TIE_NIBBLES = [7, 0, 8, 1, 0, 2, 2, 4, 4, 6, 6, 7, 0xE, 0, 8, 0, 8]
TIE_BYTES = [0x80, 0x01, 0x22, 0x44, 0x66, 0xE7, 0x80, 0x80]
# the scale bytes of blocks 0 .. 12 without and with ALLRED_MX_SCALE_RCEIL
SCALES = {False: [125, 125, 125, 127, 107, 0, 0, 252, 0, 255, 255, 255, 252], True: [125, 126, 125, 127, 107, 0, 0, 253, 0, 255, 255, 255, 253]}


def block(i, rng):
    """BLOCKS[i] as 32 uint32 bit patterns, the filler from rng (mx_cases.block's rule)"""
    _, amax, pos, planted = BLOCKS[i]
    a = np.uint32(amax & 0x7FFFFFFF).view(np.float32)
    mag = (np.float64(a) if np.isfinite(a) else 1.0) * np.exp2(rng.uniform(-6.0, -2.0, 32))
    with np.errstate(under="ignore"):
        out = (mag * (rng.integers(0, 2, 32) * 2.0 - 1.0)).astype(np.float32).view(np.uint32).copy()
    for p, bits in planted.items():
        out[p] = bits
    out[pos] = amax
    return out


def shard(total, blk, seed):
    """(total, blk) float32, blk % 256 == 0: MX block m of the flattened shard is planted block m % 17 with fresh filler"""
    rng = np.random.default_rng(seed)
    return np.stack([block(m % NBLOCKS, rng) for m in range(total * blk // 32)]).reshape(total, blk).view(np.float32)
