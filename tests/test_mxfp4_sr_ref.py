"""The host statement of allred.h's SR rule (t.philox4x32_10, t.e2m1_sr, t.mxfp4_sr_quantize), without a GPU: Philox's
known answers, and the rounding's EXACT unbiasedness — over all 2^22 values of the random field the number of
round-ups is the dropped fraction's numerator, no tolerance."""
import numpy as np
import pytest

import tenstorrentallreduce_amd as t

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)
ALL_R = np.arange(1 << 22, dtype=np.uint32)
DENORMAL = np.uint32(0x00400000).view(np.float32)
# scaled values over [0, 8): a denormal, 2^-24 (E = 103: T = 0), 2^-23 (E = 104: T = 1), both sides of every step
VALUES = [DENORMAL, 2.0 ** -24, 2.0 ** -23, 0.25, 0.75, 0.99999994, 1.25, 2.5, 5.0, 5.999, 6.5, 7.9999995]


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{w:08x}" for w in t.philox4x32_10(counter, key)) == want


def test_a_grid_value_never_moves():
    for sign in (1.0, -1.0):
        for code, v in enumerate(GRID):
            got = t.e2m1_sr(np.full(ALL_R.shape, sign * v, dtype=np.float32), ALL_R)
            assert (got == (code | (8 if sign < 0 else 0))).all(), (sign, v)


@pytest.mark.parametrize("v", VALUES)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_round_ups_are_exactly_the_dropped_fraction(v, sign):
    v = np.float32(v)
    a = int(v.view(np.uint32))
    down = int(np.searchsorted(GRID, v, side="right")) - 1   # the code toward zero; above 6 that is 7 and nothing is above it
    if v >= 1:
        ups = 0 if down == 7 else a & 0x3FFFFF
    else:
        e = a >> 23
        ups = ((((a & 0x7FFFFF) | 0x800000) >> (127 - e)) if e >= 104 else 0) & 0x3FFFFF
    got = t.e2m1_sr(np.full(ALL_R.shape, sign * v, dtype=np.float32), ALL_R)
    assert ((got >> 3) == (1 if sign < 0 else 0)).all()
    mag = got & 7
    assert int((mag == down + 1).sum()) == ups and int((mag == down).sum()) == (1 << 22) - ups
    assert mag[0] == down   # r = 0 truncates toward zero


def test_quantize_is_the_rule_block_by_block():
    """scale bytes and the NaN block are the MXFP4 call's; the words are those of (e / 4, 0, bucket, step) under the seed"""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(256) * np.exp2(rng.integers(-20, 20, 256))).astype(np.float32)
    x[40] = np.nan
    seed, step, bucket = 0x0123456789ABCDEF, 7, 33
    for rceil in (False, True):
        by, sc = t.mxfp4_sr_quantize(x, seed, step, bucket, rceil=rceil)
        assert sc[1] == 0xFF and not by[16:32].any()
        blk = x[160:192]   # block 5: elements 160 .. 191, Philox counters 40 .. 47
        amax = int((blk.view(np.uint32) & 0x7FFFFFFF).max())
        sb = max((amax >> 23) - 2 + (1 if rceil and amax & 0x7FFFFF > 0x400000 else 0), 0)
        words = np.concatenate([t.philox4x32_10((g, 0, bucket, step), (seed & 0xFFFFFFFF, seed >> 32)) for g in range(40, 48)])
        code = t.e2m1_sr(blk * np.float32(2.0 ** (127 - sb)), words)
        assert sc[5] == sb and np.array_equal(by[80:96], code[0::2] | code[1::2] << 4)
    a, b = t.mxfp4_sr_quantize(x, seed, step + 1, bucket), t.mxfp4_sr_quantize(x, seed, step, bucket)
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[0], b[0])
    rot = t.mxfp4_sr_quantize(x[64:], seed, step, bucket, sign_mask=0x9E3779B9)
    plain = t.mxfp4_sr_quantize(t.hadamard32(x[64:], 0x9E3779B9), seed, step, bucket)
    assert np.array_equal(rot[0], plain[0]) and np.array_equal(rot[1], plain[1])
