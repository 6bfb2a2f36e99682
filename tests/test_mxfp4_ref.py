"""tests/mxfp4_ref.py on the CPU: known nibbles, scale bytes and the packing order, written out, so that the GPU tests
compare against a reference that is itself pinned to include/allred.h's rule."""
import numpy as np
import pytest

import mx4_cases as mc
import mxfp4_ref as ref

rng = np.random.default_rng(0)
X = np.stack([mc.block(i, rng) for i in range(mc.NBLOCKS)]).view(np.float32)


@pytest.mark.parametrize("y,nibble", [(0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6), (5.0 + 2.0 ** -21, 7),
                                      (-0.25, 8), (0.25 + 2.0 ** -25, 1), (0.5, 1), (6.0, 7), (7.9, 7), (-1e30, 0xF), (-0.0, 8),
                                      (-(2.0 ** -140), 8), (np.inf, 7)])
def test_known_nibbles(y, nibble):
    assert ref.e2m1_nibbles(np.float32([y]))[0] == nibble


def test_the_tie_block_and_the_packing_order():
    (e, s), (e2, s2) = ref.quantize(X[mc.TIES], rceil=False), ref.quantize(X[mc.TIES], rceil=True)
    assert s[0] == s2[0] == 127 and np.array_equal(e, e2)
    assert [(e[p // 2] >> (4 * (p % 2))) & 0xF for p in range(1, 18)] == mc.TIE_NIBBLES   # element 2 i: bits 3:0 of byte i
    assert list(e[1:9]) == mc.TIE_BYTES
    assert list(ref.pack(np.uint8([1, 2, 3, 0xF]))) == [0x21, 0xF3]
    assert list(ref.dequantize64(np.uint8([0x21, 0xF3] * 8), np.uint8([128]))[:4]) == [1.0, 2.0, 3.0, -12.0]


@pytest.mark.parametrize("rceil", [False, True])
def test_scale_bytes_and_special_blocks(rceil):
    e, s = ref.quantize(X, rceil)
    assert list(s[:13, 0]) == mc.SCALES[rceil]
    assert (e[9:12] == 0).all() and set(e[8]) <= {0x00, 0x08, 0x80, 0x88} and 0x08 in e[8]   # NaN scale over zero bytes; -0 kept
    assert np.isnan(ref.dequantize64(e[9:12], s[9:12])).all()
    finite = np.delete(np.arange(mc.NBLOCKS), [9, 10, 11])
    top = np.abs(ref.scaled(X[finite], ref.scale_exponent(ref.block_amax_bits(X[finite]), rceil)).astype(np.float64)).max(axis=-1)
    assert (top <= 6.0).all() if rceil else (top > 6.0).any()                   # RCEIL: nothing saturates
    assert (top[s[finite, 0] > 0] > (3.0 if rceil else 4.0) - 1e-9).all()       # and no scale is larger than needed
