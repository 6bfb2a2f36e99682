"""tests/mxfp8_ref.py — the numpy expectation of allred_plan_all_gather_shards_mxfp8 — held to torch's
e4m3 cast, to the format's error bound and to what tests/mx_cases.py plants, on the CPU.

What each mistake must show on mx_cases is stated per test as a share of the 24 planted blocks and
derived from the planted amax values, not read off a run."""
import numpy as np
import pytest

import mx_cases
import mxfp8_ref as ref
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")


def torch_e4m3(y):
    return torch.from_numpy(np.ascontiguousarray(y)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_e4m3_rounding_is_torchs_cast_up_to_448():
    rng = np.random.default_rng(0)
    quarter = (np.arange(-448 * 64, 448 * 64 + 1) / 64.0).astype(np.float32)              # every tie of the upper binades
    small = (np.arange(-4096, 4097) * 2.0 ** -12).astype(np.float32)                       # quarter steps of the subnormals
    bits = (rng.integers(0, 2, 300000, dtype=np.uint32) << 31) | rng.integers(0, 0x43E00001, 300000, dtype=np.uint32)
    ties = np.array([k * 2.0 ** (e - 4) for e in range(-9, 9) for k in range(16, 33)], dtype=np.float32)   # halfway points of every binade
    y = np.concatenate([quarter, small, bits.view(np.float32), ties, -ties, ties * np.float32(1 + 2.0 ** -23),
                        np.array([0.0, -0.0, 448.0, -448.0], dtype=np.float32)])
    y = y[np.abs(y) <= 448.0]
    assert y.size > 300000
    assert np.array_equal(ref.e4m3_bytes(y), torch_e4m3(y))


def test_above_448_it_saturates_where_torch_gives_nan():
    y = np.array([448.0001, 464.0, 465.0, 1e9, 3.4e38, np.inf, -448.0001, -480.0, -1e30, -np.inf], dtype=np.float32)
    assert np.array_equal(ref.e4m3_bytes(y), np.array([0x7E] * 6 + [0xFE] * 4, dtype=np.uint8))
    assert ((torch_e4m3(y[[2, 3, 8]]) & 0x7F) == 0x7F).all()   # torch: the NaN byte above 464
    tiny = np.array([-0.0, -1e-30, -(2.0 ** -10), 2.0 ** -10, -(2.0 ** -10) * 1.001], dtype=np.float32)
    assert np.array_equal(ref.e4m3_bytes(tiny), np.array([0x80, 0x80, 0x80, 0x00, 0x81], dtype=np.uint8))


def gauss(sigma, n=1 << 16, seed=1):
    return (np.random.default_rng(seed).standard_normal(n) * sigma).astype(np.float32)


@pytest.mark.parametrize("data", ["gauss", "cases"])
def test_rceil_never_saturates_and_the_error_bound_holds(data):
    x = gauss(0.02) if data == "gauss" else mx_cases.shard(8, 256 * 3, 3).reshape(-1)
    for rceil in (False, True):
        A = ref.block_amax_bits(x)
        X, special = ref.scale_exponent(A, rceil), ref.is_special(A)
        assert not special.all() and (data == "gauss" or special.any())
        sat = ref.saturated(x, X, special)
        if rceil:
            assert not sat.any(), "under RCEIL no finite element saturates"
        e, s = ref.quantize(x, rceil)
        fin = ~np.repeat(special, 32)
        err = np.abs(ref.dequantize64(e, s)[fin] - x.astype(np.float64)[fin])
        # half the spacing of 32 in the top binade; an element the floor rule saturates lies in (448, 512) 2^X
        # and is off by less than 64 2^X — 2^(X + 4) cannot hold for it, 448 being what the call must give
        bound = np.where(sat, np.repeat(np.exp2(X + 6.0), 32), np.repeat(np.exp2(X + 4.0), 32))
        assert (err[~sat[fin]] <= bound[fin][~sat[fin]]).all(), "|dequantised - x| <= 2^(X + 4)"
        assert (err[sat[fin]] < bound[fin][sat[fin]]).all(), "a saturated element: below 2^(X + 6)"
        # the package's float32 dequantiser is the same function (Inf where 256 x 2^120 is past fp32)
        with np.errstate(over="ignore"):
            want = ref.dequantize64(e, s).astype(np.float32)
        got = t.mxfp8_dequantize(e, s)
        assert np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]) and np.isnan(got[~fin]).all()


def test_the_floor_rule_saturates_some_gaussian_elements():
    x = gauss(0.02, 1 << 18)
    A = ref.block_amax_bits(x)
    share = ref.saturated(x, ref.scale_exponent(A, False), ref.is_special(A)).mean()
    # a block saturates its amax when the mantissa is above 1.75: a quarter of the binade's log range
    assert share >= 0.001, share


# ------------------------------------------------------------------ what the planted blocks tell
CASES = mx_cases.tile_blocks(7).view(np.float32)   # (24, 32)
AMAX = np.array([b[1] & 0x7FFFFFFF for b in mx_cases.BLOCKS], dtype=np.uint32)
FINITE = AMAX < 0x7F800000


def differs(a, b):
    """per planted block: any element byte or the scale byte differs"""
    return (a[0] != b[0]).any(axis=-1) | (a[1] != b[1]).reshape(24)


def test_planted_amax_is_where_it_was_planted():
    assert np.array_equal(ref.block_amax_bits(CASES), AMAX.reshape(24, 1))
    names = [b[0] for b in mx_cases.BLOCKS]
    assert len(set(names)) == 24
    assert FINITE.sum() == 20


def test_floor_and_rceil_are_told_apart():
    """they differ exactly where a finite amax has a mantissa above 0x600000 and the clamp does not bind:
    the blocks planted at 0x600001 (x 2), 0x700000, 0x7FFF00, 0x7FFFFF (x 2) and 0x7F600001 — 7 of 24"""
    want = FINITE & ((AMAX & 0x7FFFFF) > 0x600000) & ((AMAX >> 23) >= 8)
    assert want.sum() == 7
    got = differs(ref.quantize(CASES, False), ref.quantize(CASES, True))
    assert np.array_equal(got, want)
    # the three around 0x600000: exactly at and one below it the two rules agree
    assert not got[0] and got[1] and not got[2]


def test_truncation_is_told_from_rne():
    """every finite non-zero block has 29 or more filler elements with random low bits, about half of which
    round up; the two tie blocks differ by construction.  18 of 24: the 20 finite blocks but the all-zero
    one and the one with a denormal amax, whose every element is +-0 either way."""
    A = ref.block_amax_bits(CASES)
    X, special = ref.scale_exponent(A, False), ref.is_special(A)
    got = differs(ref.quantize_with(CASES, X, special), ref.quantize_with(CASES, X, special, truncate=True))
    assert got[12] and got[13], "the tie blocks"
    assert got.sum() >= 18 and not got[~FINITE].any()


@pytest.mark.parametrize("group", [8, 16])
def test_amax_over_fewer_elements_is_told(group):
    """the filler lies two binades or more below the amax, so every sub-group without the amax gets a smaller
    scale wherever the clamp at -127 does not hide it: every finite block with (A >> 23) >= 9 — 15 of 24.  A
    block with ONE non-finite value differs too: its sub-groups without it come out finite."""
    A = ref.block_amax_bits(CASES, group)            # (24, 32 / group): per sub-group
    x = CASES.reshape(24, 32 // group, group)
    Xs, sp = ref.scale_exponent(A, False), ref.is_special(A)
    y = x * ref.pow2(-Xs)[..., None]
    e = np.where(sp[..., None], np.uint8(0x7F), ref.e4m3_bytes(y)).reshape(24, 32)
    s = np.where(sp, 0xFF, Xs + 127).astype(np.uint8)[:, :1]   # whichever sub-group's scale such a kernel would store
    with np.errstate(invalid="ignore"):
        got = differs((e, s), ref.quantize(CASES, False))
    want = FINITE & ((AMAX >> 23) >= 9)
    assert want.sum() == 15
    assert got[want].all() and got[[9, 10, 11]].all()


def test_a_float_max_that_ignores_nan_is_told():
    """np.fmax drops a NaN: the block with one NaN and no Inf comes out finite — 1 of 24; Inf still shows"""
    amax = np.fmax.reduce(np.abs(CASES), axis=-1)
    A = amax.view(np.uint32).reshape(24, 1)
    got = differs(ref.quantize_with(CASES, ref.scale_exponent(A, False), ref.is_special(A)), ref.quantize(CASES, False))
    want = np.zeros(24, dtype=bool)
    want[10] = True
    assert np.array_equal(got, want)


@pytest.mark.parametrize("rceil,blocks", [(False, {7, 19, 21}), (True, {1, 7, 20, 21, 23})])
def test_a_scale_from_the_bf16_rounded_amax_is_told(rceil, blocks):
    """bf16 rounding carries 0x3FFFFF00 into the next binade and the largest finite fp32 to Inf (3 of 24).
    Under RCEIL the carried 0x3FFFFF00 gives the exponent the ceiling gives anyway, but the mantissas
    0x600001 round down to 0x600000, which is not above it (5 of 24)."""
    up = AMAX.astype(np.uint64) + 0x7FFF + ((AMAX >> 16) & 1)
    A16 = ((up >> 16) << 16).astype(np.uint32).reshape(24, 1)
    got = differs(ref.quantize_with(CASES, ref.scale_exponent(A16, rceil), ref.is_special(A16)), ref.quantize(CASES, rceil))
    assert set(np.flatnonzero(got)) == blocks


def test_known_answers():
    (e, s), (er, sr) = ref.quantize(CASES, False), ref.quantize(CASES, True)
    s, sr = s.reshape(24), sr.reshape(24)
    assert list(s[:8]) == [119, 119, 119, 127, 107, 0, 0, 246] and list(sr[:8]) == [119, 120, 119, 127, 107, 0, 0, 247]
    assert e[3, 0] == 0x7E and e[4, 9] == 0xFE                          # amax 448 x 2^k -> +-448, exactly
    assert e[0, 5] == 0x7E and e[1, 17] == 0x7E and er[1, 17] == 0x76  # 1.75 x 2^8 = 448; above it: saturated, or 224 under RCEIL
    assert (e[5] == 0x00).sum() + (e[5] == 0x80).sum() == 32            # a denormal amax: 291 x 2^-149 x 2^127 is far below 2^-10
    assert e[6, 3] == 0x40                                              # 2^-126 x 2^127 = 2: exponent field 8, mantissa 0
    assert (s[8] == 0) and set(e[8]) == {0x00, 0x80} and e[8, 0] == 0x80 and e[8, 1] == 0x00
    for i in (9, 10, 11, 22):
        assert s[i] == 0xFF and (e[i] == 0x7F).all() and sr[i] == 0xFF and (er[i] == 0x7F).all()
    ties = {2: 0x38, 3: 0x3A, 4: 0x58, 5: 0x5A, 6: 0x76, 7: 0x78, 8: 0xB8, 9: 0xBA, 10: 0xD8, 11: 0xDA, 12: 0xF6, 13: 0xF8,
            14: 0x39, 15: 0x38, 16: 0x08, 17: 0x0A}
    assert s[12] == 127 and {p: int(e[12, p]) for p in ties} == ties
    sub = {0: 0x00, 1: 0x02, 2: 0x02, 3: 0x04, 4: 0x06, 5: 0x08, 6: 0x80, 7: 0x82, 8: 0x88, 9: 0x01, 10: 0x81, 11: 0x01}
    assert {p: int(e[13, p]) for p in sub} == sub
    zero = {0: 0x00, 1: 0x80, 2: 0x00, 3: 0x80, 4: 0x00, 5: 0x80, 6: 0x00, 7: 0x80, 8: 0x80, 9: 0x00, 10: 0x80, 11: 0x80}
    assert {p: int(e[14, p]) for p in zero} == zero
    assert e[15, 31] == 0xFE and er[15, 31] == 0xF7                      # -7.5: saturated under floor, -240 x 2^-5 under RCEIL
    assert s[18] == 0 and sr[18] == 0 and s[23] == 246 and sr[23] == 247
