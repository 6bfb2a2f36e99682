"""The MXFP8 rows, consumed by the instruction they are written for: v_mfma_scale_f32_16x16x128_f8f6f4 with
e4m3 on both sides, through tests/mx_consumer.hip (tenstorrentallreduce_amd/build/libmx_consumer.so, test
infrastructure).  Every other MXFP8 test compares bytes with tests/mxfp8_ref.py, a restatement of the
semantics of include/allred.h; here the MI355X itself says what a byte pair means.

1. CONTROLS.  The helper against integer arithmetic with nothing of the project in it: small asymmetric
   integers, uniform and per-(row, 32-group) scales.  They establish the helper's lane map; if they fail
   the helper is wrong and nothing below means anything.
2. THE DECODE TABLE.  Every element byte under eight scale bytes, isolated by a one-hot B, against
   mxfp8_ref.e4m3_value(byte) * 2^(scale - 127); the NaN encodings in runs of their own.
3. THE ROWS AS WRITTEN.  Rank rows and scale rows of allred_plan_all_gather_shards_mxfp8 on mx_cases' planted
   blocks, read in place at their strides, against t.mxfp8_dequantize of the CPU expectation.
4. ONE DENSE CASE.  Four differently scaled groups accumulated in one instruction, against float64.

THE COMPARISON RULE (same_value): values compare as values (+0 == -0: the sum of the other 127 products
decides a zero's sign) and must be EQUAL wherever the expected magnitude is 0 or a normal fp32.  Where it
is a non-zero fp32 denormal the MFMA may return it or 0; where it overflows fp32 the MFMA must return
+-Inf.  What the hardware does there is printed, and written down in DESIGN §17 and include/allred.h.

WHAT THE MI355X SAID.  The lane map is LANE_MAP below (a lane's eight dwords are halves of two MX blocks, not
one block: the first guess failed the varied-scale control); denormal-range values are KEPT, every one;
overflow gives +-Inf of the right sign and leaves the zeros of the same row zeros; the dense case's error
figure is 9.527e-06 = 2^-16.68 of sum |a_k b_k|.  include/allred.h's semantics stood as written."""
import ctypes
import functools
import os

import numpy as np
import pytest

import mx_cases
import mxfp8_ref as ref
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import test_gpu_shards_mxfp8 as mxt  # noqa: E402  (its MxBucket, Shards and cases)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ONE, UNIT = 0x38, 127                      # the e4m3 byte of 1.0, the E8M0 byte of 2^0
TINY = float(np.finfo(np.float32).tiny)    # 2^-126: below it an fp32 is a denormal
SCALES = (0, 1, 8, 119, 127, 135, 246, 254)
LANE_MAP = ("lane l, g = l >> 4: A row l & 15, bytes k0 + 16 g .. + 15 in dwords 0-3 and k0 + 64 + 16 g .. + 15 in dwords 4-7; "
            "B alike by column; scale byte 0 of lane l = the row's MX block g, bytes k0 + 32 g .. + 31; D[4 g + i][l & 15]")


@functools.lru_cache(maxsize=None)
def helper():
    """a missing helper is an error: build() makes it with the package"""
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(t.__file__)), "build", "libmx_consumer.so"))
    lib.mx_consume.restype = ctypes.c_int
    lib.mx_consume.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                               ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib.mx_consume


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)


def consume_at(a_ptr, a_row_stride, sa_ptr, sa_stride, m, k, b, sb):
    """out (m, 16) float32 of A read IN PLACE (device addresses and strides) against B (16, k), sb (16, k / 32) uint8"""
    assert b.shape == (16, k) and sb.shape == (16, k // 32)
    db, dsb = dev8(b), dev8(sb)
    out = torch.full((m, 16), float("nan"), dtype=torch.float32, device=DEV)
    rc = helper()(a_ptr, a_row_stride, sa_ptr, sa_stride, m, k, db.data_ptr(), dsb.data_ptr(), out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"mx_consume returned {rc}"
    torch.cuda.synchronize()
    return out.cpu().numpy()


def consume(a, sa, b, sb):
    """host A (m, k), sa (m, k / 32)"""
    m, k = a.shape
    assert sa.shape == (m, k // 32)
    da, dsa = dev8(a), dev8(sa)
    return consume_at(da.data_ptr(), k, dsa.data_ptr(), k // 32, m, k, b, sb)


def one_hot(k, j):
    """B (16, k) whose column n selects k-index (k / 16) n + j, and its unit scales"""
    b = np.zeros((16, k), dtype=np.uint8)
    b[np.arange(16), (k // 16) * np.arange(16) + j] = ONE
    return b, np.full((16, k // 32), UNIT, dtype=np.uint8)


def every_element(a_ptr, a_row_stride, sa_ptr, sa_stride, m, k):
    """(m, k) float32: what the MFMA makes of every element of A under its scale, k / 16 one-hot launches"""
    got = np.empty((m, k), dtype=np.float32)
    for j in range(k // 16):
        got[:, j::k // 16] = consume_at(a_ptr, a_row_stride, sa_ptr, sa_stride, m, k, *one_hot(k, j))
    return got


def same_value(got, want64, what):
    """THE COMPARISON RULE of the module docstring.  want64: float64, exact.  Returns what the hardware did with
    the denormal-range and the overflowing expectations, for the report."""
    got = np.asarray(got, dtype=np.float32)
    with np.errstate(over="ignore"):
        want = want64.astype(np.float32)          # exact below, +-Inf above the fp32 range
    assert not np.isnan(want64).any()
    mag = np.abs(want64)
    den = (mag > 0) & (mag < TINY)
    plain = ~den
    bad = np.argwhere(plain & ~(got == want))
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}: " \
                          f"{got[tuple(bad[0])]!r}, expected {want[tuple(bad[0])]!r}"
    kept, flushed = den & (got == want), den & (got == 0)
    bad = np.argwhere(den & ~kept & ~flushed)
    assert bad.size == 0, f"{what}: a denormal-range value came out as neither itself nor 0, first at " \
                          f"{tuple(bad[0])}: {got[tuple(bad[0])]!r}, expected {want[tuple(bad[0])]!r}"
    return {"denormal kept": int(kept.sum()), "denormal flushed to 0": int(flushed.sum()),
            "overflow to Inf": int(np.isinf(want).sum())}


def report(what, did):
    print(f"{what}: " + ", ".join(f"{k}: {v}" for k, v in did.items()))


# ------------------------------------------------------------------ 1. controls: the helper against arithmetic
INT_BYTE = {0: 0x00, 1: 0x38, 2: 0x40, 3: 0x44, -1: 0xB8, -2: 0xC0, -3: 0xC4}   # e4m3fn, from the OCP table


def control_operands(k):
    """A, B (16, k) int64, |.| <= 3.  A[m][c] != A[c][m] for every m != c < 16; B not symmetric; no two rows of
    either equal on any 32-group, so a lane, a row or a group taken for another changes the product."""
    m, c = np.meshgrid(np.arange(16), np.arange(k), indexing="ij")
    a = np.where(c < 16, np.where(m < c, 1 + (m + 2 * c) % 3, np.where(m > c, -((2 * m + c) % 4), m % 4)),
                 (3 * m + 5 * c + (m * c) // 5) % 7 - 3)
    b = (5 * m + 2 * c + (m * c) // 3) % 7 - 3
    assert np.abs(a).max() <= 3 and np.abs(b).max() <= 3
    assert all(a[i, j] != a[j, i] for i in range(16) for j in range(16) if i != j)
    assert (b[:, :16] != b[:, :16].T).any()
    for x in (a, b):
        for g in range(k // 32):
            assert len({bytes(r) for r in x[:, 32 * g:32 * g + 32]}) == 16
    return a, b


def as_e4m3(ints):
    return np.vectorize(INT_BYTE.__getitem__, otypes=[np.uint8])(ints)


def scaled_product(a, sa, b, sb):
    """float64: sum over groups of 2^(sa - 127 + sb - 127) times the int64 group product — exact here"""
    k = a.shape[1]
    out = np.zeros((a.shape[0], b.shape[0]))
    for g in range(k // 32):
        dot = a[:, 32 * g:32 * g + 32] @ b[:, 32 * g:32 * g + 32].T           # int64
        out += dot * np.exp2(sa[:, g].astype(np.float64) - 127)[:, None] * np.exp2(sb[:, g].astype(np.float64) - 127)[None, :]
    return out


@pytest.mark.parametrize("scales", ["unit", "varied"])
@pytest.mark.parametrize("k", [128, 256])
def test_control_integer_product(k, scales):
    """Exact integer data: every term and every sum is an fp32.  This is what establishes the lane map (LANE_MAP;
    tests/mx_consumer.hip states it in full).  Under equal scales any map that loads A and B alike gives the
    product; the varied scales tell which 32 bytes a lane's scale byte covers.  The first guess, a lane's 32
    consecutive bytes = one MX block, gave 255 of 256 outputs wrong here."""
    a, b = control_operands(k)
    m, g = np.meshgrid(np.arange(16), np.arange(k // 32), indexing="ij")
    if scales == "unit":
        sa, sb = np.full((16, k // 32), UNIT), np.full((16, k // 32), UNIT)
    else:
        sa, sb = 124 + (m + 3 * g) % 7, 125 + (2 * m + g) % 5
    want = scaled_product(a, sa, b, sb)
    assert np.array_equal(want, want.astype(np.float32).astype(np.float64))
    assert not np.array_equal(want, want.T) and not np.array_equal(want, scaled_product(b, sb, a, sa))
    got = consume(as_e4m3(a), sa.astype(np.uint8), as_e4m3(b), sb.astype(np.uint8))
    bad = np.argwhere(got != want.astype(np.float32))
    assert bad.size == 0, f"the helper's lane map does not hold: {len(bad)} of 256 outputs differ, first at " \
                          f"{tuple(bad[0])}: {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}"
    print(f"control k={k}, {scales} scales: 256 outputs equal the integer product; lane map: {LANE_MAP}")


def test_control_two_waves_and_strides():
    """m = 32 at a row stride and a scale stride wider than the payload: the second wave and the strides"""
    k = 128
    a, b = control_operands(k)
    a = np.concatenate([a, -a[::-1]])
    m, g = np.meshgrid(np.arange(32), np.arange(4), indexing="ij")
    sa = 124 + (m + 3 * g) % 7
    sb = (125 + (2 * m + g) % 5)[:16]
    wide, swide = np.full((32, k + 48), 0x7F, dtype=np.uint8), np.full((32, 4 + 4), 0xFF, dtype=np.uint8)   # NaN fill
    wide[:, :k], swide[:, :4] = as_e4m3(a), sa
    da, dsa = dev8(wide), dev8(swide)
    got = consume_at(da.data_ptr(), k + 48, dsa.data_ptr(), 8, 32, k, as_e4m3(b), sb.astype(np.uint8))
    assert np.array_equal(got, scaled_product(a, sa, b, sb).astype(np.float32))


# ------------------------------------------------------------------ 2. the decode table
def decode_operands():
    """A (16, 128), sa (16, 4): (row, group) slot q = 4 row + group holds the 32 element bytes 32 (q / 8) .. + 31,
    the two NaN encodings replaced by 0x00, under scale byte SCALES[q % 8]: every pair once, and the four
    groups of a row under four different scales"""
    q = np.arange(64)
    a = (32 * (q // 8))[:, None] + np.arange(32)[None, :]
    a = np.where((a & 0x7F) == 0x7F, 0, a).astype(np.uint8)
    sa = np.asarray(SCALES, dtype=np.uint8)[q % 8]
    return a.reshape(16, 128), sa.reshape(16, 4)


def test_decode_table_every_element_byte_under_eight_scale_bytes():
    """the hardware's e4m3(byte) * 2^(scale - 127) against mxfp8_ref's, 254 x 8 pairs: the E8M0 bias, scale
    bytes 0 and 254, e4m3 subnormals, the sign bit, and a scale byte over exactly its 32 elements (the four
    groups of a row lie under four different scales, so a scale taken from a neighbouring group shows)"""
    a, sa = decode_operands()
    assert {int(x) for x in a.reshape(-1)} == set(range(256)) - {0x7F, 0xFF}
    da, dsa = dev8(a), dev8(sa)
    got = every_element(da.data_ptr(), 128, dsa.data_ptr(), 4, 16, 128)
    want = ref.e4m3_value(a) * np.exp2(sa.astype(np.float64) - 127.0).repeat(32, axis=-1)
    did = same_value(got, want, "decode table")
    assert did["denormal kept"] + did["denormal flushed to 0"] > 0 and did["overflow to Inf"] > 0
    report("decode table (254 element bytes x scale bytes 0, 1, 8, 119, 127, 135, 246, 254)", did)


def test_decode_nan_encodings_poison_their_row_only():
    """element bytes 0x7F and 0xFF, each alone in its row, and a 0xFF scale over an all-zero group: that row's
    sixteen outputs are NaN — the found-inf signal on the consumer's side — and every other row is exact"""
    k = 128
    a, b = control_operands(k)
    ea, sa = as_e4m3(a), np.full((16, 4), UNIT, dtype=np.uint8)
    ea[3, 77], ea[9, 5] = 0x7F, 0xFF
    ea[12, 64:96], sa[12, 2] = 0, 0xFF
    a[12, 64:96] = 0
    got = consume(ea, sa, as_e4m3(b), np.full((16, 4), UNIT, dtype=np.uint8))
    nan_rows = np.zeros(16, dtype=bool)
    nan_rows[[3, 9, 12]] = True
    assert np.isnan(got[nan_rows]).all(), "a NaN encoding did not make its whole row NaN"
    assert np.array_equal(got[~nan_rows], (a @ b.T)[~nan_rows].astype(np.float32))


# ------------------------------------------------------------------ 3. the rows as written
NAN_BLOCKS = [i for i, (_, amax, _, planted) in enumerate(mx_cases.BLOCKS)
              if any((bits & 0x7FFFFFFF) >= 0x7F800000 for bits in [amax, *planted.values()])]


@pytest.mark.parametrize("rceil", [False, True], ids=["floor", "rceil"])
def test_rows_as_written_feed_the_mfma(rceil):
    """8 ranks (Swing 4x4), two buckets in the flat layout: blk = 256 (a rank row is a 16 x 128 matrix, one
    k-step) and blk = 512 with stride skew (16 x 256, two k-steps, scale bytes 4..7 of a matrix row in use).
    Rank 0's and the last rank's rows go to the MFMA where the call wrote them: a_row_stride = k and
    a_scale_stride = k / 32 inside the rank row."""
    algo, side, total = t.SWING, 4, 8
    buckets = [mxt.MxBucket(total, 256 * total), mxt.MxBucket(total, 512 * total, skew=True)]
    keys = [(total, 256, 21), (total, 512, 22)]
    shards = mxt.Shards(buckets, "flat")
    shards.fill([mxt.cases(*key) for key in keys])
    plan = mxt.any_plan(algo, side, total)
    with t.launch_trace() as tr:
        plan.all_gather_shards_mxfp8(shards.args(), rceil=rceil, stream=mxt.stream())
    assert tr.kernels == [f"k_ag_group_mxfp8<{total}, {'true' if rceil else 'false'}>"]
    mxt.check_all(buckets, keys, rceil, "the rows the MFMA is about to read")
    seen = {"all-NaN rows": 0, "exact rows": 0, "denormal-range elements": 0, "overflowing elements": 0}
    for bk, key in zip(buckets, keys):
        k = bk.blk // 2
        we, ws = mxt.expected(*key, rceil)
        want = ref.dequantize64(we, ws).reshape(16, k)
        with np.errstate(over="ignore"):
            assert np.array_equal(t.mxfp8_dequantize(we, ws).reshape(16, k), want.astype(np.float32), equal_nan=True)
        nan_rows = np.isnan(want).any(axis=1)
        planted = np.isin(np.arange(bk.n // 32) % mx_cases.NBLOCKS, NAN_BLOCKS).reshape(16, k // 32).any(axis=1)
        assert np.array_equal(nan_rows, planted), "NaN rows are exactly those with a planted NaN / Inf block"
        for r in (0, total - 1):
            got = every_element(bk.buf[0].data_ptr() + r * bk.row_stride, k, bk.buf[1].data_ptr() + r * bk.scale_stride, k // 32,
                                16, k)
            assert np.isnan(got[nan_rows]).all() and not np.isnan(got[~nan_rows]).any(), \
                f"NaN rows {np.flatnonzero(np.isnan(got).all(axis=1)).tolist()}, expected {np.flatnonzero(nan_rows).tolist()}"
            did = same_value(got[~nan_rows], want[~nan_rows], f"n={bk.n}, rank {r}'s row")
            report(f"rows as written, rceil={rceil}, blk={bk.blk}, rank {r}", did)
            w = np.abs(want[~nan_rows])
            seen["all-NaN rows"] += int(nan_rows.sum())
            seen["exact rows"] += int((~nan_rows).sum())
            seen["denormal-range elements"] += int(((w > 0) & (w < TINY)).sum())
            seen["overflowing elements"] += did["overflow to Inf"]
    plan.close()
    assert seen["all-NaN rows"] and seen["exact rows"] and seen["denormal-range elements"], seen
    assert bool(seen["overflowing elements"]) == rceil, seen    # 256 x 2^120, under RCEIL only


# ------------------------------------------------------------------ 4. one dense case
DENSE_MEASURED = 9.527e-06          # = 2^-16.68, on an MI355X; see the test's docstring


def test_dense_accumulation_across_four_scales():
    """Gaussian data of mixed block magnitude (2^-20 .. 2^11 per 32-block) quantised by the CPU reference, a
    16 x 128 A; B integers |b| <= 3 at unit scale; out against the float64 product of the dequantised operands.
    The error figure is max |out - ref| / sum_k |a_k b_k|.
    MEASURED on an MI355X: 9.527e-06 = 2^-16.68.  That is ABOVE K 2^-24 = 2^-17, the bound of 128 fp32 adds of
    the (exact) products in any order: the matrix core does not add them as fp32 adds would (how it aligns
    them was not established; the four groups of a row differ by up to 2^31 in scale here), so a consumer
    has 16 to 17 bits of sum |a_k b_k| from one instruction, not 24.  The assertion is FOUR TIMES the measured
    figure: the data is seeded, so the margin covers a change of data, not of hardware."""
    algo, side, total = t.SWING, 4, 8
    rng = np.random.default_rng(128)
    x = (rng.standard_normal((total, 256)) * np.exp2(rng.integers(-20, 12, (total, 8)).repeat(32, axis=1))).astype(np.float32)
    e, s = ref.expected_rows(x)
    a, sa = e.reshape(16, 128), s.reshape(16, 4)
    b = rng.integers(-3, 4, (16, 128))
    sb = np.full((16, 4), UNIT, dtype=np.uint8)
    got = consume(a, sa, as_e4m3(b), sb)
    a64 = ref.dequantize64(a, sa)
    want, mass = a64 @ b.T.astype(np.float64), np.abs(a64) @ np.abs(b.T).astype(np.float64)
    assert len({int(v) for v in sa.reshape(-1)}) > 8 and (mass > 0).all()
    figure = float((np.abs(got.astype(np.float64) - want) / mass).max())
    print(f"dense case: max |out - ref| / sum |a_k b_k| = {figure:.3e} = 2^{np.log2(figure) if figure else -np.inf:.2f} "
          f"(a chain of 128 fp32 adds: at most 2^-17; asserted: 4 x {DENSE_MEASURED:.3e})")
    assert figure <= 4 * DENSE_MEASURED
    # the same case with the kernel's rows in place of the reference's: the bytes are equal, so is out
    bk = mxt.MxBucket(total, 256 * total)
    shards = mxt.Shards([bk], "flat")
    shards.fill([x])
    plan = mxt.any_plan(algo, side, total)
    plan.all_gather_shards_mxfp8(shards.args(), rceil=False, stream=mxt.stream())
    bk.check(bk.after(e, s), "dense case")
    for r in (0, total - 1):
        again = consume_at(bk.buf[0].data_ptr() + r * bk.row_stride, 128, bk.buf[1].data_ptr() + r * bk.scale_stride, 4,
                           16, 128, as_e4m3(b), sb)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    plan.close()
