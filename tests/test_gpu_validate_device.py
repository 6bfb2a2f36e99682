"""k_validate (allred_validate_device) against the host validator
(allred_validate_result_vector, host_data.cpp:49-91 = allred_helper.cpp:18-120).

Per row `bad` must equal what the host function returns (total_nodes = 2 * mult,
ALLRED_BF16_ROUND matching round_mode); first_bad and max_error are checked against
a numpy restatement of the definition in include/allred.h: expected =
bf16((a + b) * mult) with both operations in fp32, diff = |actual - expected| in
fp32, bad = !(diff <= error), first_bad = lowest bad index, max_error = largest
non-NaN diff over the bad elements (the host leaves the first mismatch out of its
maximum; the device does not).

Shapes: the smallest at which the kernel can go wrong — one 16-byte vector, a
ragged last wave (264 = 33 vectors), one tile, 65,544 (8193 vectors: a ragged 129th
tile), and 2048 x 512 + 8 elements, one vector more than one grid pass of the
launcher's 2048 workgroups (the grid-stride path)."""
import functools

import numpy as np
import pytest
import torch

import tenstorrentallreduce_amd as t

pytestmark = pytest.mark.gpu

GRID_PASS = 2048 * 64 * 8   # elements one pass of the largest grid covers (kMaxGrid tiles of 64 vectors)


def f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def to_bf16(x, rne):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    if not rne:
        return (u >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def expected_bits(s0, s1, mult, rne):
    with np.errstate(all="ignore"):
        return to_bf16((f32(s0) + f32(s1)) * np.float32(mult), rne)


def restate(rows, s0, s1, mult, error, rne):
    """The definition, per row: (bad, first_bad or None, max_error)."""
    with np.errstate(all="ignore"):
        e = f32(expected_bits(s0, s1, mult, rne))
        out = []
        for row in rows:
            diff = np.abs(f32(row) - e)
            bad = ~(diff <= np.float32(error))
            idx = np.flatnonzero(bad)
            fin = diff[bad & ~np.isnan(diff)]
            out.append((int(idx.size), int(idx[0]) if idx.size else None, float(fin.max()) if fin.size else 0.0))
    return out


@functools.lru_cache(maxsize=None)
def sources(n, seed=0):
    """src0, src1: random bf16 in [1, 100), shared by every case of a size (never modified)."""
    rng = np.random.default_rng(1000 + n + seed)
    s = rng.integers(0x3F80, 0x42C8, (2, n)).astype(np.uint16)
    s.setflags(write=False)
    return s[0], s[1]


@functools.lru_cache(maxsize=None)
def correct_row(n, mult, rne, seed=0):
    s0, s1 = sources(n, seed)
    e = expected_bits(s0, s1, mult, rne)
    e.setflags(write=False)
    return e


def device_check(rows, stride, s0, s1, mult, error, rne, calls=1):
    """rows: (R, n) uint16 on the host -> the device records (of the last of `calls` calls)."""
    R, n = rows.shape
    buf = np.full((R, stride), 0xFFFF, dtype=np.uint16)   # the skew holds NaNs: never counted
    buf[:, :n] = rows
    d = torch.from_numpy(buf.view(np.int16)).cuda()
    d0 = torch.from_numpy(np.array(s0).view(np.int16)).cuda()   # (copies: the shared sources are read-only)
    d1 = torch.from_numpy(np.array(s1).view(np.int16)).cuda()
    got = None
    for _ in range(calls):
        rec = t.validate_device(d.data_ptr(), stride, n, R, d0.data_ptr(), d1.data_ptr(), mult, error, rne,
                                torch.cuda.current_stream())
        if got is not None:   # the counters are zeroed before every launch
            assert rec == got
        got = rec
    return got


def host_bad(rows, s0, s1, mult, error, rne, monkeypatch):
    monkeypatch.setenv("ALLRED_BF16_ROUND", "rne" if rne else "trunc")
    n = rows.shape[1]
    return [t.validate_result_vector(np.ascontiguousarray(r).view(np.uint32), np.ascontiguousarray(s0).view(np.uint32),
                                     np.ascontiguousarray(s1).view(np.uint32), n // 2, error, int(2 * mult))[0]
            for r in rows]


def check_all(rows, stride, s0, s1, mult, error, rne, monkeypatch, calls=1):
    got = device_check(rows, stride, s0, s1, mult, error, rne, calls)
    want = restate(rows, s0, s1, mult, error, rne)
    host = host_bad(rows, s0, s1, mult, error, rne, monkeypatch)
    assert [g["bad"] for g in got] == host == [w[0] for w in want]
    assert [g["first_bad"] for g in got] == [w[1] for w in want]
    for g, w in zip(got, want):
        assert g["max_error"] == w[2], (g, w)
    return got


def strides(n):
    return (n, t.preferred_rank_stride(n))


@pytest.mark.parametrize("n", [8, 264, 1024, 65544])
@pytest.mark.parametrize("R", [1, 3, 64])
def test_correct_rows_and_single_wrong_elements(monkeypatch, R, n):
    mult, rne, error = 32.0, 1, 0.0
    s0, s1 = sources(n)
    good = np.tile(correct_row(n, mult, rne), (R, 1))
    for stride in strides(n):
        got = check_all(good, stride, s0, s1, mult, error, rne, monkeypatch, calls=2)
        assert all(g == {"bad": 0, "first_bad": None, "max_error": 0.0} for g in got)
        first = good.copy()
        first[0, 0] += 1                      # index 0 of row 0: the next bf16 up
        got = check_all(first, stride, s0, s1, mult, error, rne, monkeypatch)
        assert (got[0]["bad"], got[0]["first_bad"]) == (1, 0) and sum(g["bad"] for g in got) == 1
        last = good.copy()
        last[R - 1, n - 1] ^= 0x0100          # index n - 1 of the last row
        got = check_all(last, stride, s0, s1, mult, error, rne, monkeypatch, calls=2)
        assert (got[R - 1]["bad"], got[R - 1]["first_bad"]) == (1, n - 1) and sum(g["bad"] for g in got) == 1


def test_more_columns_than_one_grid_pass(monkeypatch):
    """One vector beyond what the launcher's largest grid covers in one pass: the grid-stride
    loop's second trip (workgroup 0 only) and the tiles around the wrap."""
    n, R, mult, rne = GRID_PASS + 8, 3, 2.0, 0
    s0, s1 = sources(n)
    rows = np.tile(correct_row(n, mult, rne), (R, 1))
    rows[0, 0] ^= 0x0080
    rows[1, GRID_PASS - 1] += 1      # last element of the first pass
    rows[1, GRID_PASS] += 1          # first element of the second pass
    rows[2, n - 1] += 1
    got = check_all(rows, n, s0, s1, mult, 0.0, rne, monkeypatch, calls=2)
    assert [(g["bad"], g["first_bad"]) for g in got] == [(1, 0), (2, GRID_PASS - 1), (1, n - 1)]


@pytest.mark.parametrize("error", [0.0, 32.0])
def test_threshold_is_inclusive(monkeypatch, error):
    """diff == error is a match; the next bf16 up is bad."""
    n, mult, rne = 264, 2.0, 1
    s0, s1 = (x.copy() for x in sources(n))
    at = [0, 7, 133, n - 1]
    s0[at] = s1[at] = 0x4280                     # 64 + 64 -> expected 256
    good = expected_bits(s0, s1, mult, rne)
    edge = to_bf16(np.array([256.0 + error], dtype=np.float32), 0)[0]
    assert f32(np.array([edge]))[0] == 256.0 + error      # representable: diff is exactly `error`
    rows = np.tile(good, (3, 1))
    rows[0, at] = edge                            # diff == error everywhere: all match
    rows[1, at] = edge + 1                        # one bf16 step further: all four bad
    rows[2, at[2]] = edge + 1
    for stride in strides(n):
        got = check_all(rows, stride, s0, s1, mult, error, rne, monkeypatch)
        assert [g["bad"] for g in got] == [0, 4, 1]
        assert (got[1]["first_bad"], got[2]["first_bad"]) == (0, at[2])
        assert got[1]["max_error"] == error + 2.0     # bf16 spacing at 256 is 2


def test_nan_and_infinities(monkeypatch):
    """NaN, +inf and -inf results are bad; so is inf - inf (an expected value that overflowed,
    met by an inf result): NaN diffs count but stay out of max_error."""
    n, mult, rne, error = 1024, 32.0, 1, 32.0
    s0, s1 = (x.copy() for x in sources(n))
    s0[[5, 600]] = s1[[5, 600]] = 0x7F7F         # (a + b) * mult overflows to +inf
    good = expected_bits(s0, s1, mult, rne)
    assert good[5] == 0x7F80
    rows = np.tile(good, (4, 1))                 # rows 0..3: inf - inf at 5 and 600 already
    rows[1, 9] = 0x7FC0                          # NaN
    rows[2, 700] = 0x7F80                        # +inf against a finite expected value
    rows[3, 1023] = 0xFF80                       # -inf
    rows[3, 5] = 0xFF80                          # -inf - inf = -inf: diff +inf, not NaN
    for stride in strides(n):
        got = check_all(rows, stride, s0, s1, mult, error, rne, monkeypatch)
        assert [g["bad"] for g in got] == [2, 3, 3, 3]
        assert [g["first_bad"] for g in got] == [5, 5, 5, 5]
        assert [g["max_error"] for g in got] == [0.0, 0.0, float("inf"), float("inf")]


@pytest.mark.parametrize("rne", [0, 1])
def test_every_element_bad(monkeypatch, rne):
    """The rows hold the unreduced inputs (RUN_KERNEL = 0): nearly every element of every row."""
    n, R, mult = 1024, 64, 32.0
    s0, s1 = sources(n)
    rows = np.stack([s1 if (r % 8) % 2 == 0 else s0 for r in range(R)])
    for stride in strides(n):
        got = check_all(rows, stride, s0, s1, mult, 32.0, rne, monkeypatch, calls=2)
        assert all(g["bad"] > n - 8 for g in got)


@pytest.mark.parametrize("mult", [2.0, 32.0, 2048.0])
@pytest.mark.parametrize("rne", [0, 1])
def test_round_modes_and_multipliers(monkeypatch, rne, mult):
    """Rows that are correct under ONE conversion: the other mode sees every element the two
    conversions disagree on; plus scattered errors of one bf16 step."""
    n, R = 264, 3
    s0, s1 = sources(n)
    rows = np.stack([correct_row(n, mult, rne), correct_row(n, mult, 1 - rne), correct_row(n, mult, rne)]).copy()
    rows[2, ::37] += 1
    for error in (0.0, 32.0):
        got = check_all(rows, t.preferred_rank_stride(n), s0, s1, mult, error, rne, monkeypatch)
        assert got[0]["bad"] == 0
    got = check_all(rows, n, s0, s1, mult, 0.0, rne, monkeypatch)
    assert got[1]["bad"] > 0 and got[2]["bad"] == len(range(0, n, 37))


def test_argument_errors_on_the_gpu_box():
    d = torch.zeros(64, dtype=torch.int16, device="cuda")
    for stride, n, rows in ((16, 12, 1), (16, 16, 0), (8, 16, 1), (16, 16, 65)):
        with pytest.raises(t.AllredError) as e:
            t.validate_device(d.data_ptr(), stride, n, rows, d.data_ptr(), d.data_ptr(), 2.0, 0.0)
        assert e.value.status == t._lib.ERR_ARG
