"""Rank vectors on which a reduction can be wrong and show it (plain module, no GPU needed).

The suite's usual data — bf16 patterns 0x3F80..0x42C8, values in [1, 100) — sums exactly in
fp32 for up to 64 ranks, so an fp32-accumulating kernel may add in any order and still match
the oracle (tests/test_hard_inputs.py pins that).  The two datasets here do discriminate:

cancel(total, n, seed)     signed [1, 100) values, and in every column +B in one rank and -B
                           in another, B in [2^20, 2^31): while B is in the running sum the
                           small addends lose their low bits, so the result depends on the
                           order of the adds.  Fixed columns hold +0, -0, mixed zeros, the
                           smallest denormals of both signs and x / -x by rank parity.
                           Every result is finite.
nonfinite(total, n, seed)  positive [1, 100) values with columns that must come out as NaN,
                           +Inf or -Inf on every rank that receives them.

Both return a read-write (total, n) uint16 array.  The planted columns sit in the first and
in the last 16-byte vector of the row and on both sides of a block boundary (block = n / total
elements); cancel_columns / nonfinite_columns give (column, class) for a shape.
"""
import numpy as np

LO_BITS, HI_BITS = 0x3F80, 0x42C8      # [1, 100): the range of the suite's other inputs
BIG_LO, BIG_HI = 0x4980, 0x4F00        # [2^20, 2^31)
QNAN, PINF, NINF, MAXF = 0x7FC0, 0x7F80, 0xFF80, 0x7F7F
MIN_ELEMS = 32                         # below this the first and the last vector would overlap the boundary columns

# cancel: class -> what a rank holds in that column
CANCEL_CLASSES = ("pos_zero", "neg_zero", "mixed_zero", "pos_denorm", "neg_denorm", "parity")
# nonfinite: class -> what every receiving rank must hold: "nan" (any NaN) or the exact bits
NONFINITE_CLASSES = {"nan": "nan", "pos_inf": PINF, "inf_minus_inf": "nan", "overflow": PINF, "neg_inf": NINF}
# the classes that need two different ranks
_PAIR_CLASSES = ("inf_minus_inf", "overflow")


def is_nan(bits):
    """bf16 bit patterns (array or int) that are NaNs"""
    return (np.asarray(bits, dtype=np.uint16) & 0x7FFF) > 0x7F80


def _boundary(total, n):
    """an element index where one block ends and the next begins (the middle of the row for one rank)"""
    blk = n // total
    return blk * (total // 2) if total > 1 else n // 2


def _columns(classes, total, n):
    """(column, class): every class once in the first vector, once in the last, once around the boundary —
    the first half of the classes before it, the rest behind it"""
    assert n % 8 == 0 and n >= MIN_ELEMS, f"n = {n}: a multiple of 8, at least {MIN_ELEMS}"
    k, b = len(classes), _boundary(total, n)
    assert k <= 8 and 8 + k // 2 <= b <= n - 8 - (k - k // 2)
    cols = [(i, c) for i, c in enumerate(classes)]
    cols += [(n - 8 + i, c) for i, c in enumerate(classes)]
    cols += [(b - k // 2 + i, c) for i, c in enumerate(classes)]
    assert len({c for c, _ in cols}) == len(cols)
    return cols


def cancel_columns(total, n):
    return _columns(CANCEL_CLASSES, total, n)


def nonfinite_classes(total):
    """one rank cannot hold a pair: the two-rank classes need total >= 2"""
    return tuple(c for c in NONFINITE_CLASSES if total >= 2 or c not in _PAIR_CLASSES)


def nonfinite_columns(total, n):
    return _columns(nonfinite_classes(total), total, n)


def _two_ranks(rng, total, size):
    """two different ranks per column"""
    a = rng.integers(0, total, size)
    b = (a + rng.integers(1, total, size)) % total
    return a, b


def cancel(total, n, seed):
    rng = np.random.default_rng(seed)
    data = rng.integers(LO_BITS, HI_BITS, (total, n)).astype(np.uint16)
    data |= (rng.integers(0, 2, (total, n)) << 15).astype(np.uint16)
    cols = np.arange(n)
    if total >= 2:
        big = rng.integers(BIG_LO, BIG_HI, n).astype(np.uint16)
        plus, minus = _two_ranks(rng, total, n)
        data[plus, cols] = big
        data[minus, cols] = big | 0x8000
    x = rng.integers(LO_BITS, HI_BITS, n).astype(np.uint16)
    r = np.arange(total)
    column = {
        "pos_zero": lambda c: np.full(total, 0x0000),
        "neg_zero": lambda c: np.full(total, 0x8000),
        "mixed_zero": lambda c: np.where(r % 3 == 0, 0x8000, 0x0000),   # rank 0 -0, rank 1 +0
        "pos_denorm": lambda c: np.full(total, 0x0001),
        "neg_denorm": lambda c: np.full(total, 0x8001),
        "parity": lambda c: np.where(r % 2 == 0, x[c], x[c] | 0x8000),
    }
    for c, cls in cancel_columns(total, n):
        data[:, c] = column[cls](c).astype(np.uint16)
    return data


def nonfinite(total, n, seed):
    rng = np.random.default_rng(seed)
    data = rng.integers(LO_BITS, HI_BITS, (total, n)).astype(np.uint16)
    for c, cls in nonfinite_columns(total, n):
        a = int(rng.integers(0, total))
        b = (a + int(rng.integers(1, total))) % total if total >= 2 else a
        if cls == "nan":
            data[a, c] = QNAN
        elif cls == "pos_inf":
            data[a, c] = PINF
        elif cls == "neg_inf":
            data[a, c] = NINF
        elif cls == "inf_minus_inf":
            data[a, c], data[b, c] = PINF, NINF
        else:   # overflow: 2 x 0x7F7F is beyond the largest finite fp32
            data[a, c] = data[b, c] = MAXF
    return data


def soft(total, n, seed, signed=False):
    """the suite's usual range, for the control: [1, 100), positive or with random signs"""
    rng = np.random.default_rng(seed)
    data = rng.integers(LO_BITS, HI_BITS, (total, n)).astype(np.uint16)
    if signed:
        data |= (rng.integers(0, 2, (total, n)) << 15).astype(np.uint16)
    return data


def check_nonfinite(got_row, want_row, total, n, cols=None, offset=0):
    """One result row (or the slice [offset, offset + len) of one) against the oracle's: bit-exact
    outside the planted columns; inside them the stated class, against the oracle and as a known
    answer.  Returns the number of planted columns checked."""
    got_row, want_row = np.asarray(got_row), np.asarray(want_row)
    planted = [(c - offset, cls) for c, cls in (cols or nonfinite_columns(total, n))
               if offset <= c < offset + got_row.size]
    mask = np.ones(got_row.size, dtype=bool)
    for c, cls in planted:
        mask[c] = False
        known = NONFINITE_CLASSES[cls]
        if known == "nan":
            assert is_nan(want_row[c]), f"oracle: column {c + offset} ({cls}) is 0x{int(want_row[c]):04X}, not a NaN"
            assert is_nan(got_row[c]), f"column {c + offset} ({cls}) is 0x{int(got_row[c]):04X}, not a NaN"
        else:
            assert int(want_row[c]) == known, f"oracle: column {c + offset} ({cls}) is 0x{int(want_row[c]):04X}"
            assert int(got_row[c]) == known, f"column {c + offset} ({cls}) is 0x{int(got_row[c]):04X}, not 0x{known:04X}"
    differing = int((got_row[mask] != want_row[mask]).sum())
    assert differing == 0, f"{differing} differing elements outside the planted columns"
    return len(planted)
