"""What the shape lists of k_ag_group_mxfp8_2d's GPU tests (tests/mx2d_cases.py) can see, on the CPU.

A work unit `rem` of a shard block is split into (row group, column group), and the row group enters three
offsets of csrc/mx2d_span.hpp's mx2d_unit_at: the shard read, the row-wise rows and the t rows.  At ONE row group
per block all three terms vanish.

1. THE CENSUS.  mx2d_cases.shape_class (held against the C++ by tests/test_mx2d_span.py) classifies every shape
   at the build's TSA_MX2D_LG_SIDE: the first lists have one row group throughout; ROW_GROUP_SHAPES,
   ROW_GROUP_SHAPES_64 and the soak's list have the classes they are there for.
2. THE SHAPES DISCRIMINATE.  mx2d_ref.walk emulates the kernel's placement from a restatement of mx2d_unit_at.
   Unchanged, it gives the expectation bit for bit at every shape the GPU runs.  With one of three mistakes in
   the row-group terms it STILL gives the expectation at every shape of the first lists — the suite was blind
   to them — and differs, in element bytes and not in scale bytes alone, at every shape of the new lists.  A
   control mutant that needs no second row group already differs at a shape of the first lists.
"""
import functools
import os
import re

import numpy as np
import pytest

import mx2d_cases as mc
import mx2d_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")
ROW_GROUP_MUTANTS = mx2d_ref.MUTANTS[:3]
CONTROL = mx2d_ref.MUTANTS[3]
SEED = 3


@functools.lru_cache(maxsize=None)
def lg_side():
    with open(os.path.join(CSRC, "mx2d_span.hpp")) as f:
        return int(re.search(r"#define TSA_MX2D_LG_SIDE (\d+)", f.read()).group(1))


def cls(shape):
    return mc.shape_class(*shape, lg_side())


def table(*lists):
    """(P, (cols, R)) of every (rank counts, shapes) pair, each once, in order"""
    return list(dict.fromkeys((p, s) for ranks, shapes in lists for p in ranks for s in shapes))


# every (P, shape) a GPU test runs: the lists from before the row-group tests, and those that came with them
OLD = table((mc.GPU_RANKS, mc.SHAPES), ((64,), mc.SHAPES_64), (mc.SOAK_RANKS, mc.SOAK_SHAPES[:4]))
NEW = table((mc.GPU_RANKS, mc.ROW_GROUP_SHAPES), ((64,), mc.ROW_GROUP_SHAPES_64), (mc.SOAK_RANKS, mc.SOAK_SHAPES[4:]))
ids = lambda table: [f"P{p}-{c}x{r}" for p, (c, r) in table]  # noqa: E731
old_shapes = pytest.mark.parametrize("total,shape", OLD, ids=ids(OLD))
new_shapes = pytest.mark.parametrize("total,shape", NEW, ids=ids(NEW))
all_shapes = pytest.mark.parametrize("total,shape", OLD + NEW, ids=ids(OLD + NEW))


# ------------------------------------------------------------------ 1. the census
def test_shape_class_restates_the_header():
    assert mc.shape_class(32, 32, 1) == (0, 0, 1, 1) and mc.shape_class(96, 64, 1) == (1, 0, 1, 3)
    assert mc.shape_class(96, 64, 0) == (0, 0, 2, 3) and mc.shape_class(256, 128, 1) == (1, 1, 2, 4)
    assert mc.shape_class(256, 128, 2) == (2, 2, 1, 2) and mc.shape_class(64, 192, 2) == (1, 1, 3, 1)
    for cols, R in mc.SHAPES + mc.SHAPES_64 + mc.ROW_GROUP_SHAPES + mc.ROW_GROUP_SHAPES_64 + mc.SOAK_SHAPES:
        for lg in (0, 1):
            lgh, lgw, rgs, cgs = mc.shape_class(cols, R, lg)
            assert lgh <= lg and lgw <= lg and (rgs << (5 + lgh)) == R and (cgs << (5 + lgw)) == cols
            assert (lgh == lg or rgs % 2) and (lgw == lg or cgs % 2)  # the largest patch the divisibility allows


def test_the_first_lists_have_one_row_group_throughout():
    """a stated fact about what the lists before ROW_GROUP_SHAPES could see at the build's 64 x 64 patch"""
    assert lg_side() == 1
    assert mc.SHAPES == ((32, 32), (96, 64), (160, 32), (64, 64), (128, 32)) and set(mc.SHAPES_64) == {(32, 32)}
    assert mc.SOAK_SHAPES[:4] == ((32, 32), (96, 64), (64, 32), (160, 32))
    for shape in mc.SHAPES + mc.SHAPES_64 + mc.SOAK_SHAPES[:4]:
        assert cls(shape)[2] == 1, shape
    assert {(p, s) for p, s in OLD} >= {(p, s) for p in mc.GPU_RANKS for s in mc.SHAPES}


def test_below_64_ranks_every_patch_class_has_row_groups_and_column_groups():
    lg = lg_side()
    classes = [cls(s) for s in mc.gpu_shapes(8)]
    assert mc.gpu_shapes(8) == mc.gpu_shapes(16) == mc.gpu_shapes(32) == mc.SHAPES + mc.ROW_GROUP_SHAPES
    for lgh in range(lg + 1):
        for lgw in range(lg + 1):
            assert any(c[:2] == (lgh, lgw) and c[2] >= 2 and c[3] >= 2 for c in classes), (lgh, lgw)
    assert any(rgs >= 3 and rgs % 2 for _, _, rgs, _ in classes), "no odd row group count"
    assert any(rgs >= 2 and cgs & (cgs - 1) for _, _, rgs, cgs in classes), "no column group count off the powers of two"
    # lgw taken for lgh shows only where they differ: a patch higher than wide and one wider than high
    assert any(lgh > lgw and rgs >= 2 for lgh, lgw, rgs, _ in classes) and any(lgh < lgw and rgs >= 2 for lgh, lgw, rgs, _ in classes)
    if lg == 1:
        assert [cls(s) for s in mc.ROW_GROUP_SHAPES] == [(0, 0, 3, 1), (0, 0, 3, 3), (1, 0, 2, 3), (0, 1, 3, 2), (1, 1, 2, 3)]


def test_at_64_ranks_row_groups_under_the_smallest_and_the_largest_patch():
    lg = lg_side()
    classes = [cls(s) for s in mc.gpu_shapes(64)]
    assert any(lgh == 0 and rgs >= 2 for lgh, _, rgs, _ in classes)
    assert any(lgh == lg and rgs >= 2 for lgh, _, rgs, _ in classes)
    assert any(cgs >= 2 for _, _, _, cgs in classes)
    assert any(lgh != lgw and rgs >= 2 for lgh, lgw, rgs, _ in classes)   # where lgw taken for lgh shows
    if lg == 1:
        assert [cls(s) for s in mc.ROW_GROUP_SHAPES_64] == [(0, 0, 3, 3), (1, 1, 2, 1), (1, 0, 2, 1)]
    assert all(64 * cols * R <= 1 << 20 for cols, R in mc.gpu_shapes(64))
    assert all(32 * cols * R <= 1 << 20 for cols, R in mc.gpu_shapes(32))


def test_the_soak_list_has_row_groups_under_the_smallest_and_the_largest_patch():
    lg = lg_side()
    classes = [cls(s) for s in mc.SOAK_SHAPES]
    assert any(lgh == 0 and rgs >= 2 for lgh, _, rgs, _ in classes)
    assert any(lgh == lg and rgs >= 2 for lgh, _, rgs, _ in classes)
    assert mc.SOAK_SHAPES[4:] == ((32, 96), (64, 128))
    assert all(max(mc.SOAK_RANKS) * cols * R <= 1 << 20 for cols, R in mc.SOAK_SHAPES)


def test_every_new_shape_has_several_row_groups():
    assert all(cls(s)[2] >= 2 for _, s in NEW)
    assert not set(OLD) & set(NEW) and len(set(NEW)) == len(NEW) >= 3 * len(mc.ROW_GROUP_SHAPES) + len(mc.ROW_GROUP_SHAPES_64)


# ------------------------------------------------------------------ 2. the placement emulator and its mutants
@functools.lru_cache(maxsize=None)
def matrix(total, cols, R):
    W = mx2d_ref.hard_t(total, cols, R, SEED)
    W.flags.writeable = False
    return W


@functools.lru_cache(maxsize=None)
def expected(total, cols, R, rceil):
    W = matrix(total, cols, R)
    return mx2d_ref.expected_rows(W, total, rceil) + mx2d_ref.expected_t(W, rceil)


NAMES = ("rows", "scales", "t rows", "t scales")


def differing(total, shape, rceil, mutant):
    """the names of the outputs in which walk differs from the expectation"""
    got = mx2d_ref.walk(matrix(total, *shape), total, rceil, lg_side(), mutant)
    want = expected(total, *shape, rceil)
    assert [g.shape for g in got] == [w.shape for w in want] and all(g.dtype == np.uint8 for g in got)
    return [name for name, g, w in zip(NAMES, got, want) if not np.array_equal(g, w)]


@pytest.mark.parametrize("rceil", [False, True], ids=["floor", "rceil"])
@all_shapes
def test_the_emulated_walk_is_the_expectation(total, shape, rceil):
    assert differing(total, shape, rceil, None) == []
    if not rceil:
        return
    W = mx2d_ref.hard_rows(total, *shape, SEED)   # the other kind of data, under one rule
    got = mx2d_ref.walk(W, total, rceil, lg_side())
    for name, g, w in zip(NAMES, got, mx2d_ref.expected_rows(W, total, rceil) + mx2d_ref.expected_t(W, rceil)):
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("mutant", ROW_GROUP_MUTANTS)
@old_shapes
def test_the_first_lists_are_blind_to_a_wrong_row_group_term(total, shape, mutant):
    assert differing(total, shape, False, mutant) == []
    assert differing(total, shape, True, mutant) == []


@pytest.mark.parametrize("mutant", ROW_GROUP_MUTANTS)
@new_shapes
def test_the_new_lists_see_a_wrong_row_group_term(total, shape, mutant):
    """ONE condition cannot hold at every shape: where the patch is as high as wide (lgh == lgw), lgw in place of
    lgh is no mistake, and row_group_shift_lgw must give the expectation there.  It is held at the shapes with
    lgh != lgw, and the census above demands such shapes at every rank count."""
    lgh, lgw, _, _ = cls(shape)
    if mutant == "row_group_shift_lgw" and lgh == lgw:
        assert differing(total, shape, False, mutant) == differing(total, shape, True, mutant) == []
        return
    for rceil in (False, True):
        names = differing(total, shape, rceil, mutant)
        assert set(names) & {"rows", "t rows"}, f"differs in {names}: a scale row alone, or nothing"
    if mutant != "src_ignores_row_group":   # a misplaced patch shows in BOTH orientations, elements and scales
        assert differing(total, shape, False, mutant) == list(NAMES)


def test_the_control_mutant_shows_on_the_first_lists_already():
    """the method itself: a mistake that needs no second row group is seen where the row-group mutants are not"""
    seen = [s for s in mc.SHAPES if set(differing(8, s, False, CONTROL)) & {"rows", "t rows"}]
    assert seen == [s for s in mc.SHAPES if cls(s)[3] >= 2] and len(seen) >= 2, seen
    assert differing(8, (32, 32), False, CONTROL) == []   # one unit per block: nothing to swap
