"""tests/f32_tree.py — the expectation of the fp32-shard tests — and the inputs it is used on, on
the CPU: the inputs must be able to show a wrong kernel, and the expectation must be what it
says it is.

hard_inputs.cancel discriminates the ORDER of an fp32 tree (a kernel that used one tree for all
blocks, or natural rank order, differs in most columns, before and after the rounding to bf16);
hard_inputs.soft does not — its fp32 tree is the exact sum — and serves as a known answer."""
import numpy as np
import pytest

import f32_tree
import hard_inputs

RANKS = [8, 16, 32, 64]


@pytest.mark.parametrize("total", RANKS)
def test_cancel_data_tells_one_tree_order_from_another(total):
    n = 256 * total
    data = hard_inputs.cancel(total, n, 100 + total)
    natural = f32_tree.tree_sum(data, np.arange(total))
    perm = np.random.default_rng(total).permutation(total)
    assert not np.array_equal(perm, np.arange(total))
    other = f32_tree.tree_sum(data, perm)
    differ = float((natural.view(np.uint32) != other.view(np.uint32)).mean())
    rounded = float((f32_tree.bf16_rne(natural) != f32_tree.bf16_rne(other)).mean())
    print(f"P={total}: fp32 trees differ in {differ:.3f} of the columns, after bf16_rne in {rounded:.3f}")
    assert differ > 0.5
    assert rounded > 0.5


@pytest.mark.parametrize("total", RANKS)
def test_swapping_the_leaves_of_every_pair_changes_no_bit(total):
    data = hard_inputs.cancel(total, 256 * total, 7)
    order = np.random.default_rng(3).permutation(total)
    swapped = order.reshape(-1, 2)[:, ::-1].reshape(-1)
    a, b = f32_tree.tree_sum(data, order), f32_tree.tree_sum(data, swapped)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("total", RANKS)
def test_every_cancel_result_is_finite(total):
    data = hard_inputs.cancel(total, 256 * total, 11)
    for order in (np.arange(total), np.random.default_rng(5).permutation(total)):
        assert np.isfinite(f32_tree.tree_sum(data, order)).all()


@pytest.mark.parametrize("total", RANKS)
@pytest.mark.parametrize("signed", [False, True])
def test_soft_data_sums_exactly_in_any_order(total, signed):
    """a known answer, not a discriminator: the fp32 tree is the float64 sum"""
    data = hard_inputs.soft(total, 256 * total, 13, signed)
    exact = f32_tree.widen(data).astype(np.float64).sum(axis=0)
    for order in (np.arange(total), np.random.default_rng(9).permutation(total)):
        assert np.array_equal(f32_tree.tree_sum(data, order).astype(np.float64), exact)


def test_expect_shard_is_a_multiply_then_an_add():
    """two roundings: (s * scale) rounded to fp32, then old + that rounded again — an fma differs"""
    total, n = 8, 256 * 8
    data = hard_inputs.cancel(total, n, 17)
    order = [list(range(total))] * total
    s = f32_tree.tree_sums(data, order)
    old = np.random.default_rng(1).standard_normal(s.shape).astype(np.float32) * np.float32(3e4)
    want = f32_tree.expect_shard(data, order, 0.1, old)
    product = (s.astype(np.float64) * np.float64(np.float32(0.1))).astype(np.float32)   # exact in float64, rounded once
    assert np.array_equal(want.view(np.uint32), (old + product).view(np.uint32))
    fused =(old.astype(np.float64) + s.astype(np.float64) * np.float64(np.float32(0.1))).astype(np.float32)
    assert (fused.view(np.uint32) != want.view(np.uint32)).any(), "the data cannot tell an fma from mul + add"


def test_bf16_rne_known_answers():
    cases = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F808001: 0x3F81, 0x3F807FFF: 0x3F80, 0x3F818001: 0x3F82,
             0x3F817FFF: 0x3F81, 0x7F7FFFFF: 0x7F80, 0x00000000: 0x0000, 0x80000000: 0x8000, 0x00018000: 0x0002,
             0x00008000: 0x0000, 0x807FFFFF: 0x8080, 0x7F800000: 0x7F80, 0xFF800000: 0xFF80}
    bits = np.array(list(cases), dtype=np.uint32)
    assert f32_tree.bf16_rne(bits.view(np.float32)).tolist() == list(cases.values())
    nans = np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001], dtype=np.uint32).view(np.float32)
    assert f32_tree.is_nan16(f32_tree.bf16_rne(nans)).all()
