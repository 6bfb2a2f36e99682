"""Where the fp32 family's tree comes from.  tests/f32_tree.py evaluates "the tree of block b" over
t.schedule(...)["tree_order"] — the table the product uploads and its kernels read.  Here that table is
held to the reference: tests/bo_tree.py derives every block's tree from the partners and receive masks of
tests/golden/schedule_ref.json (the reference's own functions) alone, and

  structure   it is, up to swapping the two children of a node, the balanced pairing f32_tree.tree_sum
              applies to tree_order[b] — no data involved;
  fp32 bits   evaluated in float32 on hard_inputs.cancel it equals f32_tree.tree_sums bit for bit;
  bf16 bits   with every add rounded to bf16 it equals oracle.allreduce("bo", ...) bit for bit.

Every valid golden grid, both algorithms; and Swing-1D at 8 ranks, the other schedule the fp32 GPU tests
run, with the masks of oracle.schedule (test_schedule pins its partners to the reference)."""
import numpy as np
import pytest

import bo_tree
import f32_tree
import hard_inputs
import oracle
import tenstorrentallreduce_amd as t
from test_schedule import VALID

ALGOS = {"swing": t.SWING, "recdub": t.RECDUB}
CASES = [(name, side, total) for side, total in sorted(VALID) for name in sorted(ALGOS)] + [("swing_1d", 1, 8)]
cases = pytest.mark.parametrize("name,side,total", CASES, ids=[f"{a}-{s}x{p}" for a, s, p in CASES])


def reference_trees(golden, name, side, total):
    """(the product's algo id, the trees derived from the golden partners and masks)"""
    if name == "swing_1d":
        rc, s = oracle.schedule(oracle.SWING_1D, 1, total)
        assert rc == 0
        want = [g for g in golden["swing_1d"] if g["total"] == total][0]["partners"]
        partners = [[s.partner[r][k] for k in range(s.steps)] for r in range(total)]
        assert partners == want
        return t.SWING_1D, bo_tree.derive(partners, [[s.recv[r][k] for k in range(s.steps)] for r in range(total)])
    g = [g for g in golden["grids"] if (g["algo"], g["side"], g["total"]) == (name, side, total)]
    assert len(g) == 1
    ranks = g[0]["ranks"]
    return ALGOS[name], bo_tree.derive([r["partners"] for r in ranks], [r["recv"] for r in ranks])


@cases
def test_every_block_tree_has_every_rank_once(golden_schedule, name, side, total):
    _, trees = reference_trees(golden_schedule, name, side, total)
    for b, tree in enumerate(trees):
        assert sorted(bo_tree.leaves(tree)) == list(range(total)), f"block {b}"


@cases
def test_structure_is_the_balanced_pairing_of_tree_order(golden_schedule, name, side, total):
    algo, trees = reference_trees(golden_schedule, name, side, total)
    order = t.schedule(algo, side, total)["tree_order"]
    for b in range(total):
        assert bo_tree.canonical(trees[b]) == bo_tree.canonical(bo_tree.balanced(order[b][:total])), f"block {b}"


@cases
def test_a_tree_order_with_two_leaves_of_different_pairs_exchanged_fails(golden_schedule, name, side, total):
    """the negative control of the structure test; below 4 ranks there are no two pairs"""
    algo, trees = reference_trees(golden_schedule, name, side, total)
    order = t.schedule(algo, side, total)["tree_order"]
    for b in range(total if total >= 4 else 0):
        for i, j in ((0, 2), (1, total - 1)):
            wrong = list(order[b][:total])
            wrong[i], wrong[j] = wrong[j], wrong[i]
            assert bo_tree.canonical(trees[b]) != bo_tree.canonical(bo_tree.balanced(wrong)), f"block {b}"
    # and swapping the two leaves of a pair is no change: the canonical form is what it says
    for b in range(total if total >= 2 else 0):
        same = list(order[b][:total])
        same[0], same[1] = same[1], same[0]
        assert bo_tree.canonical(trees[b]) == bo_tree.canonical(bo_tree.balanced(same))


@cases
def test_fp32_bits_equal_f32_tree(golden_schedule, name, side, total):
    algo, trees = reference_trees(golden_schedule, name, side, total)
    data = hard_inputs.cancel(total, 32 * total, 40 + total)
    want = f32_tree.tree_sums(data, t.schedule(algo, side, total)["tree_order"])
    got = bo_tree.evaluate_blocks(trees, data)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@cases
def test_bf16_bits_equal_the_oracle_allreduce(golden_schedule, name, side, total):
    """every add one float32 add rounded to bf16 by the integer rule: the BO allreduce of the CPU oracle"""
    algo, trees = reference_trees(golden_schedule, name, side, total)
    data = hard_inputs.cancel(total, 32 * total, 60 + total)
    ranks = [row.copy() for row in data]
    oracle.allreduce("bo", algo, side, ranks, total)
    got = f32_tree.bf16_rne(bo_tree.evaluate_blocks(trees, data, bf16=True)).reshape(-1)
    assert not f32_tree.is_nan16(got).any()
    for r in range(total):
        assert np.array_equal(ranks[r], got), f"rank {r}"


def test_the_trees_of_a_grid_differ_from_block_to_block(golden_schedule):
    """so one tree for all blocks cannot pass the tests above: 8 x 4 Swing, the grid this file adds"""
    _, trees = reference_trees(golden_schedule, "swing", 8, 32)
    assert len({bo_tree.canonical(tr) for tr in trees}) > 1
