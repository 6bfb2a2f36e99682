"""The BO tree of every block, derived from a schedule's partners and receive masks ALONE (helper, no
tests): no tree_order, no library.  With tests/golden/schedule_ref.json as the source these are the
reference's own functions' trees.

A tree is a leaf (a rank, an int) or a pair (left, right) of trees.  expr[r][b] is what rank r holds of
block b: at first the leaf r; at step k, for every block b in recv[r][k], rank r adds what its partner
held of b after step k - 1 to what it held itself.  After the last step rank b holds block b's tree."""
import numpy as np

import f32_tree


def bits(mask):
    return [b for b in range(mask.bit_length()) if mask >> b & 1]


def derive(partners, recv):
    """partners[r][k], recv[r][k] (block masks) -> [tree of block b for b in range(total)]"""
    total = len(partners)
    expr = [[r] * total for r in range(total)]
    for k in range(len(partners[0]) if total else 0):
        prev = expr
        expr = [row[:] for row in prev]
        for r in range(total):
            p = partners[r][k]
            for b in bits(recv[r][k]):
                expr[r][b] = (prev[r][b], prev[p][b])
    return [expr[b][b] for b in range(total)]


def balanced(order):
    """the tree f32_tree.tree_sum applies to a tree_order row: level k pairs adjacent groups of 2^k leaves"""
    x = [int(v) for v in order]
    assert len(x) & (len(x) - 1) == 0
    while len(x) > 1:
        x = [(x[i], x[i + 1]) for i in range(0, len(x), 2)]
    return x[0]


def leaves(tree):
    return [tree] if isinstance(tree, int) else leaves(tree[0]) + leaves(tree[1])


def canonical(tree):
    """the tree up to swapping the two children of a node: at every node the child with the smaller least leaf first"""
    if isinstance(tree, int):
        return tree
    a, b = canonical(tree[0]), canonical(tree[1])
    return (a, b) if min(leaves(a)) < min(leaves(b)) else (b, a)


def evaluate(tree, data_u16, bf16=False):
    """(P, m) bf16 patterns -> (m,) float32: every node ONE float32 add, rounded to bf16 (f32_tree.bf16_rne, then
    widened again) if bf16"""
    if isinstance(tree, int):
        return f32_tree.widen(data_u16[tree])
    with np.errstate(all="ignore"):
        s = evaluate(tree[0], data_u16, bf16) + evaluate(tree[1], data_u16, bf16)
    assert s.dtype == np.float32
    return f32_tree.widen(f32_tree.bf16_rne(s)) if bf16 else s


def evaluate_blocks(trees, data_u16, bf16=False):
    """(P, n) -> (P, blk) float32: row b = tree b over columns [b blk, (b + 1) blk)"""
    total, n = data_u16.shape
    blk = n // total
    return np.stack([evaluate(trees[b], data_u16[:, b * blk:(b + 1) * blk], bf16) for b in range(total)])
