"""What the grouped calls on fp32 shards must compute, in numpy float32 (plain module, no GPU,
no library needed).  numpy's float32 arithmetic is IEEE: round to nearest even, no flushing
of denormals, one rounding per operation.

tree_sum(data, order_row)                     the BO tree of one block: leaves = the rank rows in
                                              order_row's order, widened bf16 -> fp32 exactly, level k
                                              adds adjacent groups of 2^k leaves, every add one fp32 add
expect_shard(data, tree_order, scale, old)    (P, blk) float32: block b = tree b of columns
                                              [b blk, (b + 1) blk), times scale, then old + that —
                                              two separate float32 operations (no fma)
bf16_rne(f32)                                 uint16: the integer rule (u + 0x7FFF + ((u >> 16) & 1)) >> 16;
                                              a NaN comes out as SOME NaN: compare NaNs by class (same_bf16)

WHERE THE ORDER IS PINNED.  The callers pass t.schedule(...)["tree_order"], the table the product uploads and
its kernels read.  tests/test_bo_tree.py holds that table to the reference on the CPU: the tree derived from
the partners and receive masks of tests/golden/schedule_ref.json alone (tests/bo_tree.py) is, up to swapping
the children of a node, the balanced pairing tree_sum applies to tree_order[b], for every grid the GPU tests
run — the 8 x 4 grid of their 32-rank cases included — and for Swing-1D at 8 ranks; its float32 bits equal
tree_sums', and with every add rounded to bf16 it is the CPU oracle's BO allreduce.
"""
import numpy as np


def widen(u16):
    """bf16 bit patterns -> the float32 of the same value (exact)"""
    return (np.asarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def tree_sum(data_u16, order_row):
    """(P, m) uint16 bf16 patterns, P a power of two -> (m,) float32"""
    data_u16 = np.asarray(data_u16)
    order = np.asarray(order_row, dtype=np.int64)[:data_u16.shape[0]]
    assert sorted(order.tolist()) == list(range(data_u16.shape[0]))
    x = widen(data_u16)[order]
    with np.errstate(all="ignore"):
        while x.shape[0] > 1:
            x = x[0::2] + x[1::2]
    assert x.dtype == np.float32
    return x[0]


def tree_sums(data_u16, tree_order):
    """(P, n) -> (P, blk) float32: row b = tree b over columns [b blk, (b + 1) blk)"""
    total, n = data_u16.shape
    blk = n // total
    return np.stack([tree_sum(data_u16[:, b * blk:(b + 1) * blk], tree_order[b]) for b in range(total)])


def scaled(sums, scale, old=None):
    """sums * scale, then old + that: separate float32 operations"""
    with np.errstate(all="ignore"):
        v = sums * np.float32(scale)
        if old is not None:
            v = np.asarray(old, dtype=np.float32) + v
    assert v.dtype == np.float32
    return v


def expect_shard(data_u16, tree_order, scale, old=None):
    return scaled(tree_sums(data_u16, tree_order), scale, old)


def is_nan32(f32):
    return (np.asarray(f32, dtype=np.float32).view(np.uint32) & 0x7FFFFFFF) > 0x7F800000


def is_nan16(u16):
    return (np.asarray(u16, dtype=np.uint16) & 0x7FFF) > 0x7F80


def bf16_rne(f32):
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(is_nan32(f32), np.uint16(0x7FC0), r).astype(np.uint16)


def same_f32(got, want):
    """bit-equal as uint32, NaNs by class"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    gn, wn = is_nan32(got), is_nan32(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~wn], want.view(np.uint32)[~wn]))


def same_bf16(got, want):
    """bit-equal, NaNs by class"""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    gn, wn = is_nan16(got), is_nan16(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got[~wn], want[~wn]))
