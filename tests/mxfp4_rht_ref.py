"""The numpy expectation of allred_plan_all_gather_shards_mxfp4_rht (helper, no tests): include/allred.h's rotation
written out index by index in float32 — on purpose not the reshaping form of t.hadamard32 —, then mxfp4_ref.quantize."""
import numpy as np

import mxfp4_ref

NORM = np.uint32(0x3E3504F3).view(np.float32)
STRIDES = (1, 2, 4, 8, 16)


def rotate(x, sign_mask, strides=STRIDES):
    """x (..., 32 k) float32 -> the rotated blocks; `strides`: the stage order (the rule's unless a test says otherwise)"""
    v = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 32).copy()
    for i in range(32):
        if sign_mask >> i & 1:
            v[:, i] = (v[:, i].view(np.uint32) ^ np.uint32(0x80000000)).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for h in strides:
            for i in range(32):
                if not i & h:
                    v[:, i], v[:, i + h] = v[:, i] + v[:, i + h], v[:, i] - v[:, i + h]
        v *= NORM
    return v.reshape(np.shape(x))


def expected_rows(blocks, sign_mask, rceil=False):
    """mxfp4_ref.expected_rows of the rotated shard blocks: what EVERY rank's rows receive"""
    return mxfp4_ref.expected_rows(rotate(blocks, sign_mask), rceil)


def cancel_shard(total, blk, seed):
    """(total, blk) float32: small integers in [-3, 3] with +2^25 and -2^25 planted at a pair (i, i + h) of every MX
    block, h cycling over the five strides from block to block and i over the block.  The pair cancels exactly in
    stage h and swallows its partners in every stage run before it, so a wrong stage order, operand order or sign bit
    changes e2m1 nibbles — which it does not on random data (e2m1 is too coarse)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-3, 4, (total * blk // 32, 32)).astype(np.float32)
    for m in range(len(v)):
        h = STRIDES[m % 5]
        i = [k for k in range(32) if not k & h][(m // 5) % 16]
        v[m, i], v[m, i + h] = 2.0 ** 25, -(2.0 ** 25)
    return v.reshape(total, blk)
