"""What allred_plan_adamw_all_gather_shards_mxfp8 must compute (helper, no tests; plain numpy, no GPU
and no library needed): tests/adamw_ref.py's step, then tests/mxfp8_ref.py's quantisation of the new
param plane — or of p on a skipped step.  p' is quantised from fp32: there is no bf16 in between.

step(p, g, m, v, hyper, norm_sq, P, zero_grad, rceil)   (total, blk) arrays -> ((p', g', m', v'), (the element
                                                        row (n,), the scale row (n / 32,)), info)

The mistakes a correct-looking kernel could make instead (tests/test_adamw_mx_ref.py pins that the GPU
tests' data tells them apart):
  quantize_sub(x, rceil, group, pick)   the amax over aligned sub-groups of `group` < 32 elements (two DPP
                                        steps where three are needed give group = 16), the block's scale
                                        byte taken from sub-group `pick` of the block;
  wrong="old_p"                         the rows from p instead of p';
  wrong="bf16"                          the rows from bf16_rne(p') widened again.
"""
import numpy as np

import adamw_ref
import f32_tree
import mxfp8_ref

F = np.float32


def bf16_round(x):
    """bf16_rne(x) widened to float32 again"""
    return (f32_tree.bf16_rne(np.ascontiguousarray(x, dtype=F)).astype(np.uint32) << 16).view(F)


def step(p, g, m, v, hyper, norm_sq, P, zero_grad, rceil, wrong=None):
    planes, _, info = adamw_ref.step(p, g, m, v, hyper, norm_sq, P, zero_grad)
    src = planes[0]   # p' — p itself on a skipped step
    if wrong == "old_p":
        src = np.asarray(p, dtype=F)
    elif wrong == "bf16":
        src = bf16_round(src)
    e, s = mxfp8_ref.quantize(np.ascontiguousarray(src, dtype=F), rceil)
    return planes, (e.reshape(-1), s.reshape(-1)), info


def quantize_sub(x, rceil, group, pick=0):
    """x (..., 32 k) float32 -> (element bytes, scale bytes) as a kernel writes them whose amax reaches
    over aligned sub-groups of `group` < 32 elements only: every sub-group's elements are scaled by its OWN
    amax's exponent, and the block's scale byte is the one sub-group `pick` of the block holds"""
    x = np.ascontiguousarray(x, dtype=F)
    A = mxfp8_ref.block_amax_bits(x, group)                    # (..., 32 k / group)
    X, special = mxfp8_ref.scale_exponent(A, rceil), mxfp8_ref.is_special(A)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x.reshape(X.shape + (group,)) * mxfp8_ref.pow2(-X)[..., None]).reshape(x.shape)
    elems = np.where(np.repeat(special, group, axis=-1), np.uint8(mxfp8_ref.NAN_BYTE), mxfp8_ref.e4m3_bytes(y))
    per = 32 // group
    Xb, sb = X.reshape(X.shape[:-1] + (-1, per))[..., pick], special.reshape(special.shape[:-1] + (-1, per))[..., pick]
    return elems, np.where(sb, mxfp8_ref.NAN_SCALE, Xb + 127).astype(np.uint8)
