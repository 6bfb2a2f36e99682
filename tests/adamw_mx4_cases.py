"""The data of the AdamW-MXFP4 tests (tests/test_gpu_adamw_mx4.py, tests/test_gpu_soak_adamw_mx4.py): helper, plain
numpy, no GPU and no library needed.  tests/adamw_mx_cases.py with tests/mx4_cases.py's planted blocks and
tests/mxfp4_ref.py's rows.

identity buckets carry mx4_cases.shard in parameter group 1 (weight_decay = 0) with g = m = v = 0: p' has p's bits,
as adamw_mx_cases.identity argues, so the 17 planted MXFP4 blocks reach the quantiser THROUGH the update path.  A
bucket holds 8 total k blocks, never a multiple of 17: a planted block meets every lane octet and tile position.
update buckets are tests/adamw_cases.py's.  expect: adamw_ref.step, then mxfp4_ref.expected_rows of the new param
plane (of p on a skipped step)."""
import numpy as np

import adamw_groups_cases as gc
import adamw_mx_cases as mc
import adamw_ref
import mx4_cases
import mxfp4_ref

FLAGS, LIST, TILES, GROUP_OF = mc.FLAGS, mc.LIST, mc.TILES, mc.GROUP_OF   # blk = 256 and 768, identity and update


def make(total, seed, lst=LIST):
    """data[i] = (p, g, m, v), each (total, 256 k) float32, for the buckets of `lst`"""
    out = []
    for i, (k, kind, _) in enumerate(lst):
        if kind == "identity":
            p = mx4_cases.shard(total, 256 * k, seed + i).copy()
            out.append((p,) + tuple(np.zeros_like(p) for _ in range(3)))
        else:
            out.append(mc.update(kind, seed + i, (total, 256 * k)))
    return out


def expect(data, group_of, norm_sq, total, zero, rceil, groups=gc.GROUPS):
    """per bucket the planes after the call and (element row (n / 2,), scale row (n / 32,)); the info words (group 0's)"""
    planes, rows = [], []
    for i, d in enumerate(data):
        pl, _, _ = adamw_ref.step(*d, gc.eff(group_of[i] if group_of is not None else 0, groups), norm_sq, total, zero)
        planes.append(pl)
        rows.append(mxfp4_ref.expected_rows(pl[0], rceil))
    u = adamw_ref.uniforms(groups[0], norm_sq, total)
    return planes, rows, np.array([u["N"], u["c"], 1.0 if u["skip"] else 0.0, 0.0], dtype=np.float32)
