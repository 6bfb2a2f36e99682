"""The data of the AdamW-MXFP8 tests (tests/test_adamw_mx_ref.py on the CPU, tests/test_gpu_adamw_mx.py and
tests/test_gpu_soak_adamw_mx.py on the GPU): plain numpy on tests/mx_cases.py, tests/adamw_cases.py and
tests/adamw_groups_cases.py, no GPU and no library needed.

Two kinds of bucket.
identity(total, blk, seed)   p = mx_cases.shard, g = m = v = 0, to be put in IDENTITY_GROUP = 1 of
                             adamw_groups_cases.GROUPS (weight_decay = 0): d = 1, m' = v' = 0, the ratio
                             is 0 / eps = 0, so p' has p's bits and all 24 planted MX blocks of mx_cases
                             reach the quantiser THROUGH the update path (tests/test_adamw_mx_ref.py).
update(kind, seed, shape)    adamw_cases.planes / negative_v / zero_den, for groups 0 and 2: p' differs
                             from p and may be NaN.
LIST            the bucket list of the GPU tests: tiles per block, kind, group.  blk = 256: one tile per
                block; blk = 768: the 24 planted blocks cycle through every tile position.
expect(..)      per bucket adamw_mx_ref.step with eff(group_of[i]); info is group 0's
FLAGS           the four (zero_grad, rceil) pairs
"""
import numpy as np

import adamw_cases
import adamw_groups_cases as gc
import adamw_mx_ref
import adamw_ref
import mx_cases

F = np.float32
IDENTITY_GROUP = 1
FLAGS = [(False, False), (False, True), (True, False), (True, True)]
# (tiles per block, kind, group)
LIST = ((1, "identity", 1), (3, "identity", 1), (1, "planes", 0), (3, "planes", 2))
TILES = tuple(k for k, _, _ in LIST)
GROUP_OF = tuple(g for _, _, g in LIST)


def identity(total, blk, seed):
    p = mx_cases.shard(total, blk, seed).copy()
    z = np.zeros_like(p)
    return p, z, z.copy(), z.copy()


def update(kind, seed, shape):
    return getattr(adamw_cases, kind)(seed, shape)


def make(total, seed, lst=LIST):
    """data[i] = (p, g, m, v), each (total, 256 k) float32, for the buckets of `lst`"""
    return [identity(total, 256 * k, seed + i) if kind == "identity" else update(kind, seed + i, (total, 256 * k))
            for i, (k, kind, _) in enumerate(lst)]


def expect(data, group_of, norm_sq, total, zero, rceil, groups=gc.GROUPS, wrong=None):
    """per bucket the planes after the call and (element row, scale row); the info words (group 0's)"""
    planes, rows = [], []
    for i, d in enumerate(data):
        pl, r, _ = adamw_mx_ref.step(*d, gc.eff(group_of[i] if group_of is not None else 0, groups), norm_sq, total, zero, rceil,
                                     wrong=wrong)
        planes.append(pl)
        rows.append(r)
    u = adamw_ref.uniforms(groups[0], norm_sq, total)
    info = np.array([u["N"], u["c"], 1.0 if u["skip"] else 0.0, 0.0], dtype=F)
    return planes, rows, info


# ------------------------------------------------------------------ the replay soak's table
# (tests/test_gpu_soak_adamw_mx.py runs it; tests/test_adamw_mx_table.py checks on the CPU that it covers every
# launch adamw_mx_kernels.hip can trace): the one kernel at every instantiated rank count and all four
# (ZERO, RCEIL) values, on soak_cases' UNEQUAL list in the flat layout at pipe_grid 5 with its GROUP_OF.
SOAK_FILE = "adamw_mx_kernels.hip"
SOAK_FORMAT = "k_adamw_ag_mxfp8<%d, %s, %s>"
SOAK_RANKS = (8, 16, 32, 64)
SOAK_TILES = (1, 3, 2, 5)
SOAK_GRID = 5
SOAK_GROUP_OF = (0, 1, 0, 1)
SOAK_CASES = [{"total": p, "zero": z, "rceil": r, "tiles": SOAK_TILES, "grid": SOAK_GRID, "launches": 1}
              for p in SOAK_RANKS for z, r in FLAGS]


def soak_kernel_name(total, zero, rceil):
    return SOAK_FORMAT % (total, "true" if zero else "false", "true" if rceil else "false")


def soak_case_id(c):
    return f"adamw-mx-{c['total']}-zero{int(c['zero'])}-rceil{int(c['rceil'])}"
