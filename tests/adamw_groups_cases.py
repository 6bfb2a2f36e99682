"""The parameter groups of the AdamW-groups tests (tests/test_adamw_groups_cases.py on the CPU,
tests/test_gpu_adamw_groups.py on the GPU): plain numpy on tests/adamw_cases.py and
tests/adamw_ref.py, no GPU and no library needed.

GROUPS          three hyper sets that differ in EVERY field (lr, betas, eps, weight_decay — and with
                the betas both bias corrections —, max_norm)
hyper_array(G)  the first G of them as the (G, 8) float32 array the call reads
eff(g)          group g's set with max_norm replaced by group 0's: what the call uses for a bucket
                of group g (allred.h: N, skip and c are the call's, max_norm is hyper[0]'s)
expect(..)      per bucket adamw_ref.step with eff(group_of[i]); info is group 0's
FIELDS          the seven per-group fields by index into a set (max_norm, index 7, is the call's)
"""
import numpy as np

import adamw_cases
import adamw_ref

GROUPS = (
    adamw_cases.hyper(step=3, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=1.0),
    adamw_cases.hyper(step=3, lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0, max_norm=1e-3),
    adamw_cases.hyper(step=3, lr=2e-3, betas=(0.95, 0.95), eps=1e-10, weight_decay=0.1, max_norm=float("inf")),
)
FIELDS = {"lr": 0, "beta1": 1, "beta2": 2, "eps": 3, "weight_decay": 4, "bias_corr1": 5, "bias_corr2_sqrt": 6}
MAX_NORM = 7


def hyper_array(ngroups=3, groups=GROUPS):
    return np.stack(groups[:ngroups]).astype(np.float32)


def eff(g, groups=GROUPS):
    h = np.array(groups[g], dtype=np.float32)
    h[MAX_NORM] = groups[0][MAX_NORM]
    return h


def expect(data, group_of, norm_sq, total, zero, groups=GROUPS):
    """per bucket the planes after the call and the rows' blocks; the info words (group 0's).
    group_of None: every bucket in group 0."""
    planes, rows = [], []
    for i, d in enumerate(data):
        pl, r, _ = adamw_ref.step(*d, eff(group_of[i] if group_of is not None else 0, groups), norm_sq, total, zero)
        planes.append(pl)
        rows.append(r)
    u = adamw_ref.uniforms(groups[0], norm_sq, total)
    info = np.array([u["N"], u["c"], 1.0 if u["skip"] else 0.0, 0.0], dtype=np.float32)
    return planes, rows, info
