"""The cases of the replay soak of k_ag_group_mxfp8_2d (tests/test_gpu_soak_mx2d.py), data only: numpy, no
torch, no library call.  tests/test_mx2d_table.py holds the table against csrc/mx2d_kernels.hip on the CPU.

Every instantiated rank count and all four (RCEIL, ROWS) values on ONE unequal list of matrices at pipe_grid
5: one square per block, two row groups of three column groups, two column groups, five column groups.  A
work unit is at most 4^TSA_MX2D_LG_SIDE squares (csrc/mx2d_span.hpp), so every workgroup walks at least three
units across bucket and block ends and the LDS image rotates."""
import soak_cases as sc

SOAK_FILE = "mx2d_kernels.hip"
SOAK_FORMAT = "k_ag_group_mxfp8_2d<%d, %s, %s>"
SOAK_RANKS = sc.RANKS
SOAK_SHAPES = ((32, 32), (96, 64), (64, 32), (160, 32))   # (cols, R) per bucket
SOAK_SQUARES = tuple(cols // 32 * (R // 32) for cols, R in SOAK_SHAPES)   # per shard block
SOAK_GRID = sc.GRID


def tf(x):
    return "true" if x else "false"


def soak_kernel_name(total, rceil, rows):
    return SOAK_FORMAT % (total, tf(rceil), tf(rows))


def soak_case_id(c):
    return f"mx2d-{c['total']}-{tf(c['rceil'])}-{tf(c['rows'])}"


SOAK_CASES = [{"total": p, "rceil": rceil, "rows": rows, "shapes": SOAK_SHAPES, "grid": SOAK_GRID, "launches": 1}
              for p in SOAK_RANKS for rceil in (False, True) for rows in (False, True)]
