"""The shapes and cases of k_ag_group_mxfp8_2d's tests, data only: numpy, no torch, no library call.

SHAPE LISTS.  tests/test_gpu_shards_mxfp8_2d.py runs SHAPES (SHAPES_64 at P = 64) in its first tests and
ROW_GROUP_SHAPES (ROW_GROUP_SHAPES_64) in the tests of several row groups per shard block; shape_class
restates csrc/mx2d_span.hpp's classification, and tests/test_mx2d_classes.py holds the lists against the
classes they are there for, on the CPU.

THE SOAK (tests/test_gpu_soak_mx2d.py; tests/test_mx2d_table.py holds the table against
csrc/mx2d_kernels.hip on the CPU).  Every instantiated rank count and all four (RCEIL, ROWS) values on ONE
unequal list of matrices at pipe_grid 5.  With the build's 64 x 64 patch (TSA_MX2D_LG_SIDE = 1): one square
per block; ONE row group of three column groups of two squares; one unit of two squares; five column groups
of one square; three row groups of one square; two row groups of one unit of four squares.  A work unit is
at most 4^TSA_MX2D_LG_SIDE squares (csrc/mx2d_span.hpp), so every workgroup walks at least three units
across bucket and block ends and the LDS image rotates."""
import soak_cases as sc

# (cols, R) per bucket.  At the build's patch every one of SHAPES, SHAPES_64 and the first four SOAK_SHAPES
# is ONE row group per shard block: the row group enters no offset.
SHAPES = ((32, 32), (96, 64), (160, 32), (64, 64), (128, 32))
SHAPES_64 = ((32, 32), (32, 32), (32, 32))   # P = 64: one square per block
# two or three row groups AND (but for (32, 96)) two or three column groups under each of the four patch
# classes (lgh, lgw); an odd row group count, a column group count that is no power of two
ROW_GROUP_SHAPES = ((32, 96), (96, 96), (96, 128), (128, 96), (192, 128))
# P = 64.  (32, 128), a patch higher than wide, is there for one mistake the other two cannot see: the row group
# shifted by lgw where lgh belongs changes nothing at lgh == lgw (tests/test_mx2d_classes.py)
ROW_GROUP_SHAPES_64 = ((96, 96), (64, 128), (32, 128))
GPU_RANKS = (8, 16, 32)   # the rank counts below 64 of the GPU tests' schedules


def mx2d_lg(x, lg_side):
    """mx2d_span.hpp's mx2d_lg: the largest k <= lg_side with x % 2^k == 0"""
    k = 0
    while k < lg_side and x % (2 << k) == 0:
        k += 1
    return k


def shape_class(cols, R, lg_side):
    """(lgh, lgw, rgs, cgs) of a bucket of shard blocks of R rows of cols floats: the patch is (32 << lgh) rows
    by (32 << lgw) columns, a block has rgs row groups of cgs column groups (mx2d_shape_make)"""
    assert cols > 0 and R > 0 and cols % 32 == 0 and R % 32 == 0
    lgw, lgh = mx2d_lg(cols // 32, lg_side), mx2d_lg(R // 32, lg_side)
    return lgh, lgw, R >> (5 + lgh), cols >> (5 + lgw)


def gpu_shapes(total):
    """every shape the tests of tests/test_gpu_shards_mxfp8_2d.py run at a rank count"""
    return SHAPES_64 + ROW_GROUP_SHAPES_64 if total == 64 else SHAPES + ROW_GROUP_SHAPES


SOAK_FILE = "mx2d_kernels.hip"
SOAK_FORMAT = "k_ag_group_mxfp8_2d<%d, %s, %s>"
SOAK_RANKS = sc.RANKS
SOAK_SHAPES = ((32, 32), (96, 64), (64, 32), (160, 32), (32, 96), (64, 128))   # (cols, R) per bucket
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
