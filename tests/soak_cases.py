"""The cases of the replay soak (tests/soak.py), data only: numpy, no torch, no library call.

tests/test_gpu_soak_shards.py runs them, tests/test_gpu_soak_routes.py uses ROUTE_EXCLUDED, and
tests/test_soak_table.py checks on the CPU that the table covers every launch the three shard-family
kernel files can trace and that arrangement (c) lies where it says.

SHARD_CASES: every kernel of shard_f32_kernels.hip, adamw_kernels.hip and mx_kernels.hip at every
instantiated rank count and both values of its bool, on the UNEQUAL (1, 3, 2, 5) list in the flat layout
at pipe_grid 5: every workgroup walks at least three tiles across bucket and block ends with loads in
flight, and the wait constants differ per rank count.

HANDOFF_CASES: the one in-launch hand-off between workgroups (norm_finish) in four more arrangements,
ACC both ways:
  eighty   the STRIDED list: 80 partials per rank, the strided sum past 64.
  grid     a pipe_grid larger than the tile count.  The launcher clamps the grid to the tile count
           (launch_util.hpp persistent_grid), so through the library no workgroup is without a tile;
           what this arrangement reaches is G = T, one tile per workgroup: the shortest walk before the ticket.
  warm     arrangement (c), below.
  chain    65 buckets: two launches back to back on one workspace, the second adding to norm_sq.

ARRANGEMENT (c), `warm`: one bucket of one tile per block (blk = 256 floats = 1024 bytes), P = 8 and 64.
With B a 128-byte aligned address:
    shard           = B + 16                      block b at shard + 4 b WARM_STRIDE
    WARM_STRIDE     = 256 + 80 floats             a gap of 320 bytes behind every block
    workspace       = B + 16 + 1024 = the first byte behind block 0 (16-byte aligned): 64 counter bytes,
                      then the P partials
    P = 8    the workspace is 96 bytes, [B + 1040, B + 1136): ONE 128-byte line, [B + 1024, B + 1152),
             which begins with the last 16 bytes of block 0.
    P = 64   the workspace is 320 bytes = the whole gap, [B + 1040, B + 1360); block 1 begins at B + 1360.
             The partials, [B + 1104, B + 1360), lie in three lines: line 8 of B (with block 0's last 16
             bytes and the counter), line 9 — 32 partials and nothing else: 256 contiguous bytes of
             partials cannot leave room in every line —, and line 10, which holds 20 partials and the
             first 48 bytes of block 1.
The ACC form loads every shard float of the launch, so it pulls those lines into the L2 the finalizer
reads through, before or while the partials are written: the nearest thing to a pre-reading consumer
that needs no change to the kernel.  The ranges rule accepts a workspace in a stride's gap.
"""
import numpy as np

# the route cases the soak leaves out: exactly those whose trace is empty (they enqueue nothing)
ROUTE_EXCLUDED = ("rs-inplace-one-rank", "ag-inplace-one-rank", "lo-one-rank-butterfly")

SEEDS = (21, 22)                 # the two datasets of a soak
RANKS = (8, 16, 32, 64)          # every instance of for_ranks<8, 64>
SIDE = {8: 4, 16: 4, 32: 8, 64: 8}
UNEQUAL = (1, 3, 2, 5)
GRID = 5
SCALE = 0.1
GROUP_OF = (0, 1, 0, 1)          # two parameter groups alternating bucket by bucket

# family -> (kernel file, trace_launch format, the bool's values or None)
KERNELS = {
    "tree": ("shard_f32_kernels.hip", "k_tree_group_f32<%d, %s>", (False, True)),
    "norm": ("shard_f32_kernels.hip", "k_tree_group_f32_norm<%d, %s>", (False, True)),
    "ag": ("shard_f32_kernels.hip", "k_ag_group_f32<%d>", None),
    "adamw": ("adamw_kernels.hip", "k_adamw_ag_group_f32<%d, %s>", (False, True)),
    "groups": ("adamw_kernels.hip", "k_adamw_ag_groups_f32<%d, %s>", (False, True)),
    "mxfp8": ("mx_kernels.hip", "k_ag_group_mxfp8<%d, %s>", (False, True)),
}


def kernel_name(family, total, flag):
    fmt = KERNELS[family][1]
    return fmt % total if flag is None else fmt % (total, "true" if flag else "false")


def case_id(c):
    flag = "" if c["flag"] is None else ("-true" if c["flag"] else "-false")
    return f"{c['family']}-{c.get('arrangement', 'unequal')}-{c['total']}{flag}"


SHARD_CASES = [{"family": f, "total": p, "flag": flag, "tiles": UNEQUAL, "grid": GRID, "launches": 1}
               for f, (_, _, flags) in KERNELS.items() for p in RANKS for flag in (flags or (None,))]

STRIDED_TILES = (5,) * 16        # f32_norm_cases.STRIDED's list at P = 8: 80 partials per rank
HANDOFF_CASES = [dict(family="norm", arrangement=a, total=p, flag=acc, tiles=tiles, grid=grid, launches=n)
                 for a, p, tiles, grid, n in (("eighty", 8, STRIDED_TILES, GRID, 1),
                                              ("grid", 8, (1,), 64, 1),
                                              ("warm", 8, (1,), 0, 1),
                                              ("warm", 64, (1,), 0, 1),
                                              ("chain", 8, (1,) * 65, 0, 2))
                 for acc in (False, True)]

# ------------------------------------------------------------------ arrangement (c): the byte layout
LINE = 128
WARM_BLK = 256                   # floats per block: one tile
WARM_SHARD_OFF = 16              # bytes from the 128-byte aligned base B to block 0
WARM_STRIDE = WARM_BLK + 80      # floats from block to block
WARM_WS_OFF = WARM_SHARD_OFF + 4 * WARM_BLK   # bytes from B to the workspace: the first byte behind block 0
COUNTER_BYTES = 64


def warm_layout(total):
    """byte offsets from B: (blocks [(first, last + 1)], workspace (first, last + 1), partials (first, last + 1), buffer bytes)"""
    blocks = [(WARM_SHARD_OFF + 4 * b * WARM_STRIDE, WARM_SHARD_OFF + 4 * b * WARM_STRIDE + 4 * WARM_BLK) for b in range(total)]
    ws = (WARM_WS_OFF, WARM_WS_OFF + COUNTER_BYTES + 4 * total)
    return blocks, ws, (ws[0] + COUNTER_BYTES, ws[1]), 4 * total * WARM_STRIDE + LINE


def finite_planes(seed, shape):
    """(p, g, m, v) float32 for the AdamW soaks: finite, of ordinary magnitude, v >= 0 — nothing in them or in
    what the step makes of them is compared by class"""
    rng = np.random.default_rng(seed)
    p, g, m = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    v = (rng.random(shape) * 1e-2).astype(np.float32)
    return p, g, m, v


def finite_floats(seed, shape):
    """finite float32 of both signs, magnitudes 2^-7 .. 2^9: their squares and sums stay finite"""
    rng = np.random.default_rng(seed)
    bits = (rng.integers(0, 2, shape, dtype=np.uint32) << 31) | (rng.integers(120, 136, shape, dtype=np.uint32) << 23) \
        | rng.integers(0, 1 << 23, shape, dtype=np.uint32)
    return bits.view(np.float32)
