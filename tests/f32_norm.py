"""What allred_plan_reduce_scatter_shards_f32_norm must leave in norm_sq, in numpy float32 (plain
module, no GPU, no library needed), on top of tests/f32_tree.py.  numpy's float32 arithmetic is
IEEE: one rounding per operation, no fma, no flushing.

tile_partial(tile)            256 float32 -> the balanced binary tree over their squares in element
                              order: one multiply each, level k adds adjacent groups of 2^k
launch_sum(partials)          a rank's tile partials S of ONE launch, in list order -> a_l = the
                              left-to-right sum of S[l], S[l + 64], .. from +0.0f (l = 0 .. 63), then
                              the balanced tree over a_0 .. a_63
expect_norm_sq(blocks)        blocks[i]: (P, blk_i) float32, the values the call STORED into bucket
                              i's blocks -> (P,) float32: launch k covers buckets [64 k, 64 k + 64);
                              norm_sq[b] = (..(R_0 + R_1) + R_2 ..)

The alternatives a correct-looking kernel could compute instead (tests/test_f32_norm.py pins that
the GPU tests' data tells them apart): tile_partial_sequential, tile_partial_fma,
tile_partial_c_first, launch_sum_sequential.
"""
import numpy as np

TILE = 256
LANES = 64
GROUP_MAX = 64


def tree(x):
    """balanced binary tree over axis 0 (a power of two long), adjacent pairs first"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        while x.shape[0] > 1:
            x = x[0::2] + x[1::2]
    assert x.dtype == np.float32
    return x[0]


def squares(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        return x * x


def tile_partial(tile):
    """(256,) or (256, m) float32 -> the tile partial (of every column)"""
    tile = np.asarray(tile, dtype=np.float32)
    assert tile.shape[0] == TILE
    return tree(squares(tile))


def tile_partials(block):
    """(blk,) float32, blk a multiple of 256 -> (blk / 256,) float32"""
    block = np.asarray(block, dtype=np.float32)
    assert block.ndim == 1 and block.size % TILE == 0
    return tile_partial(block.reshape(-1, TILE).T)


def launch_sum(partials):
    """(L,) float32, any L >= 0 -> R of the launch"""
    s = np.asarray(partials, dtype=np.float32)
    rows = -(-s.size // LANES)
    padded = np.zeros(max(rows, 1) * LANES, dtype=np.float32)   # +0.0f: x + 0 = x for every x but -0, and a sum of squares is never -0
    padded[:s.size] = s
    a = np.zeros(LANES, dtype=np.float32)
    with np.errstate(all="ignore"):
        for row in padded.reshape(-1, LANES):
            a = a + row
    return tree(a)


def rank_partials(blocks, b):
    """rank b's tile partials in list order: bucket ascending, tile ascending inside block b"""
    parts = [tile_partials(v[b]) for v in blocks]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


def expect_norm_sq(blocks, partial=tile_partials, combine=launch_sum):
    """blocks: a list of (P, blk_i) float32 -> (P,) float32"""
    total = blocks[0].shape[0]
    out = np.zeros(total, dtype=np.float32)
    with np.errstate(all="ignore"):
        for b in range(total):
            acc = None
            for k in range(0, len(blocks), GROUP_MAX):
                r = combine(np.concatenate([partial(v[b]) for v in blocks[k:k + GROUP_MAX]]))
                acc = r if acc is None else np.float32(acc + r)
            out[b] = acc
    return out


# ---------------------------------------------------------------- what it must NOT be
def tile_partials_sequential(block):
    """the squares of a tile added left to right"""
    sq = squares(np.asarray(block, dtype=np.float32).reshape(-1, TILE))
    acc = np.zeros(sq.shape[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(TILE):
            acc = acc + sq[:, j]
    return acc


def tile_partials_fma(block):
    """a lane's four elements as an fma chain — fma(x3, x3, fma(x2, x2, fma(x1, x1, x0 x0))) — then the
    tree over the 64 lanes: float64 holds a float32 square exactly, and the sum of such a square and a
    float32 is rounded ONCE to float32 here — double rounding apart, which these data do not hit often
    enough to matter for a test that only needs SOME difference"""
    x = np.asarray(block, dtype=np.float32).reshape(-1, 64, 4).astype(np.float64)
    with np.errstate(all="ignore"):
        acc = (x[:, :, 0] * x[:, :, 0]).astype(np.float32)
        for j in range(1, 4):
            acc = (x[:, :, j] * x[:, :, j] + acc.astype(np.float64)).astype(np.float32)
    return tree(acc.T)


def tile_partials_c_first(block):
    """the lane's four, then the c levels (lanes (q, c): element group 2 c + q), then q last"""
    sq = squares(np.asarray(block, dtype=np.float32).reshape(-1, 32, 2, 4))   # [tile, c, q, e]
    with np.errstate(all="ignore"):
        lane = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])          # [tile, c, q]
        per_q = tree(np.moveaxis(lane, 1, 0))                                  # over c -> [tile, q]
        return per_q[:, 0] + per_q[:, 1]


def launch_sum_sequential(partials):
    acc = np.float32(0)
    with np.errstate(all="ignore"):
        for p in np.asarray(partials, dtype=np.float32):
            acc = np.float32(acc + p)
    return acc
