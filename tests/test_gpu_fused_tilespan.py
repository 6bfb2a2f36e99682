"""The persistent fused passes whose tile index arithmetic comes from csrc/tile_span.hpp,
against the CPU oracle, bit for bit (0 differing elements).

64 ranks, 8x8 Swing, EXEC_FUSED, rows at preferred_rank_stride (a sentinel in the stride
skew and one guard row behind the last rank must keep their bits).  The shapes are the
smallest that reach these kernels (>= 1024 whole tiles of 256 elements) and walk the
helper's paths:
  1024 tiles (16 per block)   every workgroup takes exactly 2 tiles, ntiles % G == 0
  1088 tiles (17 per block)   odd tiles per block; 64 workgroups take 3 tiles
  1280 tiles, pipe_grid=96    13-14 tiles per workgroup, G / tpb = 4 remainder 16: many carries
  1280 tiles, pipe_grid=7     G < tiles per block: the block often does not advance
  2176 tiles, fused_chunk_tiles=725   three launches whose first tile falls inside a block
Variants: BO -> k_tree_lds_lag, MEM -> k_mem_lds_lag, LO -> k_lo_dag_reg (its `mine` only);
Plan.reduce_scatter, in place and to a compact buffer, at 1088 tiles -> k_tree_lds_pipe<64, false>.
"""
import functools

import numpy as np
import pytest

import oracle
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5A5
SIDE, TOTAL = 8, 64

SHAPES = [(1024, {}), (1088, {}), (1280, {"pipe_grid": 96}), (1280, {"pipe_grid": 7}), (2176, {"fused_chunk_tiles": 725})]
SHAPE_IDS = ["1024", "1088", "1280-grid96", "1280-grid7", "2176-chunk725"]
VARIANTS = [("bo", t.BO), ("mem", t.MEM), ("lo", t.LO)]


@functools.lru_cache(maxsize=None)
def inputs(tiles):
    data = np.random.default_rng(4000 + tiles).integers(0x3F80, 0x42C8, (TOTAL, tiles * 256)).astype(np.uint16)
    data.flags.writeable = False
    return data


@functools.lru_cache(maxsize=None)
def reference(name, tiles):
    """the oracle's allreduce of inputs(tiles), (TOTAL, n) uint16: computed once, read-only"""
    want = [r.copy() for r in inputs(tiles)]
    oracle.allreduce(name, t.SWING, SIDE, want, TOTAL)
    want = np.stack(want)
    want.flags.writeable = False
    return want


def rows(data):
    total, n = data.shape
    stride = t.preferred_rank_stride(n)
    host = np.full((total + 1, stride), SENT, dtype=np.uint16)
    host[:total, :n] = data
    return host, torch.from_numpy(host.view(np.int16)).to(DEV), stride


def from_dev(buf):
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("name,variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("tiles,keys", SHAPES, ids=SHAPE_IDS)
def test_fused_allreduce_is_the_oracle(tiles, keys, name, variant):
    n = tiles * 256
    want = reference(name, tiles)
    host, buf, stride = rows(inputs(tiles))
    plan = t.Plan(t.SWING, variant, SIDE, n, TOTAL, t.EXEC_FUSED)
    with t.tuned(**keys):
        plan.execute(buf.data_ptr(), stride, None, torch.cuda.current_stream())
        if variant == t.BO:
            launch = t.last_launch()
            assert launch["kernel"] == "k_tree_lds_lag<64>"
            assert launch["grid"] == keys.get("pipe_grid", 512)
    got = from_dev(buf)
    plan.close()
    differing = int((got[:TOTAL, :n] != want).sum())
    print(f"{name} {tiles} tiles {keys}: {differing} differing elements")
    assert differing == 0
    assert (got[:TOTAL, n:] == SENT).all() and (got[TOTAL] == SENT).all()


@pytest.mark.parametrize("compact", [False, True], ids=["in-place", "compact"])
def test_reduce_scatter_is_the_oracle(compact):
    tiles = 1088
    n, blk = tiles * 256, tiles * 256 // TOTAL
    want = reference("bo", tiles)
    want_blocks = np.stack([want[b, b * blk:(b + 1) * blk] for b in range(TOTAL)])
    host, buf, stride = rows(inputs(tiles))
    out = torch.from_numpy(np.full((TOTAL + 1, blk), SENT, dtype=np.uint16).view(np.int16)).to(DEV)
    plan = t.Plan(t.SWING, t.BO, SIDE, n, TOTAL, t.EXEC_FUSED)
    if compact:
        plan.reduce_scatter(buf.data_ptr(), stride, out.data_ptr(), blk, stream=torch.cuda.current_stream())
    else:
        plan.reduce_scatter(buf.data_ptr(), stride, stream=torch.cuda.current_stream())
    got, got_out = from_dev(buf), from_dev(out)
    plan.close()
    expect = host.copy()
    if compact:
        differing = int((got_out[:TOTAL] != want_blocks).sum())
        assert (got_out[TOTAL] == SENT).all()
    else:
        for b in range(TOTAL):
            expect[b, b * blk:(b + 1) * blk] = want_blocks[b]
        differing = int((np.stack([got[b, b * blk:(b + 1) * blk] for b in range(TOTAL)]) != want_blocks).sum())
    print(f"reduce-scatter {'compact' if compact else 'in place'}: {differing} differing elements")
    assert differing == 0
    assert np.array_equal(got, expect)   # everything else keeps its input bits
