// tile_span.hpp — the tile index arithmetic of the persistent passes, made on
// the host once per launch and passed to the kernel by value.
//
// A launch covers tiles t0 .. t0 + ntiles - 1 on a grid of G workgroups;
// workgroup g takes tiles t0 + g + j * G, j = 0 .. mine - 1.  A kernel needs
// `mine` before its first load and, where the tree order or the owner depends
// on it, the block (tile / tiles-per-block) of every tile.  Both are quotients
// of launch parameters, so the host divides and the device adds:
//   mine  = ntiles / G + (g < ntiles % G)
//   block = (t0 + g) / tpb at j = 0 (a multiply by the host's reciprocal and
//           one correction), then per iteration + G / tpb, with G % tpb added
//           to the tile's index inside its block and one conditional carry.
// Tile indices are 32-bit: t0 + ntiles <= 2^31 - 1 (tile_span_make refuses
// more; 2^31 tiles of 512 bytes are a terabyte per rank).  No 64-bit division
// on the device.  Plain C++: kernels.hip includes it under hipcc, the CPU test
// (tests/test_tile_span.py) under g++.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TSA_HD __host__ __device__
#else
#define TSA_HD
#endif

namespace tsa {

struct TileSpan {
    uint32_t t0;         // first tile of the launch
    uint32_t G;          // workgroups of the launch
    uint32_t q, r;       // ntiles / G, ntiles % G
    uint32_t tpb;        // tiles per block; one block (tpb 0 asked): 2^31, above every tile index
    uint32_t gq, gr;     // G / tpb, G % tpb
    uint32_t rcp;        // min(floor(2^32 / tpb), 2^32 - 1)
};

// the block of a tile and the tile's index inside that block
struct TileBlock {
    uint32_t block, rem;
};

constexpr uint32_t kTileSpanOneBlock = 0x80000000u;
constexpr uint64_t kTileSpanMaxTiles = 0x7fffffffull;   // t0 + ntiles may not exceed this

// false: the range does not fit (or G == 0); *s is then untouched.
// tpb == 0 (or a block longer than every tile index): one block, block 0.
inline bool tile_span_make(TileSpan* s, uint64_t t0, uint64_t ntiles, uint64_t G, uint64_t tpb) {
    if (G == 0 || G > kTileSpanMaxTiles || t0 > kTileSpanMaxTiles || ntiles > kTileSpanMaxTiles - t0) return false;
    const uint32_t d = tpb == 0 || tpb >= kTileSpanOneBlock ? kTileSpanOneBlock : (uint32_t)tpb;
    const uint64_t rcp = (1ull << 32) / d;
    s->t0 = (uint32_t)t0;
    s->G = (uint32_t)G;
    s->q = (uint32_t)(ntiles / G);
    s->r = (uint32_t)(ntiles % G);
    s->tpb = d;
    s->gq = (uint32_t)G / d;
    s->gr = (uint32_t)G % d;
    s->rcp = rcp > 0xffffffffull ? 0xffffffffu : (uint32_t)rcp;
    return true;
}

// tiles of workgroup g
TSA_HD inline uint32_t tile_span_mine(const TileSpan& s, uint32_t g) { return s.q + (g < s.r ? 1u : 0u); }

// tile j of workgroup g (meaningful for j < mine; wraps harmlessly beyond)
TSA_HD inline uint32_t tile_span_tile(const TileSpan& s, uint32_t g, uint32_t j) { return s.t0 + g + j * s.G; }

// block of tile x < 2^31.  x * rcp / 2^32 is x / tpb or one less: rcp * tpb is within tpb
// of 2^32 from below, so the estimate is short by less than x / 2^32 + 1 < 1.5.
TSA_HD inline TileBlock tile_span_block(const TileSpan& s, uint32_t x) {
    uint32_t b = (uint32_t)(((uint64_t)x * s.rcp) >> 32);
    uint32_t rem = x - b * s.tpb;
    if (rem >= s.tpb) {
        rem -= s.tpb;
        ++b;
    }
    return TileBlock{b, rem};
}

// block of workgroup g's first tile
TSA_HD inline TileBlock tile_span_first(const TileSpan& s, uint32_t g) { return tile_span_block(s, s.t0 + g); }

// from tile j to tile j + 1 of the same workgroup (G tiles on)
TSA_HD inline void tile_span_next(const TileSpan& s, TileBlock& b) {
    b.block += s.gq;
    b.rem += s.gr;   // < 2 tpb <= 2^32
    if (b.rem >= s.tpb) {
        b.rem -= s.tpb;
        ++b.block;
    }
}

}  // namespace tsa
