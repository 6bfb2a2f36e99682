"""csrc/tile_span.hpp against the plain 64-bit formulas, on the CPU.

A stand-alone C++ program (its own main) is compiled with g++ under AddressSanitizer and
UBSan and walks every workgroup and iteration of every case: the helper's `mine`, tile and
block must equal
    mine  = g < ntiles ? (ntiles - 1 - g) / G + 1 : 0
    tile  = t0 + g + j * G
    block = tpb ? tile / tpb : 0
computed in uint64_t — the expressions the kernels carried before the helper.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "tile_span.hpp"

static unsigned long long g_checked = 0;

static void fail(const char* what, uint64_t t0, uint64_t ntiles, uint64_t G, uint64_t tpb, uint64_t g, uint64_t j,
                 uint64_t got, uint64_t want) {
    std::printf("MISMATCH %s: t0=%llu ntiles=%llu G=%llu tpb=%llu g=%llu j=%llu got=%llu want=%llu\n", what,
                (unsigned long long)t0, (unsigned long long)ntiles, (unsigned long long)G, (unsigned long long)tpb,
                (unsigned long long)g, (unsigned long long)j, (unsigned long long)got, (unsigned long long)want);
    std::exit(1);
}

// every workgroup g in [g_lo, g_hi) and every iteration of the launch
static void check(uint64_t t0, uint64_t ntiles, uint64_t G, uint64_t tpb, uint64_t g_lo, uint64_t g_hi) {
    tsa::TileSpan s;
    if (!tsa::tile_span_make(&s, t0, ntiles, G, tpb)) fail("make", t0, ntiles, G, tpb, 0, 0, 0, 1);
    for (uint64_t g = g_lo; g < g_hi; ++g) {
        const uint64_t mine = g < ntiles ? (ntiles - 1 - g) / G + 1 : 0;
        if (tsa::tile_span_mine(s, (uint32_t)g) != mine)
            fail("mine", t0, ntiles, G, tpb, g, 0, tsa::tile_span_mine(s, (uint32_t)g), mine);
        tsa::TileBlock b = tsa::tile_span_first(s, (uint32_t)g);
        for (uint64_t j = 0; j < mine; ++j) {
            const uint64_t tile = t0 + g + j * G, block = tpb ? tile / tpb : 0;
            if (tsa::tile_span_tile(s, (uint32_t)g, (uint32_t)j) != tile)
                fail("tile", t0, ntiles, G, tpb, g, j, tsa::tile_span_tile(s, (uint32_t)g, (uint32_t)j), tile);
            if (b.block != block) fail("block (carried)", t0, ntiles, G, tpb, g, j, b.block, block);
            if (tpb && b.rem != tile % tpb) fail("rem (carried)", t0, ntiles, G, tpb, g, j, b.rem, tile % tpb);
            const tsa::TileBlock d = tsa::tile_span_block(s, (uint32_t)tile);
            if (d.block != block) fail("block (direct)", t0, ntiles, G, tpb, g, j, d.block, block);
            tsa::tile_span_next(s, b);
            ++g_checked;
        }
    }
}

int main() {
    const uint64_t tpbs[] = {0, 1, 2, 3, 5, 16, 17, 20, 61};
    for (uint64_t ntiles = 1; ntiles <= 70; ++ntiles)
        for (uint64_t G = 1; G <= ntiles; ++G)
            for (uint64_t tpb : tpbs) {
                const uint64_t t0s[] = {0, 1, tpb ? tpb - 1 : 0, 1301};
                for (uint64_t t0 : t0s) check(t0, ntiles, G, tpb, 0, G);
            }
    // the edge values: config 2's 1280 tiles and 3904, G = 512, the range ending at 2^31 - 1
    const uint64_t top = 0x7fffffffull;
    const uint64_t edge_tiles[] = {1280, 3904};
    for (uint64_t ntiles : edge_tiles)
        for (uint64_t tpb : tpbs) {
            const uint64_t t0s[] = {0, 1, tpb ? tpb - 1 : 0, 1301, top - ntiles};
            for (uint64_t t0 : t0s) check(t0, ntiles, 512, tpb, 0, 512);
        }
    // one launch that is the whole range (its first and last workgroups), long blocks included
    const uint64_t whole_tpbs[] = {0, 1, 20, 61, 0x2000000};
    for (uint64_t tpb : whole_tpbs) {
        check(0, top, 512, tpb, 0, 1);
        check(0, top, 512, tpb, 511, 512);
    }
    // refused: past 2^31 - 1, no workgroups
    tsa::TileSpan s;
    if (tsa::tile_span_make(&s, top - 1279, 1280, 512, 20) || tsa::tile_span_make(&s, 0, top + 1, 512, 20) ||
        tsa::tile_span_make(&s, top + 1, 0, 512, 20) || tsa::tile_span_make(&s, 0, 1280, 0, 20)) {
        std::printf("MISMATCH make accepted a range it must refuse\n");
        return 1;
    }
    if (!tsa::tile_span_make(&s, top - 1280, 1280, 512, 20)) {
        std::printf("MISMATCH make refused t0 + ntiles == 2^31 - 1\n");
        return 1;
    }
    std::printf("tile_span ok: %llu tiles checked\n", g_checked);
    return 0;
}
"""


def test_tile_span_matches_the_64_bit_formulas(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the tile_span check"
    src = tmp_path / "tile_span_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "tile_span_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "tile_span ok" in run.stdout
