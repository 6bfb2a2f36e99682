"""csrc/group_span.hpp against brute force, on the CPU.

A stand-alone C++ program (its own main) is compiled with g++ under AddressSanitizer and
UBSan.  For every bucket list and grid it walks every workgroup g and iteration j the way
k_tree_group does — one cursor per workgroup, carried from tile to tile — and compares with
    mine   = g < T ? (T - 1 - g) / G + 1 : 0
    x      = g + j * G
    bucket = the i with first_i <= x < first_i + tiles_i   (a search from bucket 0)
    local  = x - first_i,  block = local / tpb_i,  index in block = local % tpb_i
computed in uint64_t.  Lists: random ones of 1 .. 64 buckets with 1 .. 20 tiles per block
(3, 5 and 7 among them) at 8 .. 64 ranks; buckets shorter than the grid, so a stride passes
whole buckets; grids wider than the tile range; 64 one-tile-per-block buckets; the sum of
the tiles at and past 2^31 - 1.
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
#include <vector>

#include "group_span.hpp"

static unsigned long long g_checked = 0, g_skips = 0;

struct Rng {   // a fixed 64-bit LCG: the same lists on every run
    uint64_t s;
    uint32_t next(uint32_t n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((s >> 33) % n);
    }
};

static void fail(const char* what, int count, uint64_t G, uint64_t g, uint64_t j, uint64_t got, uint64_t want) {
    std::printf("MISMATCH %s: count=%d G=%llu g=%llu j=%llu got=%llu want=%llu\n", what, count,
                (unsigned long long)G, (unsigned long long)g, (unsigned long long)j, (unsigned long long)got,
                (unsigned long long)want);
    std::exit(1);
}

// every workgroup g in [g_lo, g_hi) and every iteration of the launch
static void check(const std::vector<tsa::GroupIn>& in, uint64_t G, uint64_t g_lo, uint64_t g_hi) {
    const int count = (int)in.size();
    tsa::GroupSpan s;
    if (!tsa::group_span_make(&s, in.data(), count, G)) fail("make", count, G, 0, 0, 0, 1);
    std::vector<uint64_t> first(in.size() + 1, 0);
    for (int i = 0; i < count; ++i) first[i + 1] = first[i] + in[i].tiles;
    const uint64_t T = first[count];
    if (s.T != T || s.G != G) fail("T / G", count, G, 0, 0, s.T, T);
    for (int i = 0; i < count; ++i) {
        if (s.b[i].ranks != in[i].ranks || s.b[i].stride != in[i].stride) fail("entry", count, G, i, 0, 0, 1);
        if (s.b[i].first != first[i] || s.b[i].end != first[i + 1]) fail("range", count, G, i, 0, s.b[i].first, first[i]);
    }
    for (int i = count; i < tsa::kGroupMax; ++i)
        if (s.b[i].ranks || s.b[i].stride || s.b[i].end || s.b[i].tpb) fail("tail not zero", count, G, i, 0, 1, 0);
    for (uint64_t g = g_lo; g < g_hi; ++g) {
        const uint64_t mine = g < T ? (T - 1 - g) / G + 1 : 0;
        if (tsa::group_span_mine(s, (uint32_t)g) != mine)
            fail("mine", count, G, g, 0, tsa::group_span_mine(s, (uint32_t)g), mine);
        uint32_t cursor = 0;
        uint64_t prev_bucket = 0;
        for (uint64_t j = 0; j < mine; ++j) {
            const uint64_t x = g + j * G;
            if (tsa::group_span_tile(s, (uint32_t)g, (uint32_t)j) != x)
                fail("tile", count, G, g, j, tsa::group_span_tile(s, (uint32_t)g, (uint32_t)j), x);
            uint64_t i = 0;
            while (x >= first[i + 1]) ++i;
            const uint64_t local = x - first[i];
            const tsa::GroupTile t = tsa::group_span_at(s, (uint32_t)x, cursor);
            if (t.bucket != i || cursor != i) fail("bucket", count, G, g, j, t.bucket, i);
            if (t.local != local) fail("local", count, G, g, j, t.local, local);
            if (t.block != local / in[i].tpb) fail("block", count, G, g, j, t.block, local / in[i].tpb);
            if (t.rem != local % in[i].tpb) fail("index in block", count, G, g, j, t.rem, local % in[i].tpb);
            if (j && i > prev_bucket + 1) ++g_skips;   // whole buckets passed in one stride
            prev_bucket = i;
            ++g_checked;
        }
    }
}

static tsa::GroupIn bucket(int i, uint64_t tpb, uint64_t ranks) {
    // distinct made-up row pointers and strides: the table must carry them through unchanged
    return tsa::GroupIn{reinterpret_cast<uint16_t*>((uintptr_t)0x1000 * (uintptr_t)(i + 1)), 256 * tpb * ranks + 64 * (uint64_t)i,
                        tpb * ranks, tpb};
}

static void check_all_grids(const std::vector<tsa::GroupIn>& in) {
    uint64_t T = 0;
    for (const tsa::GroupIn& b : in) T += b.tiles;
    const uint64_t grids[] = {1, 2, 5, 24, T / 2 ? T / 2 : 1, T - 1 ? T - 1 : 1, T, T + 3, 512};
    for (uint64_t G : grids) check(in, G, 0, G);   // g >= T included where G > T: mine == 0
}

int main() {
    Rng rng{20240607};
    const uint64_t tpbs[] = {1, 2, 3, 5, 7, 10, 20};
    const uint64_t ranks[] = {8, 16, 32, 64};
    // random lists, 1 .. 64 buckets
    for (int rep = 0; rep < 60; ++rep) {
        const int count = rep < 4 ? 64 : 1 + (int)rng.next(64);
        std::vector<tsa::GroupIn> in;
        const uint64_t P = ranks[rng.next(4)];
        for (int i = 0; i < count; ++i) in.push_back(bucket(i, tpbs[rng.next(7)], P));
        check_all_grids(in);
    }
    // the lists of tests/test_gpu_group.py: unequal buckets at 8 and 64 ranks, 64 one-tile-per-block buckets
    for (uint64_t P : ranks) {
        std::vector<tsa::GroupIn> in = {bucket(0, 1, P), bucket(1, 3, P), bucket(2, 2, P), bucket(3, 5, P)};
        check_all_grids(in);
    }
    {
        std::vector<tsa::GroupIn> in;
        for (int i = 0; i < 64; ++i) in.push_back(bucket(i, 1, 8));
        check_all_grids(in);
    }
    if (g_skips == 0) {
        std::printf("MISMATCH no stride passed a whole bucket: the lists do not reach that path\n");
        return 1;
    }
    // the sum of the tiles at 2^31 - 1: accepted, first and last workgroups walked
    const uint64_t top = 0x7fffffffull;
    {
        std::vector<tsa::GroupIn> in = {tsa::GroupIn{nullptr, 0, 1ull << 30, 1ull << 24}, tsa::GroupIn{nullptr, 0, 5, 5},
                                        tsa::GroupIn{nullptr, 0, (1ull << 30) - 6, 61}};
        check(in, 512, 0, 1);
        check(in, 512, 511, 512);
    }
    // refused: past 2^31 - 1, no or too many buckets, an empty bucket, no block length, no workgroups
    tsa::GroupSpan s;
    s.T = 77;
    const tsa::GroupIn big[2] = {{nullptr, 0, 1ull << 30, 1}, {nullptr, 0, 1ull << 30, 1}};
    const tsa::GroupIn one_too_many[2] = {{nullptr, 0, top, 1}, {nullptr, 0, 1, 1}};
    const tsa::GroupIn empty[1] = {{nullptr, 0, 0, 1}};
    const tsa::GroupIn no_tpb[1] = {{nullptr, 0, 8, 0}};
    std::vector<tsa::GroupIn> many(65, tsa::GroupIn{nullptr, 0, 8, 1});
    if (tsa::group_span_make(&s, big, 2, 512) || tsa::group_span_make(&s, one_too_many, 2, 512) ||
        tsa::group_span_make(&s, empty, 1, 512) || tsa::group_span_make(&s, no_tpb, 1, 512) ||
        tsa::group_span_make(&s, many.data(), 65, 512) || tsa::group_span_make(&s, many.data(), 0, 512) ||
        tsa::group_span_make(&s, many.data(), 64, 0) || s.T != 77) {
        std::printf("MISMATCH make accepted (or wrote) a list it must refuse\n");
        return 1;
    }
    if (!tsa::group_span_make(&s, one_too_many, 1, 512) || !tsa::group_span_make(&s, many.data(), 64, 512)) {
        std::printf("MISMATCH make refused 2^31 - 1 tiles or 64 buckets\n");
        return 1;
    }
    std::printf("group_span ok: %llu tiles checked, %llu strides over whole buckets\n", g_checked, g_skips);
    return 0;
}
"""


LAYOUT = r"""
#include <cstddef>
#include <cstdio>
#include "allred.h"
#include "group_span.hpp"
int main() {
    std::printf("%zu %zu %zu %zu %d %d\n", sizeof(allred_bucket), offsetof(allred_bucket, ranks),
                offsetof(allred_bucket, rank_stride), offsetof(allred_bucket, elems_per_rank), ALLRED_GROUP_MAX,
                tsa::kGroupMax);
    return 0;
}
"""


def test_bucket_binding_matches_the_header(tmp_path):
    """_lib.Bucket mirrors allred_bucket, and the three constants for 64 buckets per launch agree."""
    import ctypes as C

    from tenstorrentallreduce_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    b = _lib.Bucket
    assert out == [C.sizeof(b), b.ranks.offset, b.rank_stride.offset, b.elems_per_rank.offset, _lib.GROUP_MAX,
                   _lib.GROUP_MAX]


def test_group_span_matches_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the group_span check"
    src = tmp_path / "group_span_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "group_span_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "group_span ok" in run.stdout
