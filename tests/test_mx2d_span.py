"""csrc/mx2d_span.hpp against brute force, on the CPU.

A stand-alone C++ program (its own main) is compiled with g++ under AddressSanitizer and UBSan.  For every
shape it walks every work unit (block, rem) of a bucket the way k_ag_group_mxfp8_2d does and compares the five
offsets mx2d_unit_at gives — shard, row-wise bytes, row-wise scales, t bytes, t scales — with an enumeration of
the patches in order (block, row group, column group) computed in 128 bits from the matrix coordinates.  At the
four small shapes (P, cols, R) = (8, 32, 32), (8, 96, 64), (64, 32, 32), (16, 160, 32), and at (8, 64, 64) and
(8, 128, 32) where the patch is wider than a square, every byte the patches cover is counted: every element byte,
every scale byte of both orientations and every shard float exactly once, none outside.  The same count is taken
at every (P, cols, R) a GPU test runs (tests/mx2d_cases.py), the shapes of several row groups per shard block among
them, and what the header makes of each shape — lgh, lgw, cgs, units — is printed and compared with
mx2d_cases.shape_class, the restatement the census of tests/test_mx2d_classes.py rests on.  One shape has
cols * nrows and r * t_row_stride beyond 2^32: its units are sampled."""
import os
import re
import shutil
import subprocess

import mx2d_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mx2d_span.hpp"

typedef unsigned __int128 u128;
static unsigned long long g_units = 0;

static void fail(const char* what, uint64_t cols, uint64_t nrows, uint64_t block, uint64_t rem, uint64_t got, u128 want) {
    std::printf("MISMATCH %s: cols=%llu nrows=%llu block=%llu rem=%llu got=%llu want=%llu\n", what, (unsigned long long)cols,
                (unsigned long long)nrows, (unsigned long long)block, (unsigned long long)rem, (unsigned long long)got,
                (unsigned long long)want);
    std::exit(1);
}

static uint32_t lg2(uint64_t P) {
    uint32_t k = 0;
    while ((1ull << k) < P) ++k;
    return k;
}

// unit (block, rem) against the matrix coordinates of its patch
static void check_unit(const tsa::Mx2dShape& s, uint64_t P, uint64_t shard_stride, uint64_t block, uint64_t rem) {
    const uint64_t cols = s.cols, nrows = s.nrows, R = nrows / P;
    const uint64_t H = 32ull << s.lgh, Wd = 32ull << s.lgw, cgs = cols / Wd;
    const uint64_t rg = rem / cgs, cg = rem % cgs;
    const u128 i0 = (u128)block * R + (u128)rg * H, j0 = (u128)cg * Wd;
    const tsa::Mx2dUnit u = tsa::mx2d_unit_at(s, (uint32_t)block, (uint32_t)rem, shard_stride, lg2(P));
    const u128 src = (u128)block * shard_stride + (u128)rg * H * cols + j0, row = i0 * cols + j0, t = j0 * nrows + i0;
    if ((u128)u.src != src) fail("src", cols, nrows, block, rem, u.src, src);
    if ((u128)u.row != row) fail("row", cols, nrows, block, rem, u.row, row);
    if ((u128)u.rscale != row / 32) fail("rscale", cols, nrows, block, rem, u.rscale, row / 32);
    if ((u128)u.t != t) fail("t", cols, nrows, block, rem, u.t, t);
    if ((u128)u.tscale != t / 32) fail("tscale", cols, nrows, block, rem, u.tscale, t / 32);
    ++g_units;
}

static void small(uint64_t P, uint64_t cols, uint64_t R, uint64_t gap) {
    const uint64_t nrows = P * R, n = nrows * cols, blk = R * cols, stride = blk + gap;
    tsa::Mx2dShape s;
    uint64_t units, all;
    if (!tsa::mx2d_shape_make(&s, cols, nrows, P, &units, &all)) fail("make", cols, nrows, 0, 0, 0, 1);
    const uint64_t H = 32ull << s.lgh, Wd = 32ull << s.lgw;
    if (cols % Wd || R % H || units != (cols / Wd) * (R / H) || all != units * P || s.cgs != cols / Wd)
        fail("shape", cols, nrows, 0, 0, units, (cols / Wd) * (R / H));
    std::printf("shape %llu %llu %llu: %u %u %u %llu\n", (unsigned long long)P, (unsigned long long)cols, (unsigned long long)R, s.lgh,
                s.lgw, s.cgs, (unsigned long long)units);
    if ((int)s.lgh > tsa::kMx2dLgSide || (int)s.lgw > tsa::kMx2dLgSide) fail("side", cols, nrows, 0, 0, s.lgh, s.lgw);
    // the widest patch the divisibility allows, up to the cap
    if ((int)s.lgw < tsa::kMx2dLgSide && (cols / Wd) % 2 == 0) fail("lgw", cols, nrows, 0, 0, s.lgw, 0);
    if ((int)s.lgh < tsa::kMx2dLgSide && (R / H) % 2 == 0) fail("lgh", cols, nrows, 0, 0, s.lgh, 0);
    std::vector<uint8_t> row(n, 0), t(n, 0), rs(n / 32, 0), ts(n / 32, 0), src(P * stride, 0);
    for (uint64_t b = 0; b < P; ++b)
        for (uint64_t rem = 0; rem < units; ++rem) {
            check_unit(s, P, stride, b, rem);
            const tsa::Mx2dUnit u = tsa::mx2d_unit_at(s, (uint32_t)b, (uint32_t)rem, stride, lg2(P));
            for (uint64_t i = 0; i < H; ++i)
                for (uint64_t j = 0; j < Wd; ++j) {
                    ++row.at(u.row + i * cols + j);
                    ++t.at(u.t + j * nrows + i);
                    ++src.at(u.src + i * cols + j);
                }
            for (uint64_t i = 0; i < H; ++i)
                for (uint64_t k = 0; k < Wd / 32; ++k) ++rs.at(u.rscale + i * (cols / 32) + k);
            for (uint64_t j = 0; j < Wd; ++j)
                for (uint64_t k = 0; k < H / 32; ++k) ++ts.at(u.tscale + j * (nrows / 32) + k);
        }
    for (uint64_t x = 0; x < n; ++x)
        if (row[x] != 1 || t[x] != 1) fail("element coverage", cols, nrows, 0, x, row[x], t[x]);
    for (uint64_t x = 0; x < n / 32; ++x)
        if (rs[x] != 1 || ts[x] != 1) fail("scale coverage", cols, nrows, 0, x, rs[x], ts[x]);
    for (uint64_t x = 0; x < P * stride; ++x)
        if (src[x] != (x % stride < blk ? 1 : 0)) fail("shard coverage", cols, nrows, 0, x, src[x], x % stride < blk);
}

int main() {
    small(8, 32, 32, 0);
    small(8, 96, 64, 64);
    small(64, 32, 32, 0);
    small(16, 160, 32, 4);
    small(8, 64, 64, 0);
    small(8, 128, 32, 8);
    small(8, 256, 128, 0);
    // every (P, cols, R) of the GPU tests' lists (tests/mx2d_cases.py), several row groups per block among them
@TABLE@
    // cols * nrows = 2^33 + ..., the last rank's t row beyond 2^32 bytes
    {
        const uint64_t P = 8, cols = 96 * 1024 + 32, R = 1u << 14, nrows = P * R, stride = R * cols + 4096;
        tsa::Mx2dShape s;
        uint64_t units, all;
        if (!tsa::mx2d_shape_make(&s, cols, nrows, P, &units, &all)) fail("make", cols, nrows, 0, 0, 0, 1);
        if (cols * nrows <= (1ull << 32)) fail("big", cols, nrows, 0, 0, 0, 0);
        uint64_t x = 12345;
        for (int k = 0; k < 200000; ++k) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            check_unit(s, P, stride, (x >> 33) % P, (x >> 20) % units);
        }
        for (uint64_t b = 0; b < P; ++b) {
            check_unit(s, P, stride, b, 0);
            check_unit(s, P, stride, b, units - 1);
        }
        const tsa::Mx2dUnit u = tsa::mx2d_unit_at(s, (uint32_t)(P - 1), (uint32_t)(units - 1), stride, lg2(P));
        const uint64_t t_row_stride = cols * nrows + 16 * 17, r = P - 1;
        if (r * t_row_stride <= (1ull << 32) || (u128)(r * t_row_stride + u.t) != (u128)r * t_row_stride + (u128)u.t || u.t <= (1ull << 32))
            fail("far", cols, nrows, P - 1, units - 1, u.t, 0);
    }
    // refusals: not whole squares, too many units
    {
        tsa::Mx2dShape s;
        uint64_t units, all;
        if (tsa::mx2d_shape_make(&s, 48, 256, 8, &units, &all) || tsa::mx2d_shape_make(&s, 32, 128, 8, &units, &all) ||
            tsa::mx2d_shape_make(&s, 0, 256, 8, &units, &all) || tsa::mx2d_shape_make(&s, 32ull << 20, 256ull << 20, 8, &units, &all))
            fail("refusal", 0, 0, 0, 0, 0, 0);
    }
    std::printf("mx2d_span ok: %llu units checked\n", g_units);
    return 0;
}
"""


LITERAL = ((8, 32, 32), (8, 96, 64), (64, 32, 32), (16, 160, 32), (8, 64, 64), (8, 128, 32), (8, 256, 128))   # main's own small() calls
GAPS = (0, 64, 4, 8)   # floats between the shard blocks, in turn


def table():
    """(P, cols, R) of every shape a GPU test runs, each once: the shape tests' lists at their rank counts, the soak's at all"""
    lists = [((p,), mc.gpu_shapes(p)) for p in mc.SOAK_RANKS] + [(mc.SOAK_RANKS, mc.SOAK_SHAPES)]
    return list(dict.fromkeys((p, cols, R) for ranks, shapes in lists for p in ranks for cols, R in shapes))


def test_mx2d_span_matches_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the mx2d_span check"
    src = tmp_path / "mx2d_span_check.cpp"
    calls = [f"    small({p}, {cols}, {R}, {GAPS[i % 4]});" for i, (p, cols, R) in enumerate(table())]
    assert all((p, *s) in table() for p in mc.GPU_RANKS for s in mc.ROW_GROUP_SHAPES) and all((64, *s) in table() for s in mc.ROW_GROUP_SHAPES_64)
    src.write_text(PROGRAM.replace("@TABLE@", "\n".join(calls)))
    exe = tmp_path / "mx2d_span_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mx2d_span ok" in run.stdout
    # what the C++ made of every shape it walked, against mx2d_cases.shape_class
    lg = int(re.search(r"#define TSA_MX2D_LG_SIDE (\d+)", open(os.path.join(CSRC, "mx2d_span.hpp")).read()).group(1))
    printed = {}
    for m in re.finditer(r"^shape (\d+) (\d+) (\d+): (\d+) (\d+) (\d+) (\d+)$", run.stdout, re.M):
        p, cols, R, lgh, lgw, cgs, units = map(int, m.groups())
        printed[p, cols, R] = (lgh, lgw, cgs, units)
    assert set(printed) == set(LITERAL) | set(table()), sorted(set(printed) ^ (set(LITERAL) | set(table())))
    for (p, cols, R), got in printed.items():
        lgh, lgw, rgs, cgs = mc.shape_class(cols, R, lg)
        assert got == (lgh, lgw, cgs, rgs * cgs), f"P={p} cols={cols} R={R}: the header says (lgh, lgw, cgs, units) = {got}"
