"""csrc/mx4_2d_span.hpp against brute force, on the CPU, in both strip builds (S = 4 and S = 8).

A stand-alone C++ program (its own main) is compiled with g++ under AddressSanitizer and UBSan.  For every shape
it walks every work unit (strip, column group) the way k_ag_group_mxfp4_2d does, compares the offsets
mx4_2d_unit_at gives with the matrix coordinates in 128 bits and the shard block of every row group with
G / (R / 32), and counts what the kernel's loads and stores address from them: every byte of the four rank rows
and every shard float exactly once, none outside (std::vector::at), gaps between the shard blocks untouched."""
import os
import shutil
import subprocess

import pytest

import mx4_2d_ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tenstorrentallreduce_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mx4_2d_span.hpp"

typedef unsigned __int128 u128;

static void fail(const char* what, uint64_t P, uint64_t cols, uint64_t R, uint64_t a, uint64_t b) {
    std::printf("MISMATCH %s: P=%llu cols=%llu R=%llu at %llu: %llu\n", what, (unsigned long long)P, (unsigned long long)cols,
                (unsigned long long)R, (unsigned long long)a, (unsigned long long)b);
    std::exit(1);
}

static void shape(uint64_t P, uint64_t cols, uint64_t R, uint64_t gap) {
    const uint64_t S = 1ull << tsa::kMx4LgStrip, nrows = P * R, n = nrows * cols, blk = R * cols, stride = blk + gap;
    tsa::Mx4Shape s;
    uint64_t cgs, all;
    if (!tsa::mx4_2d_shape_make(&s, cols, nrows, P, &cgs, &all)) fail("make", P, cols, R, 0, 0);
    const uint64_t sw = 1ull << s.lgw, strips = nrows / (32 * S);
    if ((int)s.lgw > tsa::kMx4LgWidth || (cols / 32) % sw || cgs != cols / (32 * sw) || all != cgs * strips || s.rpb != R / 32)
        fail("shape", P, cols, R, cgs, all);
    if ((int)s.lgw < tsa::kMx4LgWidth && (cols / 32 / sw) % 2 == 0) fail("the widest strip", P, cols, R, s.lgw, 0);
    std::vector<uint8_t> row(n / 2, 0), t(n / 2, 0), rs(n / 32, 0), ts(n / 32, 0), src(P * stride, 0);
    for (uint64_t strip = 0; strip < strips; ++strip)
        for (uint64_t cg = 0; cg < cgs; ++cg) {
            const tsa::Mx4Unit u = tsa::mx4_2d_unit_at(s, (uint32_t)strip, (uint32_t)cg);
            const u128 i0 = (u128)strip * 32 * S, j0 = (u128)cg * 32 * sw;
            if (u.g0 != strip * S || (u128)u.j0 != j0) fail("g0 / j0", P, cols, R, strip, cg);
            if ((u128)u.row != (i0 * cols + j0) / 2 || (u128)u.rscale != (i0 * cols + j0) / 32) fail("row", P, cols, R, strip, cg);
            if ((u128)u.t != (j0 * nrows + i0) / 2 || (u128)u.tscale != (j0 * nrows + i0) / 32) fail("t", P, cols, R, strip, cg);
            for (uint64_t q = 0; q < S * sw; ++q) {   // the loads, square by square
                const uint64_t G = u.g0 + (q >> s.lgw), qj = q & (sw - 1);
                const tsa::Mx4Group g = tsa::mx4_2d_group_at(s, (uint32_t)G, stride);
                if (g.block != G / (R / 32)) fail("the shard block of a row group", P, cols, R, G, g.block);
                for (uint64_t r = 0; r < 32; ++r)
                    for (uint64_t c = 0; c < 32; ++c) ++src.at(g.src + r * cols + u.j0 + 32 * qj + c);
            }
            for (uint64_t i = 0; i < 32 * S; ++i) {   // the stores: a row's 16 sw bytes and sw scale bytes
                for (uint64_t b = 0; b < 16 * sw; ++b) ++row.at(u.row + i * (cols / 2) + b);
                for (uint64_t b = 0; b < sw; ++b) ++rs.at(u.rscale + i * (cols / 32) + b);
            }
            for (uint64_t j = 0; j < 32 * sw; ++j) {  // a column's 16 S bytes and S scale bytes
                for (uint64_t b = 0; b < 16 * S; ++b) ++t.at(u.t + j * (nrows / 2) + b);
                for (uint64_t b = 0; b < S; ++b) ++ts.at(u.tscale + j * (nrows / 32) + b);
            }
        }
    for (uint64_t x = 0; x < n / 2; ++x)
        if (row[x] != 1 || t[x] != 1) fail("element coverage", P, cols, R, x, row[x] * 16 + t[x]);
    for (uint64_t x = 0; x < n / 32; ++x)
        if (rs[x] != 1 || ts[x] != 1) fail("scale coverage", P, cols, R, x, rs[x] * 16 + ts[x]);
    for (uint64_t x = 0; x < P * stride; ++x)
        if (src[x] != (x % stride < blk ? 1 : 0)) fail("shard coverage", P, cols, R, x, src[x]);
}

int main() {
@TABLE@
    tsa::Mx4Shape s;
    uint64_t cgs, all;   // refusals: not whole squares, not whole strips, too many units
    if (tsa::mx4_2d_shape_make(&s, 48, 256, 8, &cgs, &all) || tsa::mx4_2d_shape_make(&s, 32, 128, 8, &cgs, &all) ||
        tsa::mx4_2d_shape_make(&s, 0, 256, 8, &cgs, &all) || tsa::mx4_2d_shape_make(&s, 32ull << 20, 256ull << 20, 8, &cgs, &all))
        fail("refusal", 0, 0, 0, 0, 0);
    std::printf("mx4_2d_span ok\n");
    return 0;
}
"""

SHAPES = mx4_2d_ref.SHAPES + ((8, 256, 128), (64, 160, 96))
GAPS = (0, 64, 4, 8)   # floats between the shard blocks, in turn


@pytest.mark.parametrize("lg_strip", [2, 3])
def test_mx4_2d_span_matches_brute_force(tmp_path, lg_strip):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the mx4_2d_span check"
    src = tmp_path / "mx4_2d_span_check.cpp"
    src.write_text(PROGRAM.replace("@TABLE@", "\n".join(f"    shape({p}, {cols}, {R}, {GAPS[i % 4]});" for i, (p, cols, R) in enumerate(SHAPES))))
    exe = tmp_path / "mx4_2d_span_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-DTSA_MX4_2D_LG_STRIP={lg_strip}", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "mx4_2d_span ok" in run.stdout, run.stdout + run.stderr
