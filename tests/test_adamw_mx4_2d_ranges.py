"""csrc/adamw_mx2d_ranges.hpp at per_byte = 2 — the argument and disjointness rules of
allred_plan_adamw_all_gather_shards_mxfp4_2d — on the CPU: a stand-alone C++ program (its own main) compiled with g++
under AddressSanitizer and UBSan and run directly, as tests/test_mx2d_ranges.py does.

ONE layout, addresses made up (nothing is dereferenced): 8 ranks, a 256 x 32 matrix, the param plane's 8 blocks of 1024
floats at a wide stride whose gap behind block 0 holds, one behind the other and filling it EXACTLY, the rows and the scale
rows, three hyper sets, norm_sq, info, the t rows and the t scale rows — the element rows with the HALVED payload, n / 2
bytes per rank.  Accepted at per_byte = 2.  Refused: the rows moved 16 bytes back (one quantum on block 0's tail), the t
scale rows moved 16 bytes on (onto block 1's head), and the same list at per_byte = 1, whose payload the strides do not cover."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "adamw_mx2d_ranges.hpp"

static const void* at(uint64_t a) { return reinterpret_cast<const void*>((uintptr_t)a); }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const uint64_t total = 8, cols = 32, n = 256 * cols, blk = n / total, B = 1ull << 40;
    const uint64_t rows = B + 4 * blk, scales = rows + total * (n / 2), hyper = scales + total * (n / 32), norm_sq = hyper + 96,
                   info = norm_sq + 4 * total, t_rows = info + 16, t_scales = t_rows + total * (n / 2), end = t_scales + total * (n / 32);
    tsa::AdamwMx2dRange r{tsa::Mx2dRange{at(rows), n / 2, at(scales), n / 32, at(t_rows), n / 2, at(t_scales), n / 32, n, cols, at(B), (end - B) / 4},
                          {at(2 * B), at(3 * B), at(4 * B)}};
    uint64_t per_byte = 2;
    if (!std::strcmp(argv[1], "rows-16")) r.out.rows = at(rows - 16);
    else if (!std::strcmp(argv[1], "t_scales+16")) r.out.t_scales = at(t_scales + 16);
    else if (!std::strcmp(argv[1], "per_byte-1")) per_byte = 1;
    else if (std::strcmp(argv[1], "exact")) return 2;
    std::printf("%d\n", (int)tsa::adamw_mx2d_list_verdict(&r, 1, total, at(hyper), at(norm_sq), at(info), 96, per_byte));
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the adamw_mx2d_ranges check"
    d = tmp_path_factory.mktemp("adamw_mx4_2d_ranges")
    (d / "check.cpp").write_text(PROGRAM)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", CSRC, str(d / "check.cpp"), "-o", str(d / "check")], check=True)
    return str(d / "check")


@pytest.mark.parametrize("case,verdict", [("exact", 0), ("rows-16", 1), ("t_scales+16", 1), ("per_byte-1", 1)])   # kAdamwMxOk, kAdamwMxArg
def test_halved_payloads_fill_a_stride_gap_exactly(exe, case, verdict):
    run = subprocess.run([exe, case], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert int(run.stdout) == verdict
