"""The one argument rule of allred_plan_all_gather_shards_mxfp4 that differs from the MXFP8 call's — the row payload is
elems_per_rank / 2 bytes —: mx_ranges.hpp's mx_list_verdict, what engine.cpp applies before any HIP call, under g++
with per_byte = 2 and, on the same lists, its default.  A plan needs a device, so the stride cases through the
`_launches` twin are tests/test_gpu_shards_mxfp4.py's; what the two calls share is tests/test_mx_ranges.py's."""
import os
import subprocess

from tenstorrentallreduce_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tenstorrentallreduce_amd", "csrc")
PROGRAM = r"""
#include <cstdio>
#include "mx_ranges.hpp"
using namespace tsa;
static const void* at(uint64_t a) { return reinterpret_cast<const void*>((uintptr_t)a); }
int main() {
    const uint64_t total = 8, n = 256 * 8 * 3, rows = 1ull << 40, end = rows + total * n / 2, far = 1ull << 30;
    auto one = [&](uint64_t r, uint64_t stride, uint64_t scales, uint64_t shard) {
        return MxRange{at(r), stride, at(scales), n / 32, n, at(shard), n / total};
    };
    const MxRange half = one(rows, n / 2, 1ull << 41, 1ull << 42), full = one(rows, n, 1ull << 41, 1ull << 42);
    const MxRange shrt = one(rows, n / 2 - 16, 1ull << 41, 1ull << 42), odd = one(rows, n / 2 + 8, 1ull << 41, 1ull << 42);
    MxRange two[2] = {half, one(end, n / 2, (1ull << 41) + far, (1ull << 42) + far)};   // rows right behind the first's n / 2-byte rows
    int bad = 0, k = 0;
    auto expect = [&](MxVerdict got, MxVerdict want) { ++k; if (got != want) { std::printf("MISMATCH check %d\n", k); bad = 1; } };
    expect(mx_list_verdict(&half, 1, total, 2), kMxOk);
    expect(mx_list_verdict(&half, 1, total), kMxArg);        // the MXFP8 call on the same list still demands n
    expect(mx_list_verdict(&shrt, 1, total, 2), kMxArg);
    expect(mx_list_verdict(&odd, 1, total, 2), kMxArg);
    expect(mx_list_verdict(&full, 1, total, 2), kMxOk);
    expect(mx_list_verdict(&full, 1, total), kMxOk);
    expect(mx_list_verdict(&half, 1, total, 3), kMxArg);
    expect(mx_list_verdict(two, 2, total, 2), kMxOk);        // 8: rows abut
    two[1].rows = at(end - 16);
    expect(mx_list_verdict(two, 2, total, 2), kMxArg);       // one 16-byte quantum into the first's rows
    two[1] = one(1ull << 50, n / 2, end - 8, (1ull << 42) + far);
    expect(mx_list_verdict(two, 2, total, 2), kMxArg);       // scale rows on the rows' last 8 bytes
    two[1].scales = at(end);
    expect(mx_list_verdict(two, 2, total, 2), kMxOk);        // and right behind them
    if (!bad) std::printf("mx4_ranges ok\n");
    return bad;
}
"""


def test_the_row_payload_is_half_the_elements(tmp_path):
    src, exe = tmp_path / "mx4_ranges_check.cpp", tmp_path / "mx4_ranges_check"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "mx4_ranges ok" in run.stdout, run.stdout + run.stderr


def test_mxfp4_entry_points_refuse_before_any_hip_call():
    """no GPU here: a call that got as far as HIP would not return ALLRED_ERR_ARG"""
    arr = (_lib.MxBucketF32 * 1)((1 << 40, 1024, 1 << 39, 64, 2048, 1 << 41, 256))
    assert _lib.lib.allred_plan_all_gather_shards_mxfp4(None, arr, 1, 0, None) == _lib.ERR_ARG
    assert _lib.lib.allred_plan_all_gather_shards_mxfp4(None, arr, 1, 2, None) == _lib.ERR_ARG
    assert _lib.lib.allred_plan_all_gather_shards_mxfp4_launches(None, arr, 1) == _lib.ERR_ARG
