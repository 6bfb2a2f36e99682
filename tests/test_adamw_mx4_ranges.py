"""The one argument rule of allred_plan_adamw_all_gather_shards_mxfp4 that differs from the MXFP8 AdamW call's — the
row payload is elems_per_rank / 2 bytes —: adamw_mx_ranges.hpp's adamw_mx_list_verdict, what engine.cpp applies before
any HIP call, under g++ with per_byte = 2 and, on the same lists, its default.  The stride cases through a plan are
tests/test_gpu_adamw_mx4.py's; what the two calls share is tests/test_adamw_mx_ranges.py's."""
import os
import subprocess

from tenstorrentallreduce_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tenstorrentallreduce_amd", "csrc")
PROGRAM = r"""
#include <cstdio>
#include "adamw_mx_ranges.hpp"
using namespace tsa;
static const void* at(uint64_t a) { return reinterpret_cast<const void*>((uintptr_t)a); }
int main() {
    const uint64_t total = 8, n = 256 * 8 * 3, rows = 1ull << 40, end = rows + total * n / 2, far = 1ull << 30;
    auto one = [&](uint64_t r, uint64_t stride, uint64_t scales, uint64_t planes) {
        return AdamwMxRange{at(r), stride, at(scales), n / 32, n, {at(planes), at(planes + 4 * n), at(planes + 8 * n), at(planes + 12 * n)},
                            n / total};
    };
    const AdamwMxRange half = one(rows, n / 2, 1ull << 41, 1ull << 42), full = one(rows, n, 1ull << 41, 1ull << 42);
    const AdamwMxRange shrt = one(rows, n / 2 - 16, 1ull << 41, 1ull << 42), odd = one(rows, n / 2 + 8, 1ull << 41, 1ull << 42);
    AdamwMxRange two[2] = {half, one(end, n / 2, (1ull << 41) + far, (1ull << 42) + far)};   // rows right behind the first's n / 2-byte rows
    const void *hyper = at(1ull << 43), *nsq = at(1ull << 44), *info = at(1ull << 45);
    int bad = 0, k = 0;
    auto expect = [&](AdamwMxVerdict got, AdamwMxVerdict want) { ++k; if (got != want) { std::printf("MISMATCH check %d\n", k); bad = 1; } };
    auto verdict = [&](const AdamwMxRange* l, int count, uint64_t per_byte, const void* h) {
        return adamw_mx_list_verdict(l, count, total, h, nsq, info, kAdamwHyperBytes, per_byte);
    };
    expect(verdict(&half, 1, 2, hyper), kAdamwMxOk);
    expect(adamw_mx_list_verdict(&half, 1, total, hyper, nsq, info), kAdamwMxArg);   // the MXFP8 call on the same list still demands n
    expect(verdict(&half, 1, 1, hyper), kAdamwMxArg);
    expect(verdict(&shrt, 1, 2, hyper), kAdamwMxArg);
    expect(verdict(&odd, 1, 2, hyper), kAdamwMxArg);
    expect(verdict(&full, 1, 2, hyper), kAdamwMxOk);
    expect(adamw_mx_list_verdict(&full, 1, total, hyper, nsq, info), kAdamwMxOk);
    expect(verdict(&half, 1, 3, hyper), kAdamwMxArg);
    expect(verdict(two, 2, 2, hyper), kAdamwMxOk);                  // 9: rows abut at total * n / 2
    two[1].rows = at(end - 16);
    expect(verdict(two, 2, 2, hyper), kAdamwMxArg);                 // one 16-byte quantum into the first's rows
    expect(verdict(&half, 1, 2, at(end - 32)), kAdamwMxArg);        // hyper on the rows' last bytes
    expect(verdict(&half, 1, 2, at(end - 16)), kAdamwMxArg);
    expect(verdict(&half, 1, 2, at(end)), kAdamwMxOk);              // and right behind them
    if (!bad) std::printf("adamw_mx4_ranges ok\n");
    return bad;
}
"""


def test_the_row_payload_is_half_the_elements(tmp_path):
    src, exe = tmp_path / "adamw_mx4_ranges_check.cpp", tmp_path / "adamw_mx4_ranges_check"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "adamw_mx4_ranges ok" in run.stdout, run.stdout + run.stderr


def test_adamw_mxfp4_entry_points_refuse_before_any_hip_call():
    """no GPU here: a call that got as far as HIP would not return ALLRED_ERR_ARG"""
    arr = (_lib.AdamwMxBucketF32 * 1)((1 << 40, 1024, 1 << 39, 64, 2048, 1 << 41, 1 << 42, 1 << 43, 1 << 44, 256))
    call, dry = _lib.lib.allred_plan_adamw_all_gather_shards_mxfp4, _lib.lib.allred_plan_adamw_shards_mxfp4_launches
    assert call(None, arr, None, 1, 1 << 45, 1, None, None, 0, None) == _lib.ERR_ARG            # a NULL plan
    assert call(None, arr, None, 1, 1 << 45, 1, None, None, 4, None) == _lib.ERR_ARG            # and an unknown flag bit
    assert call(None, None, None, 0, 1 << 45, 1, None, None, 4, None) == _lib.ERR_ARG           # which an empty list does not excuse
    assert dry(None, arr, 1) == _lib.ERR_ARG
