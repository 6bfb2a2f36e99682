"""The one rule allred_plan_all_gather_shards_mxfp4_2d_sr adds to the 2D call's: its 16-byte state shares no byte with
any of a bucket's up to four output intervals — csrc/mx2d_ranges.hpp mx2d_small_disjoint, what engine.cpp applies
before any HIP call — in a stand-alone program under g++ with AddressSanitizer and UBSan, as tests/test_mx2d_ranges.py
compiles its own.  Then the entry points without a device.  The launch counts need a plan, and a plan a device: they
are tests/test_gpu_shards_mxfp4_2d_sr.py's."""
import os
import subprocess

from tenstorrentallreduce_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tenstorrentallreduce_amd", "csrc")
PROGRAM = r"""
#include <cstdio>
#include "mx2d_ranges.hpp"
using namespace tsa;
static const void* at(uint64_t a) { return reinterpret_cast<const void*>((uintptr_t)a); }
int main() {
    // total strides: rows 8 * 4096 + skew, scales 8 * 256, t rows 8 * 4096, t scales 8 * 256 + skew
    const uint64_t total = 8, n = 8192, R = 1ull << 40, S = 1ull << 41, TR = 1ull << 42, TS = 1ull << 43, SH = 1ull << 44;
    const Mx2dRange both{at(R), n / 2 + 48, at(S), n / 32, at(TR), n / 2, at(TS), n / 32 + 24, n, 32, at(SH), n / total};
    const Mx2dRange tonly{nullptr, 0, nullptr, 0, at(TR + (1ull << 30)), n / 2, at(TS + (1ull << 30)), n / 32, n, 32, at(SH + (1ull << 30)), n / total};
    const Mx2dRange list[2] = {both, tonly};
    int bad = 0, k = 0;
    auto expect = [&](uint64_t p, uint64_t bytes, bool want) {
        ++k;
        if (mx2d_small_disjoint(list, 2, total, at(p), bytes) != want) { std::printf("MISMATCH check %d\n", k); bad = 1; }
    };
    const uint64_t ends[4][2] = {{R, R + total * (n / 2 + 48)}, {S, S + total * (n / 32)}, {TR, TR + total * (n / 2)},
                                 {TS, TS + total * (n / 32 + 24)}};
    for (const auto& e : ends) {
        expect(e[0] - 16, 16, true);    // touching from below
        expect(e[0] - 8, 16, false);    // eight bytes in
        expect(e[0], 16, false);
        expect(e[1] - 8, 16, false);    // the last stride's skew belongs to the interval
        expect(e[1], 16, true);         // touching from above
        expect(e[0] - 16, e[1] - e[0] + 32, false);   // the interval inside the state's
    }
    expect(TS + (1ull << 30) + 8 * (n / 32) - 8, 16, false);   // the second bucket's t scales
    expect(TS + (1ull << 30) + 8 * (n / 32), 16, true);
    expect(SH + 64, 16, true);                  // the shard is only read: the state may lie in it
    expect(0, 16, true);                        // absent rows (nullptr, stride 0) collide with nothing
    expect(UINT64_MAX - 7, 16, false);          // the state ends beyond the address space
    expect(R + 8, 0, true);                     // an empty interval collides with nothing
    if (!bad) std::printf("mx2d_sr_ranges ok: %d checks\n", k);
    return bad;
}
"""


def test_the_state_is_off_all_four_output_intervals(tmp_path):
    src, exe = tmp_path / "mx2d_sr_ranges_check.cpp", tmp_path / "mx2d_sr_ranges_check"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "mx2d_sr_ranges ok" in run.stdout, run.stdout + run.stderr


def test_mxfp4_2d_sr_entry_points_refuse_before_any_hip_call():
    """no GPU here: a call that got as far as HIP would not return ALLRED_ERR_ARG"""
    arr = (_lib.Mx2dBucketF32 * 1)((1 << 40, 4096, 1 << 39, 256, 1 << 41, 4096, 1 << 38, 256, 8192, 32, 1 << 42, 1024))
    call, dry = _lib.lib.allred_plan_all_gather_shards_mxfp4_2d_sr, _lib.lib.allred_plan_all_gather_shards_mxfp4_2d_sr_launches
    assert _lib.MX4_2D_SR_GROUP_MAX == 20
    assert call(None, arr, 1, 0, 0, 1 << 43, None) == _lib.ERR_ARG     # a NULL plan
    assert call(None, arr, 1, 0, 0, None, None) == _lib.ERR_ARG        # a NULL state
    assert call(None, None, 0, 4, 0, 1 << 43, None) == _lib.ERR_ARG    # an unknown flag bit, which an empty list does not excuse
    assert dry(None, arr, 1) == _lib.ERR_ARG
