"""The soak's tables (tests/soak_cases.py) on the CPU: what they cover, what they leave out, and where
arrangement (c) lies.

1. Every trace_launch format string of shard_f32_kernels.hip, adamw_kernels.hip and mx_kernels.hip has a soak
   case at every rank count of its for_ranks<8, 64> and at each value of its bool; the table names no kernel
   those files do not launch.
2. The route soak leaves out exactly the route cases whose trace is empty.
3. Arrangement (c) by arithmetic: the line of every partial is the line of a shard float of the launch — all
   of them at P = 8; at P = 64 all but the ONE line that 256 contiguous bytes of partials must fill alone — and
   csrc/shard_f32_norm_ranges.hpp accepts the layout (a stand-alone C++ program, compiled with g++ under
   AddressSanitizer and UBSan and run directly, as tests/test_shard_f32_norm_ranges.py does).
"""
import os
import re
import shutil
import subprocess

import pytest

import route_cases
import soak_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")
FILES = ("shard_f32_kernels.hip", "adamw_kernels.hip", "mx_kernels.hip")


def traced(name):
    """(the format strings of the file's trace_launch calls, the bounds of its for_ranks)"""
    with open(os.path.join(CSRC, name)) as f:
        text = f.read()
    return re.findall(r'trace_launch\([^"\n]*"([^"]+)"', text), set(re.findall(r"for_ranks<(\d+), (\d+)>", text))


def test_every_traced_launch_has_a_soak_case():
    table = {(f, fmt) for f, fmt, _ in sc.KERNELS.values()}
    found = set()
    for name in FILES:
        formats, bounds = traced(name)
        assert formats, name
        assert bounds == {("8", "64")}, f"{name}: for_ranks{bounds}; the table's rank counts are {sc.RANKS}"
        found |= {(name, fmt) for fmt in formats}
    assert found == table, f"launches without a soak case: {found - table}; cases without a launch: {table - found}"
    assert sc.RANKS == (8, 16, 32, 64)
    ids = [sc.case_id(c) for c in sc.SHARD_CASES]
    assert len(set(ids)) == len(ids)
    for family, (_, fmt, flags) in sc.KERNELS.items():
        assert (fmt.count("%s") == 1) == (flags is not None) and fmt.count("%d") == 1
        for p in sc.RANKS:
            for flag in flags or (None,):
                hits = [c for c in sc.SHARD_CASES if (c["family"], c["total"], c["flag"]) == (family, p, flag)]
                assert len(hits) == 1, (family, p, flag)
                c = hits[0]
                assert c["tiles"] == (1, 3, 2, 5) and c["grid"] == 5 and p * sum(c["tiles"]) >= 3 * c["grid"]
    assert sc.kernel_name("norm", 16, True) == "k_tree_group_f32_norm<16, true>" and sc.kernel_name("ag", 8, None) == "k_ag_group_f32<8>"


def test_the_hand_off_arrangements():
    got = {(c["arrangement"], c["total"], c["flag"]) for c in sc.HANDOFF_CASES}
    want = {(a, p, acc) for a, p in (("eighty", 8), ("grid", 8), ("warm", 8), ("warm", 64), ("chain", 8)) for acc in (False, True)}
    assert got == want and len(sc.HANDOFF_CASES) == len(want)
    by = {(c["arrangement"], c["total"]): c for c in sc.HANDOFF_CASES}
    assert sum(by["eighty", 8]["tiles"]) == 80                                   # partials per rank, past 64
    assert by["grid", 8]["grid"] > 8 * sum(by["grid", 8]["tiles"])               # pipe_grid above the tile count
    assert len(by["chain", 8]["tiles"]) == 65 and by["chain", 8]["launches"] == 2
    assert all(by["warm", p]["tiles"] == (1,) for p in (8, 64))


def test_the_route_soak_leaves_out_the_empty_traces_only():
    assert sorted(sc.ROUTE_EXCLUDED) == sorted(c["id"] for c in route_cases.CASES if not c["trace"])
    assert all(c["total"] == 1 for c in route_cases.CASES if c["id"] in sc.ROUTE_EXCLUDED)


@pytest.mark.parametrize("total,alone", [(8, 0), (64, 1)])
def test_arrangement_c_shares_its_lines(total, alone):
    blocks, ws, partials, nbytes = sc.warm_layout(total)
    assert ws[0] % 16 == 0 and blocks[0][0] % 16 == 0 and sc.WARM_STRIDE % 4 == 0 and sc.WARM_STRIDE >= sc.WARM_BLK
    assert ws[1] - ws[0] == 64 + 4 * total and partials == (ws[0] + 64, ws[1]) and nbytes >= blocks[-1][1]
    assert all(ws[1] <= lo or hi <= ws[0] for lo, hi in blocks), "the workspace shares a byte with a shard block"
    assert blocks[0][1] == ws[0] and ws[1] <= blocks[1][0]                       # in the gap behind block 0
    shard_lines = {(lo + 4 * i) // sc.LINE for lo, hi in blocks for i in range((hi - lo) // 4)}
    partial_lines = [(partials[0] + 4 * i) // sc.LINE for i in range(total)]
    unshared = sorted(set(partial_lines) - shard_lines)
    assert len(unshared) == alone, (sorted(set(partial_lines)), unshared)
    for line in unshared:   # only a line that partials fill end to end may be without shard floats
        assert partial_lines.count(line) == sc.LINE // 4
    if total == 8:
        assert set(partial_lines) == {8} and ws[0] // sc.LINE == 8 == (ws[1] - 1) // sc.LINE
    else:
        assert sorted(set(partial_lines)) == [8, 9, 10] and ws[1] == blocks[1][0]


PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>

#include "shard_f32_norm_ranges.hpp"

using tsa::ShardF32Range;
static const void* at(uint64_t a) { return reinterpret_cast<const void*>((uintptr_t)a); }

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const uint64_t total = std::strtoull(argv[1], nullptr, 10), shard_off = std::strtoull(argv[2], nullptr, 10),
                   stride = std::strtoull(argv[3], nullptr, 10), ws_off = std::strtoull(argv[4], nullptr, 10),
                   ws_bytes = std::strtoull(argv[5], nullptr, 10);
    const uint64_t B = 1ull << 41, rows = 1ull << 40, sq = 1ull << 42;
    std::vector<ShardF32Range> list = {ShardF32Range{at(rows), 256 * total + 64, 256 * total, at(B + shard_off), stride}};
    if (!tsa::shard_f32_lists_disjoint(list.data(), 1, total)) return std::printf("the list is refused\n"), 1;
    if (!tsa::shard_f32_norm_disjoint(list.data(), 1, total, at(sq), 4 * total, at(B + ws_off), ws_bytes))
        return std::printf("the workspace in the gap is refused\n"), 1;
    // one byte later it reaches into block 1 (P = 64) or stays in the gap (P = 8); 16 bytes earlier it is on block 0
    if (tsa::shard_f32_norm_disjoint(list.data(), 1, total, at(sq), 4 * total, at(B + ws_off - 16), ws_bytes))
        return std::printf("a workspace on block 0's last bytes is accepted\n"), 1;
    std::printf("warm layout ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def ranges_program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the ranges check"
    d = tmp_path_factory.mktemp("soak_ranges")
    src, exe = d / "warm_ranges_check.cpp", d / "warm_ranges_check"
    src.write_text(PROGRAM)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("total", [8, 64])
def test_arrangement_c_passes_the_ranges_headers(ranges_program, total):
    _, ws, _, _ = sc.warm_layout(total)
    run = subprocess.run([ranges_program, str(total), str(sc.WARM_SHARD_OFF), str(sc.WARM_STRIDE), str(ws[0]), str(ws[1] - ws[0])],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "warm layout ok" in run.stdout, run.stdout + run.stderr
