"""The 2D MXFP8 soak's table (tests/mx2d_cases.py, SOAK_CASES) against csrc/mx2d_kernels.hip, on the CPU, as
tests/test_adamw_mx_table.py holds its table against adamw_mx_kernels.hip:

1. every trace_launch format string of mx2d_kernels.hip has a soak case at every rank count of its
   for_ranks<8, 64> and at all four (RCEIL, ROWS) values; the table names no kernel the file does not launch;
   the list is long enough for three work units per workgroup whatever patch the build takes;
2. every hipLaunchKernelGGL of the file has a trace record beside it: the statement that follows the launch is
   a trace_launch;
3. the file keeps to its rules: no inline assembly, no wait of its own beyond lds_barrier().
"""
import os
import re

import mx2d_cases as mc
import soak_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")


def source(name=mc.SOAK_FILE):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_every_traced_launch_has_a_soak_case():
    text = source()
    formats = re.findall(r'trace_launch\([^"\n]*"([^"]+)"', text)
    bounds = set(re.findall(r"for_ranks<(\d+), (\d+)>", text))
    assert formats == [mc.SOAK_FORMAT], f"launches without a soak case, or cases without a launch: {formats}"
    assert bounds == {("8", "64")}, f"for_ranks{bounds}; the table's rank counts are {mc.SOAK_RANKS}"
    assert mc.SOAK_RANKS == sc.RANKS == (8, 16, 32, 64)
    assert mc.SOAK_FORMAT.count("%d") == 1 and mc.SOAK_FORMAT.count("%s") == 2
    ids = [mc.soak_case_id(c) for c in mc.SOAK_CASES]
    assert len(set(ids)) == len(ids) == 16
    lg = int(re.search(r"#define TSA_MX2D_LG_SIDE (\d+)", source("mx2d_span.hpp")).group(1))
    for p in mc.SOAK_RANKS:
        for rceil in (False, True):
            for rows in (False, True):
                hits = [c for c in mc.SOAK_CASES if (c["total"], c["rceil"], c["rows"]) == (p, rceil, rows)]
                assert len(hits) == 1, (p, rceil, rows)
                c = hits[0]
                assert c["shapes"] == mc.SOAK_SHAPES and c["grid"] == sc.GRID
                assert p * sum(mc.SOAK_SQUARES) >= 3 * c["grid"] * 4 ** lg   # units >= squares / 4^lg
    assert len(set(mc.SOAK_SHAPES)) == len(mc.SOAK_SHAPES) and all(cols % 32 == 0 and R % 32 == 0 for cols, R in mc.SOAK_SHAPES)
    assert mc.soak_kernel_name(16, True, False) == "k_ag_group_mxfp8_2d<16, true, false>"
    # the kernel is instantiated for exactly these template arguments: P from for_ranks, both bools both ways
    assert re.search(r"template <int P, bool RCEIL, bool ROWS>\s*__global__ __launch_bounds__\(kBlock\) void k_ag_group_mxfp8_2d\(", text)
    for a in ("true, true", "true, false", "false, true", "false, false"):
        assert f"k_ag_group_mxfp8_2d<p(), {a}>" in text, a


def test_every_launch_has_a_trace_record_beside_it():
    text = re.sub(r"//[^\n]*", "", source())   # comments may name either call
    launches = [m.end() for m in re.finditer(r"\bhipLaunchKernelGGL\(", text)]
    assert launches, "the file launches nothing"
    for at in launches:
        depth, i = 1, at
        while depth:   # the end of the launch's argument list
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        rest = text[i:].lstrip()
        assert rest.startswith(";"), "a launch that is not a statement of its own"
        assert rest[1:].lstrip().startswith("trace_launch("), f"no trace record behind the launch at offset {at}: {rest[:60]!r}"
    assert len(re.findall(r"\btrace_launch\(", text)) == len(launches)


def test_the_file_keeps_to_its_rules():
    text = re.sub(r"//[^\n]*", "", source())
    assert not re.search(r"\basm\b|__asm", text), "inline assembly"
    assert not re.search(r"waitcnt|\bs_barrier|__syncthreads|sched_barrier", text), "a wait of the file's own"
    assert len(re.findall(r"\blds_barrier\(\)", text)) == 2
