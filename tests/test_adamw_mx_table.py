"""The AdamW-MXFP8 soak's table (tests/adamw_mx_cases.py, SOAK_CASES) against csrc/adamw_mx_kernels.hip, on the
CPU, as tests/test_soak_table.py holds tests/soak_cases.py against the three older shard-family files:

1. every trace_launch format string of adamw_mx_kernels.hip has a soak case at every rank count of its
   for_ranks<8, 64> and at all four (ZERO, RCEIL) values; the table names no kernel the file does not launch;
2. every hipLaunchKernelGGL of the file has a trace record beside it: the statement that follows the launch is
   a trace_launch.
"""
import os
import re

import adamw_mx_cases as mc
import soak_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")


def source():
    with open(os.path.join(CSRC, mc.SOAK_FILE)) as f:
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
    for p in mc.SOAK_RANKS:
        for zero in (False, True):
            for rceil in (False, True):
                hits = [c for c in mc.SOAK_CASES if (c["total"], c["zero"], c["rceil"]) == (p, zero, rceil)]
                assert len(hits) == 1, (p, zero, rceil)
                c = hits[0]
                assert c["tiles"] == sc.UNEQUAL and c["grid"] == sc.GRID and p * sum(c["tiles"]) >= 3 * c["grid"]
    assert mc.SOAK_GROUP_OF == sc.GROUP_OF and len(mc.SOAK_GROUP_OF) == len(mc.SOAK_TILES)
    assert mc.soak_kernel_name(16, True, False) == "k_adamw_ag_mxfp8<16, true, false>"
    # the kernel is instantiated for exactly these template arguments: P from for_ranks, both bools both ways
    assert re.search(r"template <int P, bool ZERO, bool RCEIL>\s*__global__ __launch_bounds__\(kBlock\) void k_adamw_ag_mxfp8\(", text)


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
