"""tests/route_cases.py is complete — checked on the CPU, so a new kernel or a new instantiation
without a route case fails here before anything runs on a GPU.
"""
import os
import re

import hard_inputs
import route_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")


def kernels_hip():
    return open(os.path.join(CSRC, "kernels.hip")).read()


def global_kernels():
    names = re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", kernels_hip())
    assert len(names) >= 25 and len(names) == kernels_hip().count("__global__")
    return names


def traced_names():
    return {name for c in route_cases.CASES for name in c["trace"]}


def test_every_kernel_has_a_route_case_or_a_stated_exemption():
    bases = {name.split("<")[0] for name in traced_names()}
    for k in global_kernels():
        assert (k in bases) != (k in route_cases.EXEMPT), \
            f"{k}: defined in kernels.hip — it needs a case in tests/route_cases.py, or an entry in EXEMPT (not both)"
    assert set(route_cases.EXEMPT) == {"k_add", "k_add_scalar", "k_add_segs", "k_validate"}
    for k, where in route_cases.EXEMPT.items():
        path = where.split()[0]
        assert os.path.exists(os.path.join(ROOT, path)), (k, path)
    assert bases <= set(global_kernels()), bases - set(global_kernels())


def test_every_instantiated_rank_count_has_a_route_case():
    names = traced_names()
    for pattern, ranks in route_cases.RANGES.items():
        rx = re.compile("^" + re.escape(pattern).replace("P", r"(\d+)", 1) + "$")
        got = sorted({int(m.group(1)) for m in map(rx.match, names) if m})
        assert got == ranks, f"{pattern}: the table covers the rank counts {got}, the launch site instantiates {ranks}"
    for name in route_cases.FIXED:
        assert name in names, f"{name}: no route case"
    # and nothing in a trace that neither list knows: a typo in a trace would otherwise pass here
    known = [re.compile("^" + re.escape(p).replace("P", r"\d+", 1) + "$") for p in route_cases.RANGES]
    for name in names:
        assert name in route_cases.FIXED or any(rx.match(name) for rx in known), name


def test_ranges_are_the_launch_sites_of_kernels_hip():
    """the for_ranks<LO, HI> written at each launch site: the ranges of RANGES are read from the source"""
    src = kernels_hip()
    sites = re.findall(r"for_ranks<(\d+), (\d+)>\(total, \[&\]\(auto p\) \{(.*?)\}\);", src, flags=re.S)
    assert len(sites) >= 9
    seen = {}
    for lo, hi, body in sites:
        ranks = [p for p in route_cases.ALL_RANKS if int(lo) <= p <= int(hi)]
        for kernel in set(re.findall(r"\(?(k_\w+)<p\(\)", body)) | set(re.findall(r"&(k_\w+)<p\(\)", body)):
            seen.setdefault(kernel, []).append(ranks)
    assert set(seen) == {p.split("<")[0] for p in route_cases.RANGES if p != "k_tree_lds_lag<P>"}, sorted(seen)
    for pattern, ranks in route_cases.RANGES.items():
        base = pattern.split("<")[0]
        if base != "k_tree_lds_lag":
            assert all(r == ranks for r in seen[base]), (pattern, seen[base])
    # every entry of the generated DAG list has its case
    inc = os.path.join(ROOT, "tenstorrentallreduce_amd", "build", "lo_dag_gen.inc")
    if os.path.exists(inc):
        dags = {f"k_lo_dag_reg<{d}>" for d in re.findall(r"X\((LoDag\d+),", open(inc).read())}
        assert dags == {n for n in route_cases.FIXED if n.startswith("k_lo_dag_reg<")}


def test_every_launch_site_feeds_the_trace():
    """a hipLaunchKernelGGL in kernels.hip without a trace_launch / note_launch beside it would be a blind spot"""
    src = kernels_hip()
    launches = len(re.findall(r"hipLaunchKernelGGL\(", src)) - len(re.findall(r"#define \w+\(.*hipLaunchKernelGGL\(", src))
    assert launches >= 35
    lines = src.splitlines()
    for i, line in enumerate(lines):
        if "hipLaunchKernelGGL(" in line:
            window = "\n".join(lines[i:i + 10])
            assert "trace_launch(" in window or "note_launch(" in window, f"kernels.hip:{i + 1}: launch without a trace record"


def test_every_launch_site_of_the_shard_family_feeds_the_trace():
    """the same for the fp32-shard files: their traces are what the grouped GPU tests pin"""
    for name, at_least in (("shard_f32_kernels.hip", 5), ("adamw_kernels.hip", 4), ("mx_kernels.hip", 2)):
        lines = open(os.path.join(CSRC, name)).read().splitlines()
        sites = [i for i, line in enumerate(lines) if "hipLaunchKernelGGL(" in line]
        assert len(sites) >= at_least, name
        for i in sites:
            assert "trace_launch(" in "\n".join(lines[i:i + 10]), f"{name}:{i + 1}: launch without a trace record"


def test_cases_are_well_formed():
    ids = [c["id"] for c in route_cases.CASES]
    assert len(ids) == len(set(ids)) and len(ids) >= 150
    for c in route_cases.CASES:
        assert c["op"] in route_cases.OPS
        assert route_cases.SIDE[c["total"]] == c["side"] or c["algo"] in (route_cases.SWING_1D, route_cases.RECDUB_1D)
        shapes = [n for n, _ in c["buckets"]] if c["buckets"] else [c["n"]]
        for n in shapes:   # the hard inputs fit: planted columns need room, BO and MEM need whole blocks
            assert n % 8 == 0 and n >= hard_inputs.MIN_ELEMS
            if c["op"] != "tree_bcast" and (c["variant"] != route_cases.LO or c["op"] != "allreduce"):
                assert n % (8 * c["total"]) == 0, c["id"]
            assert len(hard_inputs.cancel_columns(c["total"], n)) == 18
        grid = c["keys"].get("pipe_grid")
        assert grid is None or 3 <= grid <= 7, c["id"]
