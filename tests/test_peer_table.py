"""tests/peer_cases.py is complete, and its inputs can show a wrong add order — checked on the CPU,
so a new peer kernel, a new k_hier_* instance or a launch site without a trace record fails here
before anything runs on a GPU.
"""
import os
import re

import numpy as np
import pytest

import hard_inputs
import oracle
import peer_cases
import test_dist_host as tdh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")
SEED = 7


def peer_kernels_hip():
    return open(os.path.join(CSRC, "peer_kernels.hip")).read()


def global_kernels():
    src = peer_kernels_hip()
    names = re.findall(r"__global__\s+(?:__launch_bounds__\(.*\)\s+)?void\s+(\w+)\s*\(", src)
    assert len(names) == 10 and len(names) == src.count("__global__"), names
    return names


def traced_names():
    return {name for c in peer_cases.CASES for name in c["trace"]}


def test_every_peer_kernel_heads_a_trace():
    bases = {name.split("<")[0] for name in traced_names()}
    for k in global_kernels():
        assert k in bases, f"{k}: defined in peer_kernels.hip — it needs a case in tests/peer_cases.py"
    assert set(peer_cases.PEER_KERNELS) | {"k_hier_ws", "k_hier_x2"} == set(global_kernels())


def test_every_hier_instance_has_a_case():
    names = traced_names()
    for a in (1, 2):
        for cw in (8, 16, 32):
            assert f"k_hier_ws<{a}, {cw}>" in names, (a, cw)
    for name in ("k_hier_x2", "k_hier_x2<chunked>"):
        assert name in names, name
    # the names are the launchers' own spelling, and nothing else is in a trace (a typo would pass above)
    src = peer_kernels_hip()
    hier = [f"k_hier_ws<{a}, {cw}>" for a, cw in peer_cases.HIER_WS] + peer_cases.HIER_X2
    for name in hier + peer_cases.PEER_KERNELS:
        assert f'"{name}"' in src, f"{name}: not a name peer_kernels.hip reports"
    kernels_hip = open(os.path.join(CSRC, "kernels.hip")).read()
    for name in peer_cases.ENGINE_KERNELS:
        assert f'"{re.sub(r"<.*", "", name)}' in kernels_hip, name
    assert names == set(hier + peer_cases.PEER_KERNELS + peer_cases.ENGINE_KERNELS), names
    # the instances the launcher can select are the six the table lists
    assert sorted(set(re.findall(r"k_hier_ws<(\d), (\d+)>", src))) == \
        sorted((str(a), str(cw)) for a, cw in peer_cases.HIER_WS)


def test_every_launch_site_feeds_the_trace():
    """a hipLaunchKernelGGL in peer_kernels.hip without a trace_launch / note_launch beside it would be a blind spot"""
    lines = peer_kernels_hip().splitlines()
    sites = [i for i, line in enumerate(lines) if "hipLaunchKernelGGL(" in line]
    assert len(sites) == 12, len(sites)
    for i in sites:
        window = "\n".join(lines[i:i + 10])
        assert "trace_launch(" in window or "note_launch(" in window, \
            f"peer_kernels.hip:{i + 1}: launch without a trace record"
    # allred_last_launch is what the bench reads: the two note_launch sites and their names stay
    assert peer_kernels_hip().count("note_launch(") == 2


def test_dist_cases_are_test_dist_host_cases():
    for world in peer_cases.MULTI:
        assert peer_cases.dist_cases(world) == tdh.cases(world)
        side, total = tdh.GRIDS[world]
        assert total == world
        for variant in ("bo", "lo"):
            for form in ("sched",) + (("push",) if variant == "bo" else ()):
                got = [(c["algo"], c["local"], c["channels"]) for c in peer_cases.CASES
                       if c["id"].startswith(f"dist-{variant}-{form}-") and c["worlds"] == (world,)]
                assert got == [x[1:] for x in tdh.cases(world) if x[0] == variant], (world, variant, form)
        ll = [c for c in peer_cases.CASES if c["id"].startswith("dist-lo-ll-") and c["worlds"] == (world,)]
        assert len(ll) == sum(1 for x in tdh.cases(world) if x[0] == "lo" and x[3] == 1)
        assert {1, 2, world - 1} & {c["channels"] for c in peer_cases.CASES if c["worlds"] == (world,)} >= {1, world - 1}


def test_cases_are_well_formed():
    ids = [c["id"] for c in peer_cases.CASES]
    assert len(ids) == len(set(ids))
    for c in peer_cases.CASES:
        assert c["program"] in peer_cases.PROGRAMS and c["worlds"] and set(c["worlds"]) <= set(peer_cases.ALL_WORLDS)
        assert set(c["knobs"]) == {"oneshot_max", "mem_ll_max", "hier_ll", "lo_ll_max", "sched_push", "max_groups"}
        assert set(c["keys"]) <= {"hier_ws_cols", "hier_ws_ahead"}
        assert len(c["trace"]) <= 64, c["id"]   # the trace keeps the first 64 names
        assert all(set(c["peer_fence"][w]) <= {0, 1} and 0 in c["peer_fence"][w] for w in c["worlds"])
        dist = c["program"].startswith("dist_")
        assert (c["before"] == "mem_oneshot") == dist and (1 in c["worlds"]) != dist, c["id"]
        assert c["calls"] == (3 if c["program"] == "hier_x2" else 2)
        for world in c["worlds"]:
            n, rows = peer_cases.elems(c, world), world * c["local"]
            # the hard inputs fit: one draw over all W * local rows, planted columns need room
            assert n % 8 == 0 and n >= hard_inputs.MIN_ELEMS
            assert len(hard_inputs.cancel_columns(rows, n)) == 18
            assert len(hard_inputs.nonfinite_columns(rows, n)) == 3 * len(hard_inputs.nonfinite_classes(rows))
            # and the shape divides as its program needs
            assert n % (8 * world) == 0, c["id"]
            if c["program"] in ("hier", "hier_x2"):
                assert c["local"] == 64 and n % (256 * world) == 0, c["id"]
            if dist:
                assert c["local"] in (1, 4) and 1 <= c["channels"] <= max(1, world - 1), c["id"]
    # the routes the table must hold, by name: a case that leaves is missed here (the scheduled
    # programs: test_dist_cases_are_test_dist_host_cases)
    ws = [f"hier-ws-a{a}-c{cw}{grid}" for a in (1, 2) for cw in (8, 16, 32) for grid in ("", "-one-group", "-ring")]
    forms = ("launches", "oneshot", "ll")
    assert sorted(i for i in ids if not i.startswith("dist-")) == sorted(
        [f"mem-{f}" for f in forms] + ws + [f"hier-launch-{f}" for f in forms] + ["hier-x2", "hier-x2-chunked"])
    # every non-dist case runs wherever the add order shows, and at W = 1 (the tree order alone)
    assert all({1, 4, 8} <= set(c["worlds"]) for c in peer_cases.CASES if not c["program"].startswith("dist_"))
    # where the add order shows, both fence forms run
    assert peer_cases.PEER_FENCE[4] == (0, 1)
    # the shapes the issue of the hand-off paths rests on
    by_id = {c["id"]: c for c in peer_cases.CASES}
    assert by_id["mem-oneshot"]["unit"] == 8 * 131
    assert by_id["hier-ws-a2-c16-ring"]["unit"] == 256 * 20 and by_id["hier-ws-a2-c16-ring"]["knobs"]["max_groups"] == 1
    assert by_id["hier-x2-chunked"]["unit"] // 256 > 8     # more tiles in the one workgroup than a chunk, at every W


# ------------------------------------------------------------------ the data can show the bug
def to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def rne(f):
    """fp32 -> bf16 bits, round to nearest even (finite values)"""
    b = np.asarray(f, dtype=np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def natural_order_sum(rows):
    """rows 0, 1, ..., W - 1 added in that order in fp32, rounded once: what a kernel that ignores
    'owner first' computes for every block"""
    acc = to_f32(rows[0]).copy()
    for r in rows[1:]:
        acc = acc + to_f32(r)
    return rne(acc)


def owner_first(rows):
    want = [np.array(r, dtype=np.uint16) for r in rows]
    oracle.allreduce("mem", 0, 1, want, len(want))
    assert all(np.array_equal(w, want[0]) for w in want)
    return want[0]


def hier_partials(kind, world, n, local, side):
    """the hierarchical dataset of tests/test_gpu_peer_hard.py: one draw over all W * local rows, dealt
    to the GPUs in order; the partial of a GPU is the oracle's tree of its local rank 0"""
    data = getattr(hard_inputs, kind)(world * local, n, SEED).reshape(world, local, n)
    partials = []
    for d in data:
        loc = [x.copy() for x in d]
        oracle.allreduce("lo", 1, side, loc, local)
        partials.append(loc[0])
    return partials


def differing(rows):
    return float((natural_order_sum(rows) != owner_first(rows)).mean())


@pytest.mark.parametrize("world", [4, 8])
def test_cancel_data_shows_a_natural_order_sum(world):
    """The floor is a condition on the INPUTS: at least 5 % of the columns must tell the owner-first
    order from the natural one, or a pass of the GPU test would mean nothing.  Measured: 27 % / 32 %
    of the flat columns and 12 % / 18 % of the hierarchical ones at W = 4 / 8."""
    flat = differing(list(hard_inputs.cancel(world, peer_cases.DIST_UNIT * world, SEED)))
    hier = differing(hier_partials("cancel", world, peer_cases.HIER_UNIT * world, 64, 8))
    print(f"W = {world}: a natural-order sum differs in {flat:.1%} of the flat and {hier:.1%} of the hierarchical columns")
    assert flat >= 0.05 and hier >= 0.05
    # the mem cases' own shape as well
    assert differing(list(hard_inputs.cancel(world, peer_cases.MEM_UNIT * world, SEED))) >= 0.05


@pytest.mark.parametrize("world", [2, 4, 8])
def test_soft_data_cannot_show_it(world):
    """the reason for the table: on [1, 100) data any order gives the oracle's bits"""
    assert differing(list(hard_inputs.soft(world, peer_cases.DIST_UNIT * world, SEED))) == 0.0
    rows = [np.random.default_rng(77 + r).integers(0x3F80, 0x42C8, (64, 256 * world)).astype(np.uint16) for r in range(world)]
    partials = []
    for d in rows:
        loc = [x.copy() for x in d]
        oracle.allreduce("lo", 1, 8, loc, 64)
        partials.append(loc[0])
    assert differing(partials) == 0.0


def test_two_addends_commute():
    """W = 2 checks transport and bit patterns only: owner-first and natural order are the same sum"""
    assert differing(list(hard_inputs.cancel(2, peer_cases.DIST_UNIT * 2, SEED))) == 0.0
    assert differing(hier_partials("cancel", 2, peer_cases.HIER_UNIT * 2, 64, 8)) == 0.0


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_oracle_compositions_accept_the_hard_data(world):
    """the expected values of the GPU test exist and every nonfinite column meets its stated class"""
    n = peer_cases.HIER_UNIT * world
    want = owner_first(hier_partials("nonfinite", world, n, 64, 8))
    assert hard_inputs.check_nonfinite(want, want, world * 64, n) == 3 * len(hard_inputs.nonfinite_classes(world * 64))
    n = peer_cases.MEM_UNIT * world
    want = owner_first(list(hard_inputs.nonfinite(world, n, SEED)))
    assert hard_inputs.check_nonfinite(want, want, world, n) == 3 * len(hard_inputs.nonfinite_classes(world))
