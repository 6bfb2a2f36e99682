"""Every kernel route of tests/route_cases.py through the replay soak (tests/soak.py) under uniform load.

tests/test_gpu_routes_stream.py replays its graph twice on the SAME input image, on an idle chip, with a
host synchronise between the replays: a value left over from replay 1 is the right value in replay 2.
Here every case is built twice by route_run.PREPARE — seed 7 (the images of the other route modules) and
seed 8 — into ONE set of device buffers; the call is captured once and replayed soak.R times back to back,
the two images alternating, every buffer restored and compared whole on the device after every replay,
while k_soak_load streams through 1 GiB on another hardware queue.  The data is `cancel`: bit for bit.

AT TWO RANKS `cancel` holds +B in one rank and -B in the other in every column, so every sum is +0 under any
seed: the eight two-rank cases that reduce restore different inputs but expect the same result bits in both
datasets, and a stale read of what the replay before left would pass there.  Every other case expects
different bits in consecutive replays (asserted when the case is built).

The trace recorded during the capture is the case's.  The cases left out are exactly those whose trace is
empty (soak_cases.ROUTE_EXCLUDED): the one-rank cases that enqueue nothing and capture an empty graph.

The workspace of a plan is restored to 0xA5 before every replay, as route_run.Workspace.restore does; its
two guards are compared after every replay, and its content where the route defines it."""
import numpy as np
import pytest

import route_cases
import soak_cases
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import route_run  # noqa: E402  (needs torch)
import soak  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = (route_run.SEED, route_run.SEED + 1)
SOAKED = [c for c in route_cases.CASES if c["id"] not in soak_cases.ROUTE_EXCLUDED]


def test_the_excluded_cases_are_those_that_enqueue_nothing():
    assert sorted(soak_cases.ROUTE_EXCLUDED) == sorted(c["id"] for c in route_cases.CASES if not c["trace"])
    assert len(SOAKED) == len(route_cases.CASES) - len(soak_cases.ROUTE_EXCLUDED)


def route_case(c):
    """soak.Case of route case c: the buffers, the plan and the call of the seed-7 Prepared, the images of both"""
    p, q = (route_run.PREPARE[c["op"]](c, "cancel", seed=seed) for seed in SEEDS)
    try:
        bufs = []
        for a, b in zip(p.bufs, q.bufs):
            assert a.name == b.name and a.image.shape == b.image.shape and not a.planted and not b.planted
            bufs.append(soak.SoakBuf(a.name, a.dev, [a.image, b.image], [a.expect, b.expect]))
        assert any(not np.array_equal(a.image, b.image) for a, b in zip(p.bufs, q.bufs)), "the two datasets are the same bits"
        differ = any(not np.array_equal(a.expect, b.expect) for a, b in zip(p.bufs, q.bufs))
        assert differ or c["total"] == 2, "the two datasets expect the same bits"   # two ranks: see the module docstring
        if p.ws.nbytes:
            G, n = route_run.GUARD, p.ws.nbytes
            image = np.full(2 * G + n, 0xA5, dtype=np.uint8)
            bufs.append(soak.SoakBuf("workspace, front guard", p.ws.dev, [image, image], [image[:G], image[:G]], slice(0, G)))
            bufs.append(soak.SoakBuf("workspace, back guard", p.ws.dev, None, [image[:G], image[:G]], slice(G + n, 2 * G + n)))
            if p.ws_content is not None:
                bufs.append(soak.SoakBuf("workspace, the reduced vector", p.ws.dev, None,
                                         [p.ws_content.view(np.uint8), q.ws_content.view(np.uint8)], slice(G, G + n)))
    finally:
        q.close()
    return soak.Case(bufs, p.call, p.close), p


@pytest.mark.parametrize("c", SOAKED, ids=[c["id"] for c in SOAKED])
def test_route_soaked_under_uniform_load(c):
    with t.tuned(**c["keys"]):
        case, p = route_case(c)
        try:
            _, trace, _ = soak.soak(case, soak.R, "uniform")
            launches = p.launches()
        finally:
            case.close()
    route_run.check_trace(c, trace, launches)
