"""Every kernel route with its rank rows beyond 2^31 and 2^32 ELEMENTS of the pointer it is given.

The near tests keep every row within a few MiB, so `ranks + r * stride` (and `out + b * out_stride`,
`in + b * in_stride`, `shard + b * shard_stride`) computed in 32 bits would pass them all.  Here
every route case of tests/route_cases.py with at least two ranks and rows in device memory runs on
`cancel`, same n and tune keys, with its rows at the far stride of tests/far_arena.py:

    P >= 4   stride = roundup8(ceil(2^32 / (P-1))) + 136: the last row starts beyond 2^32 elements,
             middle rows beyond 2^31 elements = 2^32 bytes
    P == 2   stride = 2^31 + 136: row 1 beyond 2^31 elements = 2^32 bytes

and so do out / in / shard, in a region of their own (the library refuses them inside the rows'
footprint).  Of a grouped list only the middle bucket and its shard are far: the table carries
full pointers per bucket.  Everything is carved from ONE arena per module, at most 32 GiB, with 4 GiB
in front of the first row.

Per case: every payload row with 4 KiB of guard on both sides compared on the host, bit for bit,
with the oracle image; the launch trace the case's; then the sentinel is written back over those
windows and the WHOLE arena asserted sentinel on the device, in 1 GiB chunks — a stray write
anywhere in the 4 GiB below the rows or between two rows fails the test that made it.
tests/test_far_layout.py shows on the CPU that each 32-bit misreading of a row offset lands inside
the arena: a failed compare here, not a fault.
"""
import pytest

import far_arena
import route_cases
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import route_run  # noqa: E402  (needs torch)

pytestmark = pytest.mark.gpu
FAR = far_arena.far_cases(route_cases.CASES)


@pytest.fixture(scope="module")
def arena():
    nbytes = max(far_arena.route_layout(c).nbytes for c in FAR)
    a = far_arena.Arena(nbytes)   # an allocation failure is an error of the test, not a skip
    print(f"far arena: {nbytes} bytes ({nbytes / far_arena.GiB:.2f} GiB)")
    yield a
    a.close()


@pytest.mark.parametrize("c", FAR, ids=[c["id"] for c in FAR])
def test_route_far(c, arena):
    layout = far_arena.route_layout(c)
    place = route_run.Far(arena, layout)
    trace = t.launch_trace()
    with t.tuned(**c["keys"]):
        p = route_run.PREPARE[c["op"]](c, "cancel", place)
        assert not place.left, "every set of the layout is in use"
        try:
            with trace:
                p.call(torch.cuda.current_stream())
            torch.cuda.synchronize()
            launches = p.launches()
        finally:
            p.close()
        failed = []
        for check in (p.check, lambda: [b.far.wipe() for b in p.bufs if isinstance(b, route_run.FarBuf)],
                      arena.assert_sentinel):   # the arena is looked at, and left clean, whatever the compare said
            try:
                check()
            except AssertionError as e:
                failed.append(str(e))
    assert not failed, "; ".join(failed)
    for s in layout.sets:
        print(f"{s.name}: rows {s.stride} elements apart, the last at element {s.offset(s.rows - 1)}")
    route_run.check_trace(c, trace, launches)
