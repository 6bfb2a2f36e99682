"""Every kernel route on a side stream: captured into a graph and replayed, and eager behind late inputs.

tests/test_gpu_routes.py gives every call the default stream and ends in a device-wide synchronize,
so a launch enqueued on the wrong stream — the second launch of a two-launch route, an own-route
bucket of a mixed group, k_copy_ranks after an odd LO step count — passes it.  Here every entry of
tests/route_cases.py runs on `cancel` (bit for bit), same buffers and expected images
(tests/route_run.py), on a non-default torch.cuda.Stream() in two modes:

capture   an eager warm call on the stream (the capture loads no code), the buffers restored, the
          call captured with torch.cuda.graph(g, stream=s) — one linear branch on one stream.  The
          call returns OK under capture; the launch trace recorded DURING capture is the case's;
          after the capture and a synchronize every buffer and the workspace still hold the input
          image (a capture runs nothing); a replay gives the oracle image in every whole buffer;
          the inputs restored, a second replay gives it again (nothing survives in the workspace
          or the plan from replay to replay).  The one-rank cases that enqueue nothing capture
          an empty graph (torch warns about it); its replays must leave the inputs as they are.
late      every buffer holds the sentinel; on the side stream a few milliseconds of unrelated work
          (fills of a 1 GiB scratch tensor), then the copy of the input image into the buffers, then
          the call; only that stream is synchronized.  A launch that went to another stream meets
          sentinels and fails the whole-buffer compare.  Run on two streams in turn, which do not
          share a hardware queue, so a stray launch cannot hide behind the queue's own order.

The helper entry points allred_bf16_add, allred_bf16_add_masked, allred_tree_reduce and
allred_broadcast run in both modes too, on shapes with an odd tail.  allred_validate_device is not
here: it returns counts to the host and synchronizes by design (include/allred.h).
"""
import numpy as np
import pytest

import route_cases
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import route_run  # noqa: E402  (needs torch)
import test_gpu_parity as parity  # noqa: E402  (its fp32 reference of the bf16 add)

pytestmark = pytest.mark.gpu
DEV = route_run.DEV
FILLS = 8   # 1 GiB fills in front of the late inputs: a few milliseconds against microseconds for the call


@pytest.fixture(scope="module")
def scratch():
    s = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    yield s
    del s
    torch.cuda.empty_cache()


def run_capture(p, expected_trace):
    """p: a route_run.Prepared (or anything with its face); returns the trace recorded during capture"""
    s = torch.cuda.Stream()
    p.stage()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # an eager call first: nothing is loaded inside the capture
        p.call(s)
    s.synchronize()
    p.check()
    p.restore()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    trace = t.launch_trace()
    with torch.cuda.graph(g, stream=s):
        with trace:
            p.call(s)   # raises unless the library returned ALLRED_OK
    torch.cuda.synchronize()
    assert trace.kernels == expected_trace and trace.count == len(expected_trace)
    p.check_input()     # a capture runs nothing
    for _ in range(2):
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        p.check()
        p.restore()
        torch.cuda.synchronize()
    del g
    return trace


def run_late(p, scratch):
    """Twice, on two streams made one after the other: streams share the few hardware queues, and work
    that went to another stream but landed in the queue of the side stream would run behind the inputs
    after all.  Two consecutive streams do not share a queue, so no stray launch hides behind both."""
    p.stage()
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        p.sentinel()
        torch.cuda.synchronize()
        trace = t.launch_trace()
        with torch.cuda.stream(s):
            for i in range(FILLS):
                scratch.fill_(i)
            p.restore()          # the inputs land on s, behind the fills
            with trace:
                p.call(s)
        s.synchronize()          # this stream only
        p.check()
        torch.cuda.synchronize()
    return trace


@pytest.mark.parametrize("mode", ["capture", "late"])
@pytest.mark.parametrize("c", route_cases.CASES, ids=[c["id"] for c in route_cases.CASES])
def test_route_on_a_side_stream(c, mode, scratch):
    with t.tuned(**c["keys"]):
        p = route_run.PREPARE[c["op"]](c, "cancel")
        try:
            trace = run_capture(p, c["trace"]) if mode == "capture" else run_late(p, scratch)
            launches = p.launches()
        finally:
            p.close()
    route_run.check_trace(c, trace, launches)


# ------------------------------------------------------------------ the helper entry points
class Helper:
    """Prepared's face for a call on plain 1-D / row buffers: route_run.Buf images, one call"""

    def __init__(self, bufs, call):
        self.bufs, self.call = bufs, call

    def stage(self):
        for b in self.bufs:
            b.stage()

    def restore(self):
        for b in self.bufs:
            b.restore()

    def sentinel(self):
        for b in self.bufs:
            b.sentinel()

    def check(self):
        for b in self.bufs:
            b.check()

    def check_input(self):
        for b in self.bufs:
            b.check_input()


def vector(name, bits, lead=0):
    """a 1-D buffer of `bits` behind `lead` sentinel elements, in a row wide enough for a guard behind it"""
    b = route_run.Buf(name, 1, (lead + bits.size + 7) // 8 * 8 + route_run.GUARD)   # the payload 16-byte aligned
    b.image[1, lead:lead + bits.size] = bits
    return b.upload()


def finite(rng, n):
    x = rng.integers(0, 0x10000, n).astype(np.uint16)
    x[(x & 0x7F80) == 0x7F80] &= 0x807F   # no NaN / Inf: the comparison is bit for bit
    return x


def helper_add(offset):
    """allred_bf16_add: 1013 elements from an aligned pointer (k_add, then k_add_scalar over the tail of 5: two
    launches) or from one element in (k_add_scalar alone)"""
    n, rng = 1013, np.random.default_rng(5 + offset)
    a, b = finite(rng, n), finite(rng, n)
    dst, src = vector("dst", a, offset), vector("src", b, offset)
    dst.rows()[0, offset:offset + n] = parity.torch_add_ref(a, b)
    call = lambda s: t.bf16_add(dst.ptr + 2 * offset, src.ptr + 2 * offset, n, s)   # noqa: E731
    return Helper([dst, src], call), ["k_add_scalar"] if offset else ["k_add", "k_add_scalar"]


def helper_add_masked():
    """allred_bf16_add_masked: blocks of 40 elements, the mask's last block set"""
    blk, mask, rng = 40, 0x9900009999000099, np.random.default_rng(3)
    a, b = finite(rng, 64 * blk), finite(rng, 64 * blk)
    dst, src = vector("dst", a), vector("src", b)
    summed = parity.torch_add_ref(a, b)
    for k in range(64):
        if (mask >> k) & 1:
            dst.rows()[0, k * blk:(k + 1) * blk] = summed[k * blk:(k + 1) * blk]
    return Helper([dst, src], lambda s: t.bf16_add_masked(dst.ptr, src.ptr, mask, blk, s)), ["k_add_segs"]


def helper_tree_reduce():
    """allred_tree_reduce: 64 ranks x 261 vectors (odd, no whole tile): tree 0 = the LO value of rank 0"""
    total, side, n = 64, 8, 8 * 261
    rows = route_run.NEAR.rank_rows("ranks", route_run.dataset("cancel", total, n))
    out = vector("out", np.full(n, route_run.SENT, dtype=np.uint16))
    out.rows()[0, :n] = route_run.reference("cancel", "lo", t.SWING, side, total, n)[0]
    call = lambda s: t.tree_reduce(rows.ptr, rows.width, n, t.SWING, side, total, out.ptr, s)   # noqa: E731
    return Helper([rows, out], call), ["k_tree<64, false>"]


def helper_broadcast():
    """allred_broadcast: 261 vectors to every one of 64 rows"""
    total, n = 64, 8 * 261
    rows = route_run.NEAR.rank_rows("ranks", route_run.dataset("cancel", total, n))
    bits = np.random.default_rng(11).integers(0, 0x10000, n).astype(np.uint16)   # any pattern: a copy
    src = vector("src", bits)
    rows.rows()[:, :n] = bits[None, :]
    return Helper([rows, src], lambda s: t.broadcast(rows.ptr, rows.width, n, total, src.ptr, s)), ["k_broadcast"]


HELPERS = {"add": lambda: helper_add(0), "add-unaligned": lambda: helper_add(1), "add-masked": helper_add_masked,
           "tree-reduce": helper_tree_reduce, "broadcast": helper_broadcast}


@pytest.mark.parametrize("mode", ["capture", "late"])
@pytest.mark.parametrize("name", list(HELPERS))
def test_helper_on_a_side_stream(name, mode, scratch):
    p, expected = HELPERS[name]()
    trace = run_capture(p, expected) if mode == "capture" else run_late(p, scratch)
    print(f"{name}: {trace.kernels} grids {trace.grids}")
    assert trace.kernels == expected and trace.count == len(expected)
