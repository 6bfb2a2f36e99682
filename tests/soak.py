"""The replay soak (helper, no tests): one captured call, R replays back to back with no host
synchronisation between them, consecutive replays on DIFFERENT data, under a memory load.

Every other GPU test runs a kernel once, on an idle chip, and compares afterwards.  That settles what
a kernel computes, not whether its counted waits and its one cross-workgroup hand-off are ordered: an
early read of an LDS-DMA tile, or a stale read of another workgroup's partial, is right whenever the
data happens to have landed, and it has on an idle chip.  Here

    soak(case, R, load)   case.bufs   [SoakBuf]: a device (or pinned host) buffer with two staged input
                                      images and two expected images, all on the device
                          case.call   call(stream): the library call
    replay r              every buffer restored from staged[r % 2] by stream-ordered device copies;
                          g.replay(); (buf != want[r % 2]).sum() of every buffer — whole, guards and
                          gaps included — into bad[r, buffer], a device tensor.  Two datasets from
                          different seeds alternate, so what replay r - 1 left behind, in a buffer, in
                          LDS or in a cache, is the WRONG value in replay r.
    after replay R        one synchronise; bad must be all zero (the first replay, the buffer and the
                          count are named).

Soak data holds nothing that is compared by class (no NaN in a compared fp32 image): one integer
compare decides.

Load(mode): `idle` (nothing), `uniform` (k_soak_load of tests/soak_control.hip on a grid of four
workgroups per CU) or `uneven` (32 workgroups) on a stream of its own, made right after the soak's
stream: consecutive streams do not share a hardware queue.  Two launches are kept outstanding
(Event.query()) from before the first replay until after the last compare; timed events prove it, and
the soak fails with "no load" when they do not.

ONE LOAD LAUNCH: a read-modify-write of one 16-byte vector per thread and iteration, start advancing
through a 1 GiB buffer, sized to about 1 ms.  Measured once on an MI355X, as the first launch of a soak
(tests/test_gpu_soak_control.py prints it with every run; profiles/soak_control.json has the sweep):
    uniform  1024 workgroups (4 per CU) x  600 iterations: 1.088 ms  (256: 0.41 ms, 1024: 1.69 ms)
    uneven     32 workgroups            x 2048 iterations: 1.027 ms  (1024: 0.34 ms, 4096: 1.86 ms)
"""
import ctypes
import functools
import os

import numpy as np
import torch

import tenstorrentallreduce_amd as t

DEV = "cuda:0"
R = 256                      # 0.96^256 = 3e-5: what a protocol that is stale 4 % of the time survives with
R_MIN = 64
LOAD_BYTES = 1 << 30
LOAD_ITERS = {"uniform": 600, "uneven": 2048}          # iterations per launch, sized to about 1 ms
LOAD_MEASURED_MS = {"uniform": 1.088, "uneven": 1.027}   # one launch on an MI355X (profiles/soak_control.json)
LOAD_GRID = {"uniform": lambda: 4 * torch.cuda.get_device_properties(0).multi_processor_count, "uneven": lambda: 32}
MODES = ("idle", "uniform", "uneven")


@functools.lru_cache(maxsize=None)
def control():
    """a missing library is an error: build() makes it with the package"""
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(t.__file__)), "build", "libsoak_control.so"))
    lib.soak_load.restype = ctypes.c_int
    lib.soak_load.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.ticket_sum.restype = ctypes.c_int
    lib.ticket_sum.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                               ctypes.c_void_p]
    return lib


_scratch = None


def scratch():
    """the load's 1 GiB, made once per process"""
    global _scratch
    if _scratch is None:
        _scratch = torch.zeros(LOAD_BYTES, dtype=torch.uint8, device=DEV)
    return _scratch


def as_int(a):
    """a numpy array as a torch tensor of a signed integer type of the same width (bits kept)"""
    a = np.array(a, order="C")   # a copy: the references' arrays are read-only
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]))


class SoakBuf:
    """One buffer of a soak.  dev: the tensor the call reads or writes (a device tensor, or pinned host
    memory).  staged: two host images to restore from, or None — never restored (a workspace the call keeps
    in order itself).  want: two host images the buffer must equal, whole, after every replay.  window: a
    slice of the flattened buffer to compare instead of all of it (the 64 counter bytes of the norm
    workspace; the rest of it is unspecified)."""

    def __init__(self, name, dev, staged, want, window=None):
        self.name, self.dev, self.window = name, dev, window
        flat = dev.view(-1)
        self.staged = None if staged is None else [as_int(s).view(-1).to(DEV) for s in staged]
        self.want = [as_int(w).view(-1).to(DEV) for w in want]
        for x in (self.staged or []):
            assert x.dtype == flat.dtype and x.numel() == flat.numel(), name
        for x in self.want:
            assert x.dtype == flat.dtype and x.numel() == (flat[window] if window else flat).numel(), name
        self.on_host = not dev.is_cuda
        self.bounce = torch.empty(flat.numel(), dtype=flat.dtype, device=DEV) if self.on_host else None

    def restore(self, k):
        if self.staged is not None:
            self.dev.view(-1).copy_(self.staged[k], non_blocking=True)

    def differing(self, k):
        """a 0-d device tensor: elements that differ from want[k]; enqueued on the current stream"""
        got = self.dev.view(-1)
        if self.on_host:
            self.bounce.copy_(got, non_blocking=True)
            got = self.bounce
        if self.window is not None:
            got = got[self.window]
        return (got != self.want[k]).sum()


class Case:
    def __init__(self, bufs, call, close=None):
        self.bufs, self.call, self._close = bufs, call, close

    def close(self):
        if self._close:
            self._close()


class Load:
    """with Load(mode) as load: ... load.pump() ...; see the module docstring"""

    def __init__(self, mode):
        assert mode in MODES, mode
        self.mode = mode
        self.stream = torch.cuda.Stream()          # made right after the soak's stream (soak() does so)
        self.launches, self.outstanding, self.first, self.last_end, self.start = 0, [], None, None, 0

    def launch(self):
        grid, iters = LOAD_GRID[self.mode](), LOAD_ITERS[self.mode]
        begin = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            begin.record()
            rc = control().soak_load(scratch().data_ptr(), LOAD_BYTES // 16, self.start, iters, grid, self.stream.cuda_stream)
            end.record()
        assert rc == 0, f"soak_load returned {rc}"
        self.start = (self.start + grid * 256 * iters) % (LOAD_BYTES // 16)
        self.launches += 1
        if self.first is None:
            self.first = (begin, end)
        self.last_end = end
        self.outstanding.append(end)

    def pump(self):
        """two launches outstanding: every finished one is replaced"""
        if self.mode == "idle":
            return
        self.outstanding = [e for e in self.outstanding if not e.query()]
        while len(self.outstanding) < 2:
            self.launch()

    def __enter__(self):
        if self.mode != "idle":
            scratch()
            torch.cuda.synchronize()
            self.pump()
        return self

    def __exit__(self, *exc):
        self.stream.synchronize()
        return False

    def check(self, first_replay, last_compare):
        """after the final synchronise: the first launch began before the first replay and the last one ended
        after the last compare.  Returns (launches, ms of the first launch)."""
        if self.mode == "idle":
            return 0, 0.0
        lead = self.first[0].elapsed_time(first_replay)       # ms from the first launch's begin to the first replay
        tail = last_compare.elapsed_time(self.last_end)       # ms from the last compare to the last launch's end
        assert lead >= 0 and tail >= 0, f"no load: the first launch began {lead:.3f} ms before the first replay, " \
                                        f"the last ended {tail:.3f} ms after the last compare ({self.launches} launches)"
        return self.launches, self.first[0].elapsed_time(self.first[1])


def capture(case, s):
    """one eager warm call on s (the capture loads no code), then the call captured once on s: one linear
    branch on one stream.  Returns (graph, the launch trace recorded during the capture)."""
    for b in case.bufs:
        b.restore(0)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        case.call(s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    trace = t.launch_trace()
    with torch.cuda.graph(g, stream=s):
        with trace:
            case.call(s)
    torch.cuda.synchronize()
    return g, trace


def soak(case, replays, mode, expect_clean=True):
    """Returns (bad, trace, report): bad the (replays, buffers) host array of differing-element counts, trace
    the launch trace of the capture, report a dict for the log.  expect_clean: assert that bad is all zero."""
    assert replays >= R_MIN
    s = torch.cuda.Stream()
    load = Load(mode)            # its stream is made right after s
    g, trace = capture(case, s)
    bad = torch.zeros((replays, len(case.bufs)), dtype=torch.int64, device=DEV)
    first_replay = torch.cuda.Event(enable_timing=True)
    last_compare = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with load:
        with torch.cuda.stream(s):
            if mode != "idle":
                s.wait_event(load.first[0])    # the first load launch is under way (or done) before the first replay
            first_replay.record()
            for r in range(replays):
                k = r % 2
                for b in case.bufs:
                    b.restore(k)
                g.replay()
                for i, b in enumerate(case.bufs):
                    bad[r, i] = b.differing(k)
                load.pump()
            last_compare.record()
        while not last_compare.query():        # the host only feeds the load; the soak's stream runs on its own
            load.pump()
    torch.cuda.synchronize()
    launches, load_ms = load.check(first_replay, last_compare)
    host = bad.cpu().numpy()
    report = {"mode": mode, "replays": replays, "soak_ms": round(first_replay.elapsed_time(last_compare), 3),
              "load_launches": launches, "load_launch_ms": round(load_ms, 3), "differing": int(host.sum())}
    print(f"soak: {report}; kernels {trace.kernels}")
    del g
    if expect_clean and host.any():
        r, i = np.argwhere(host)[0]
        assert False, (f"{int(host.sum())} differing elements over {replays} replays under {mode} load; first in replay {r}, "
                       f"buffer {case.bufs[i].name!r}: {int(host[r, i])} differing; replays that differ: "
                       f"{np.flatnonzero(host.any(axis=1)).tolist()[:16]}")
    return host, trace, report
