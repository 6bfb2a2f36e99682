"""Every route of the peer-window (N-GPU) kernels (tests/peer_cases.py) on hard inputs.

Per case and dataset (tests/hard_inputs.py: `cancel`, whose result depends on the order of the
adds, and `nonfinite`):
  1. the bucket or the rank rows sit in a sentinel-filled buffer that is compared WHOLE: 256 guard
     elements in front of and behind a flat bucket, a guard row in front of and behind rank rows;
     the workspace between two 256-byte guards.  Every local row of a result must equal the
     expected row;
  2. cancel: 0 differing elements, bit for bit — the cross-GPU sum is "owner first, then the ranks
     ascending, fp32, one rounding", and with three or more GPUs another order gives other bits
     (tests/test_peer_table.py pins that these inputs show it).  nonfinite: bit-exact outside the
     planted columns; inside them NaN as a class, +Inf / -Inf as bits, against the oracle AND
     against the answer hard_inputs states;
  3. the launch trace of the rank's call or calls is the case's expected list of kernel names: a
     route that silently fell back to another form fails here;
  4. the peer status word is 0 at the end (no wait timed out, flags and windows uncached).
The flat programs take hard_inputs.<kind>(W, n); the hierarchical ones one draw over all W * local
rows dealt to the GPUs in order, so +B and -B mostly sit on different GPUs and the partials that
cross still hold B.  Consecutive calls of a case take different draws (a stale hand-off word of
the call before would be another value).  Expected values are the oracle compositions of
tests/test_gpu_peer.py: the tree of local rank 0, then mem_2D; test_dist_host.expected for the
scheduled programs.

W = 1 runs in this process (the tree order of every k_hier_ws / k_hier_x2 instance and the mem_2D
forms); W = 2, 4, 8 are processes sharing the GPU.  W = 2 checks transport and bit patterns only
(two addends commute); the add order is checked at W = 4 and 8.
"""
import functools

import numpy as np
import pytest

import hard_inputs
import oracle
import peer_cases
import tenstorrentallreduce_amd as t
import test_dist_host as tdh
import test_gpu_peer as tgp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENT = 0xA5A5
GUARD = 256   # elements around a flat bucket; bytes in front of and behind the workspace
SEED = 7
KINDS = ("cancel", "nonfinite")
# every name a world's table must have put into a checked trace
HIER_NAMES = {f"k_hier_ws<{a}, {cw}>" for a, cw in peer_cases.HIER_WS} | set(peer_cases.HIER_X2)
ALL_NAMES = HIER_NAMES | set(peer_cases.PEER_KERNELS)


# ------------------------------------------------------------------ data and references (computed once, read-only)
def frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def dataset(kind, world, local, n, seed):
    """(world, local, n): one draw over all world * local rows, dealt to the GPUs in order"""
    return frozen(getattr(hard_inputs, kind)(world * local, n, seed).reshape(world, local, n))


@functools.lru_cache(maxsize=None)
def mem_reference(kind, world, local, n, seed):
    """the tree of local rank 0 on every GPU (the row itself for one local rank), then mem_2D's
    owner-first sum of the partials: the row every local rank of GPU r ends with, (world, n)"""
    partials = []
    for d in dataset(kind, world, local, n, seed):
        loc = [x.copy() for x in d]
        if local > 1:
            oracle.allreduce("lo", 1, 8, loc, local)
        partials.append(loc[0])
    oracle.allreduce("mem", 0, 1, partials, world)
    return frozen(np.stack(partials))


@functools.lru_cache(maxsize=None)
def dist_reference(kind, variant, algo, world, local, chans, n, seed):
    data = [[row.copy() for row in d] for d in dataset(kind, world, local, n, seed)]
    want = tdh.expected(variant, algo, world, local, data, chans)
    return frozen(np.stack([np.stack(w) for w in want]))   # (world, local, n)


# ------------------------------------------------------------------ buffers
class Rows:
    """`local` rows of n elements in a sentinel-filled buffer: GUARD elements around one row, a guard
    row around several"""

    def __init__(self, rows, dev):
        self.local, self.n = rows.shape
        self.guard = GUARD if self.local == 1 else self.n
        image = np.full(2 * self.guard + rows.size, SENT, dtype=np.uint16)
        image[self.guard:self.guard + rows.size] = rows.reshape(-1)
        self.dev = torch.from_numpy(image.view(np.int16)).to(dev)

    @property
    def ptr(self):
        return self.dev.data_ptr() + 2 * self.guard

    def check(self, kind, want, total):
        """want: the (local, n) expected rows; total: the rows of the draw (where the planted columns are)"""
        got = self.dev.cpu().numpy().view(np.uint16)
        g, size = self.guard, self.local * self.n
        assert (got[:g] == SENT).all(), f"{int((got[:g] != SENT).sum())} elements of the guard in front were written"
        assert (got[g + size:] == SENT).all(), f"{int((got[g + size:] != SENT).sum())} elements of the guard behind were written"
        rows = got[g:g + size].reshape(self.local, self.n)
        if kind == "cancel":
            differing = int((rows != want).sum())
            assert differing == 0, f"{differing} differing elements of {size}"
            return
        # nonfinite: rows with the same expected row must hold the same bits (a NaN's payload
        # included: every local row is written from one value); each distinct row by class
        checked = {}
        for i in range(self.local):
            first = checked.setdefault(want[i].tobytes(), i)
            if first == i:
                hard_inputs.check_nonfinite(rows[i], want[i], total, self.n)
            else:
                differing = int((rows[i] != rows[first]).sum())
                assert differing == 0, f"row {i} differs from row {first} in {differing} elements"


class Workspace:
    def __init__(self, nbytes, dev):
        self.nbytes = nbytes
        self.dev = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=dev) if nbytes else None

    @property
    def ptr(self):
        return self.dev.data_ptr() + GUARD if self.nbytes else None

    def check(self):
        if self.nbytes:
            got = self.dev.cpu().numpy()
            assert (got[:GUARD] == 0xA5).all(), "the guard in front of the workspace was written"
            assert (got[GUARD + self.nbytes:] == 0xA5).all(), "the guard behind the workspace was written"


# ------------------------------------------------------------------ one case
def max_elems(world):
    """windows that hold every shape of the table (a LO program needs half a window per bucket)"""
    return 2 * max(peer_cases.elems(c, world) for c in peer_cases.CASES if world in c["worlds"])


def run_case(peer, c, kind, world, rank, dev, shared, barrier):
    """the case's calls under a launch trace, then every buffer whole; returns the trace.  `barrier`
    brings the ranks in step right before the calls: the kernels' waits for a peer are bounded."""
    n, local, k, prog = peer_cases.elems(c, world), c["local"], c["knobs"], c["program"]
    peer.set_oneshot_max(k["oneshot_max"])
    peer.set_mem_ll_max(k["mem_ll_max"])
    peer.set_hier_ll(k["hier_ll"])
    peer.set_lo_ll_max(k["lo_ll_max"])
    peer.set_sched_push(k["sched_push"])
    # the one-kernel forms wait across processes: every process's grid must be resident at once
    peer.set_max_groups((256 // world if shared else 0) if k["max_groups"] == peer_cases.FULL else k["max_groups"])
    s = torch.cuda.current_stream()
    seeds = [SEED + rep for rep in range(c["calls"])]
    bufs = [Rows(dataset(kind, world, local, n, seed)[rank], dev) for seed in seeds]
    trace = t.launch_trace()
    if prog.startswith("dist_"):
        variant = prog[5:]
        side, total = tdh.GRIDS[world]
        desc = t.dist_desc(c["algo"], t.BO if variant == "bo" else t.LO, 1 if c["algo"] >= 2 else side, total, n,
                           local_ranks=local, local_side=2, local_algo=t.SWING, channels=c["channels"])
        ws = Workspace(t.dist_workspace_bytes(desc), dev)
        front = Rows(np.zeros((1, n), dtype=np.uint16), dev)   # mem_2D of zeros: it reads every rank's window
        torch.cuda.synchronize()
        barrier()
        with trace:
            peer.allreduce(front.ptr, n, s)
            for b in bufs:
                peer.dist_allreduce(desc, b.ptr, ws.ptr, s)
        torch.cuda.synchronize()
        front.check("cancel", np.zeros((1, n), dtype=np.uint16), world)
        wants = [dist_reference(kind, variant, c["algo"], world, local, c["channels"], n, seed)[rank] for seed in seeds]
    else:
        ws = Workspace(2 * n if local > 1 else 0, dev)
        torch.cuda.synchronize()
        barrier()
        with t.tuned(**c["keys"]), trace:
            for b in bufs:
                if prog == "hier_x2":
                    peer.allreduce_pipelined2(b.ptr, n, s)
                else:
                    peer.allreduce(b.ptr, n, s, local, 8 if local > 1 else 1, t.SWING, ws.ptr)
            if prog == "hier_x2":
                peer.allreduce_pipelined2(None, n, s)
        torch.cuda.synchronize()
        wants = [np.broadcast_to(mem_reference(kind, world, local, n, seed)[rank], (local, n)) for seed in seeds]
    assert trace.kernels == c["trace"], f"trace {trace.kernels} (grids {trace.grids}), expected {c['trace']}"
    assert trace.count == len(c["trace"])
    for call, (b, want) in enumerate(zip(bufs, wants)):
        try:
            b.check(kind, want, world * local)
        except AssertionError as e:
            raise AssertionError(f"call {call}: {e}") from None
    ws.check()
    return trace.kernels


def run_table(peer, world, rank, dev, shared, fence, barrier=lambda: None):
    """every case of the table for this world; returns (failures, names traced in cases that passed)"""
    fails, seen = [], set()
    for c in peer_cases.CASES:
        if world not in c["worlds"] or fence not in c["peer_fence"][world]:
            continue
        for kind in KINDS:
            try:
                seen |= set(run_case(peer, c, kind, world, rank, dev, shared, barrier))
            except AssertionError as e:
                fails.append((c["id"], kind, str(e)[:600]))
            if peer.status() & t.PEER_TIMEOUT and not any(f[0] == "timeout" for f in fails):
                fails.append(("timeout", c["id"], kind))   # the first case whose peer waits gave up
    print(f"rank {rank} of {world}, peer_fence {fence}: checked traces held {sorted(seen)}")
    return fails, seen


# ------------------------------------------------------------------ W = 1, in this process
def test_peer_table_single_gpu():
    """every hier, hier_x2 and mem case at W = 1: the tree order of every k_hier_ws instance — the
    two-tiles-ahead ones included — and of k_hier_x2 on `cancel`, the mem_2D forms' indexing"""
    peer = t.Peer(1, 0, 0, max_elems(1))
    peer.connect([peer.handle()])
    try:
        fails, seen = run_table(peer, 1, 0, "cuda:0", False, 0)
        assert fails == [], fails
        mem = {name for form in peer_cases.MEM_FORMS.values() for name in form[1]} - {"k_copy_ranks"}
        assert seen >= HIER_NAMES | mem, (HIER_NAMES | mem) - seen
        assert peer.status() == 0
    finally:
        peer.set_hier_ll(0)
        peer.set_max_groups(0)
        peer.close()


# ------------------------------------------------------------------ W processes
def table_worker(rank, world, port, q, devs=None, tunes=None):
    """the whole table for this world, one process per rank (every rank on device 0, or devs[rank])"""
    try:
        import os
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        devs, dev, shared = tgp.placement(rank, world, devs, tunes)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        peer = t.Peer(world, rank, devs[rank], max_elems(world))
        handles = [None] * world
        dist.all_gather_object(handles, peer.handle())
        peer.connect(handles)
        fence = int((tunes or {}).get("peer_fence", 0))
        assert t.tune("peer_fence") == fence
        fails, seen = run_table(peer, world, rank, dev, shared, fence, dist.barrier)
        if ALL_NAMES - seen:
            fails.append(("never in a checked trace", sorted(ALL_NAMES - seen)))
        peer.set_hier_ll(0)
        peer.set_max_groups(0)
        status = peer.status()
        dist.barrier()
        peer.close()
        dist.destroy_process_group()
        q.put((rank, fails, status))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, [("exception", repr(e), traceback.format_exc())], -1))


WORLDS = [(world, fence) for world in peer_cases.MULTI for fence in peer_cases.PEER_FENCE[world]]


@pytest.mark.parametrize("world,fence", WORLDS, ids=[f"{w}-{'fenced' if f else 'relaxed'}" for w, f in WORLDS])
def test_peer_table_multi_process_one_gpu(world, fence):
    tgp.run_world(table_worker, world, 240, tunes={"peer_fence": fence} if fence else {})
