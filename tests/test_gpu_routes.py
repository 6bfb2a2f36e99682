"""Every kernel route of the one-GPU engine (tests/route_cases.py) on hard inputs.

Per case and dataset (tests/hard_inputs.py: `cancel`, whose result depends on the order of the
adds, and `nonfinite`):
  1. every buffer the call may touch is filled with a sentinel and compared WHOLE: the rank rows at
     preferred_rank_stride with a guard row in front of row 0, the stride skew and a guard row
     behind the last rank; the workspace between two 256-byte guards; out / in / shard buffers
     with a gap behind every row and guard rows.  The expected image is the CPU oracle where the
     operation defines a result, the input bits where it only reads (a fused reduce-scatter in
     place keeps every block it does not own), the sentinel everywhere else;
  2. cancel: 0 differing elements, bit for bit.  nonfinite: bit-exact outside the planted columns;
     inside them NaN as a class, +Inf / -Inf as bits, on every rank that receives the column — held
     against the oracle AND against the answer hard_inputs states;
  3. the launch trace of the call is the case's expected list of kernel names, and its count is
     plan.launches (the grouped calls: the dry launch count) under the same tune keys.
The schedule-form MEM plan's workspace holds the reduced vector; its content is compared too.
"""
import functools

import numpy as np
import pytest

import hard_inputs
import oracle
import route_cases
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5A5
GUARD = 256   # bytes in front of and behind the workspace; elements around 1-D buffers
GAP = 8       # elements behind every row of an out / in / shard buffer
SEED = 7
KINDS = ("cancel", "nonfinite")
VARIANT_NAME = {route_cases.BO: "bo", route_cases.LO: "lo", route_cases.MEM: "mem"}


# ------------------------------------------------------------------ data and references (computed once, read-only)
def frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def dataset(kind, total, n):
    return frozen(getattr(hard_inputs, kind)(total, n, SEED))


@functools.lru_cache(maxsize=None)
def reference(kind, name, algo, side, total, n, acc16=False):
    """the oracle's allreduce of dataset(kind, total, n): (total, n) uint16"""
    want = [r.copy() for r in dataset(kind, total, n)]
    oracle.allreduce(name, algo, side, want, total, acc16=acc16)
    return frozen(np.stack(want))


def columns(kind, total, n):
    """(column, class) a result of this dataset is compared by class in: none for cancel"""
    return hard_inputs.nonfinite_columns(total, n) if kind == "nonfinite" else []


# ------------------------------------------------------------------ buffers
class Buf:
    """A sentinel-filled 2-D image on the device (or in pinned host memory) with guard rows around
    `rows` payload rows; `expect` starts as the input image and the case writes its results into it;
    `planted` lists the (row, column, class) compared by class instead of by bits."""

    def __init__(self, name, rows, width, host=False):
        self.name = name
        self.image = np.full((rows + 2, width), SENT, dtype=np.uint16)
        self.width, self.host, self.planted, self.dev, self.expect = width, host, [], None, None

    def upload(self):
        self.expect = self.image.copy()
        flat = torch.from_numpy(self.image.view(np.int16).copy())
        self.dev = flat.pin_memory() if self.host else flat.to(DEV)
        return self

    @property
    def ptr(self):   # row 0 of the payload: one guard row in
        return self.dev.data_ptr() + 2 * self.width

    def rows(self):  # the payload rows of the expected image
        return self.expect[1:-1]

    def plant(self, row, cols, offset=0, width=None):
        """the planted columns falling into [offset, offset + width) of payload row `row`"""
        for c, cls in cols:
            if offset <= c < offset + (self.width if width is None else width):
                self.planted.append((row + 1, c - offset, cls))

    def check(self):
        got = (self.dev if self.host else self.dev.cpu()).numpy().view(np.uint16)
        exact = np.ones(got.shape, dtype=bool)
        for r, c, cls in self.planted:
            exact[r, c] = False
            known, g, w = hard_inputs.NONFINITE_CLASSES[cls], int(got[r, c]), int(self.expect[r, c])
            where = f"{self.name} row {r - 1} column {c} ({cls})"
            if known == "nan":
                assert hard_inputs.is_nan(w), f"oracle, {where}: 0x{w:04X} is no NaN"
                assert hard_inputs.is_nan(g), f"{where}: 0x{g:04X} is no NaN"
            else:
                assert w == known, f"oracle, {where}: 0x{w:04X}, not 0x{known:04X}"
                assert g == known, f"{where}: 0x{g:04X}, not 0x{known:04X}"
        differing = int((got[exact] != self.expect[exact]).sum())
        print(f"{self.name}: {differing} differing elements of {got.size}, {len(self.planted)} compared by class")
        if differing:
            r, c = np.argwhere((got != self.expect) & exact)[0]
            assert False, (f"{self.name}: {differing} differing elements; first at row {r - 1} column {c}: "
                           f"0x{int(got[r, c]):04X}, expected 0x{int(self.expect[r, c]):04X}")


def rank_rows(name, data, host=False):
    total, n = data.shape
    b = Buf(name, total, t.preferred_rank_stride(n), host)
    b.image[1:total + 1, :n] = data
    return b.upload()


def side_rows(name, total, blk, fill=None):
    """an out / in / shard buffer: `total` rows of blk elements, GAP elements behind each"""
    b = Buf(name, total, blk + GAP)
    if fill is not None:
        b.image[1:total + 1, :blk] = fill
    return b.upload()


class Workspace:
    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.dev = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=DEV) if nbytes else None

    @property
    def ptr(self):
        return self.dev.data_ptr() + GUARD if self.nbytes else None

    def check(self, content=None):
        if not self.nbytes:
            return
        got = self.dev.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all(), "the guard in front of the workspace was written"
        assert (got[GUARD + self.nbytes:] == 0xA5).all(), "the guard behind the workspace was written"
        return got[GUARD:GUARD + self.nbytes]


def owner_blocks(a, total, n):
    blk = n // total
    return np.stack([a[b, b * blk:(b + 1) * blk] for b in range(total)])


def stream():
    return torch.cuda.current_stream()


# ------------------------------------------------------------------ the operations
def run_allreduce(c, kind, trace):
    total, n = c["total"], c["n"]
    data = dataset(kind, total, n)
    want = reference(kind, VARIANT_NAME[c["variant"]], c["algo"], c["side"], total, n, c["acc"] == route_cases.BF16)
    rows = rank_rows("ranks", data, c["host"])
    plan = t.Plan(c["algo"], c["variant"], c["side"], n, total, c["exec"], mem_accum=c["acc"])
    ws = Workspace(plan.workspace_bytes)
    with trace:
        plan.execute(rows.ptr, rows.width, ws.ptr, stream())
    torch.cuda.synchronize()
    launches = plan.launches
    plan.close()
    rows.rows()[:, :n] = want
    for r in range(total):
        rows.plant(r, columns(kind, total, n), 0, n)
    rows.check()
    inside = ws.check()
    if c["variant"] == route_cases.MEM and c["exec"] == route_cases.STEPS and kind == "cancel":
        assert np.array_equal(inside.view(np.uint16), want[0]), "the workspace holds the reduced vector"
    return launches


def run_reduce_scatter(c, kind, trace):
    total, n, compact = c["total"], c["n"], c["op"] == "rs_compact"
    blk = n // total
    data = dataset(kind, total, n)
    want = owner_blocks(reference(kind, "bo", c["algo"], c["side"], total, n), total, n)
    rows = rank_rows("ranks", data)
    out = side_rows("out", total, blk)
    plan = t.Plan(c["algo"], route_cases.BO, c["side"], n, total, route_cases.FUSED)
    with trace:
        if compact:
            plan.reduce_scatter(rows.ptr, rows.width, out.ptr, out.width, stream=stream())
        else:
            plan.reduce_scatter(rows.ptr, rows.width, stream=stream())
    torch.cuda.synchronize()
    plan.close()
    for b in range(total):   # block b to rank b's row, or to out row b; everything else keeps its bits
        if compact:
            out.rows()[b, :blk] = want[b]
            out.plant(b, columns(kind, total, n), b * blk, blk)
        else:
            rows.rows()[b, b * blk:(b + 1) * blk] = want[b]
            rows.plant(b, [(col, cls) for col, cls in columns(kind, total, n) if col // blk == b])
    rows.check()
    out.check()
    return len(c["trace"])


def run_all_gather(c, kind, trace):
    """a copy: every 16-bit pattern must arrive as it is, so nothing is compared by class"""
    total, n, from_in = c["total"], c["n"], c["op"] == "ag_from_in"
    blk = n // total
    data = dataset(kind, total, n)
    rows = rank_rows("ranks", data)
    src = np.stack([data[(b + 1) % total, b * blk:(b + 1) * blk] for b in range(total)])   # not the owners' blocks
    din = side_rows("in", total, blk, src)
    plan = t.Plan(c["algo"], route_cases.BO, c["side"], n, total, route_cases.FUSED)
    with trace:
        if from_in:
            plan.all_gather(rows.ptr, rows.width, din.ptr, din.width, stream=stream())
        else:
            plan.all_gather(rows.ptr, rows.width, stream=stream())
    torch.cuda.synchronize()
    plan.close()
    rows.rows()[:, :n] = (src if from_in else owner_blocks(data, total, n)).reshape(-1)[None, :]
    rows.check()
    din.check()
    return len(c["trace"])


def run_group(c, kind, trace):
    total, op = c["total"], c["op"]
    plan = t.Plan(c["algo"], route_cases.BO, c["side"], c["n"], total, route_cases.FUSED)
    bufs, shards, args = [], [], []
    for i, (n, has_shard) in enumerate(c["buckets"]):
        blk = n // total
        data = dataset(kind, total, n)
        rows = rank_rows(f"bucket {i} ranks", data)
        src = np.stack([data[(b + 1) % total, b * blk:(b + 1) * blk] for b in range(total)])
        shard = side_rows(f"bucket {i} shard", total, blk, src if op == "shard_ag" else None) if has_shard else None
        bufs.append(rows)
        shards.append(shard)
        args.append((rows.ptr, rows.width, n, shard.ptr, shard.width) if shard else (rows.ptr, rows.width, n))
        cols = columns(kind, total, n)
        if op == "group_exec":
            rows.rows()[:, :n] = reference(kind, "bo", c["algo"], c["side"], total, n)
            for r in range(total):
                rows.plant(r, cols, 0, n)
        elif op in ("group_rs", "shard_rs"):
            want = owner_blocks(reference(kind, "bo", c["algo"], c["side"], total, n), total, n)
            for b in range(total):
                if shard:
                    shard.rows()[b, :blk] = want[b]
                    shard.plant(b, cols, b * blk, blk)
                else:
                    rows.rows()[b, b * blk:(b + 1) * blk] = want[b]
                    rows.plant(b, [(col, cls) for col, cls in cols if col // blk == b])
        else:   # shard_ag: a copy, bit for bit
            rows.rows()[:, :n] = (src if shard else owner_blocks(data, total, n)).reshape(-1)[None, :]
    plain = [a[:3] for a in args]
    with trace:
        if op == "group_exec":
            plan.execute_group(plain, stream())
        elif op == "group_rs":
            plan.reduce_scatter_group(plain, stream())
        elif op == "shard_rs":
            plan.reduce_scatter_shards(args, stream())
        else:
            plan.all_gather_shards(args, stream())
    torch.cuda.synchronize()
    if op == "group_exec":
        dry = plan.group_launches(plain)
    else:   # the in-place reduce-scatter list is the shard list without shards
        dry = plan.shards_launches(plain if op == "group_rs" else args,
                                   t.OP_ALL_GATHER if op == "shard_ag" else t.OP_REDUCE_SCATTER)
    plan.close()
    for b in bufs + [s for s in shards if s]:
        b.check()
    return dry


def run_tree_bcast(c, kind, trace):
    """tree 0 of `cur` over the whole vector to cur_out (= the LO value of rank 0), prev_src to every row of prev"""
    total, n = c["total"], c["n"]
    data = dataset(kind, total, n)
    want = reference(kind, "lo", c["algo"], c["side"], total, n)[0]
    cur = rank_rows("cur", data)
    prev = rank_rows("prev", dataset("cancel" if kind == "nonfinite" else "nonfinite", total, n))
    src_bits = np.random.default_rng(SEED + n).integers(0, 0x10000, n).astype(np.uint16)   # any pattern: a copy
    src = side_rows("prev_src", 1, n, src_bits)
    out = side_rows("cur_out", 1, n)
    with trace:
        t.tree_broadcast_pipelined(cur.ptr, prev.ptr, cur.width, n, c["algo"], c["side"], total, out.ptr, src.ptr,
                                   stream())
    torch.cuda.synchronize()
    out.rows()[0, :n] = want
    out.plant(0, columns(kind, total, n), 0, n)
    prev.rows()[:, :n] = src_bits[None, :]
    for b in (cur, prev, src, out):
        b.check()
    return len(c["trace"])


RUN = {"allreduce": run_allreduce, "rs_inplace": run_reduce_scatter, "rs_compact": run_reduce_scatter,
       "ag_inplace": run_all_gather, "ag_from_in": run_all_gather, "group_exec": run_group, "group_rs": run_group,
       "shard_rs": run_group, "shard_ag": run_group, "tree_bcast": run_tree_bcast}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", route_cases.CASES, ids=[c["id"] for c in route_cases.CASES])
def test_route(c, kind):
    trace = t.launch_trace()
    with t.tuned(**c["keys"]):
        launches = RUN[c["op"]](c, kind, trace)
    print(f"{c['id']} {kind}: {trace.kernels} grids {trace.grids}; {launches} launches expected")
    assert trace.kernels == c["trace"]
    assert trace.count == launches == len(c["trace"])
