"""The route cases of tests/route_cases.py as runnable pieces (helper, no tests).

PREPARE[op](c, kind, place, seed) builds the buffers of case c on dataset `kind` (of seed `seed`; the
default is the images the route modules have always run on) and their expected images and returns a Prepared:
    prepare   every buffer the call may touch is sentinel-filled around its payload; the expected
              image is the CPU oracle where the operation defines a result, the input bits where it
              only reads, the sentinel everywhere else;
    call(s)   the library call on stream s (raises unless it returns ALLRED_OK);
    check()   every buffer compared whole, the workspace between its guards.
`place` decides where the buffers sit: NEAR (rows at preferred_rank_stride, dense images with guard
rows, as tests/test_gpu_routes.py always ran them) or a Far placement (tests/far_arena.py).
The three route modules share this: test_gpu_routes.py (default stream), test_gpu_routes_stream.py
(side stream, graph capture) and test_gpu_routes_far.py (row offsets beyond 2^32 elements).
"""
import functools

import numpy as np
import torch

import far_arena
import hard_inputs
import oracle
import route_cases
import tenstorrentallreduce_amd as t

DEV = "cuda:0"
SENT = 0xA5A5
GUARD = 256   # bytes in front of and behind the workspace; elements around 1-D buffers
GAP = 8       # elements behind every row of an out / in / shard buffer
SEED = 7
VARIANT_NAME = {route_cases.BO: "bo", route_cases.LO: "lo", route_cases.MEM: "mem"}


# ------------------------------------------------------------------ data and references (computed once, read-only)
def frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def dataset(kind, total, n, seed=SEED):
    return frozen(getattr(hard_inputs, kind)(total, n, seed))


@functools.lru_cache(maxsize=None)
def reference(kind, name, algo, side, total, n, acc16=False, seed=SEED):
    """the oracle's allreduce of dataset(kind, total, n, seed): (total, n) uint16"""
    want = [r.copy() for r in dataset(kind, total, n, seed)]
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
        self.staged = None

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

    def stage(self):
        """a device copy of the input image, for restore()"""
        if self.staged is None:
            self.staged = torch.from_numpy(self.image.view(np.int16).copy()).to(DEV)

    def restore(self):
        """the input image over the whole buffer, enqueued on the current stream"""
        self.dev.copy_(self.staged, non_blocking=True)

    def sentinel(self):
        """the sentinel over the whole buffer, payload included"""
        self.dev.fill_(np.uint16(SENT).view(np.int16).item())

    def check(self, expect=None):
        want = self.expect if expect is None else expect
        got = (self.dev if self.host else self.dev.cpu()).numpy().view(np.uint16)
        exact = np.ones(got.shape, dtype=bool)
        for r, c, cls in self.planted if expect is None else []:
            exact[r, c] = False
            known, g, w = hard_inputs.NONFINITE_CLASSES[cls], int(got[r, c]), int(want[r, c])
            where = f"{self.name} row {r - 1} column {c} ({cls})"
            if known == "nan":
                assert hard_inputs.is_nan(w), f"oracle, {where}: 0x{w:04X} is no NaN"
                assert hard_inputs.is_nan(g), f"{where}: 0x{g:04X} is no NaN"
            else:
                assert w == known, f"oracle, {where}: 0x{w:04X}, not 0x{known:04X}"
                assert g == known, f"{where}: 0x{g:04X}, not 0x{known:04X}"
        differing = int((got[exact] != want[exact]).sum())
        print(f"{self.name}: {differing} differing elements of {got.size}, {len(self.planted)} compared by class")
        if differing:
            r, c = np.argwhere((got != want) & exact)[0]
            assert False, (f"{self.name}: {differing} differing elements; first at row {r - 1} column {c}: "
                           f"0x{int(got[r, c]):04X}, expected 0x{int(want[r, c]):04X}")

    def check_input(self):
        self.check(self.image)


class FarBuf:
    """Buf's face on one set of a far layout: `width` is the far stride, rows() the expected payload
    rows; check() compares every payload row and its guards bit for bit, then puts the sentinel back."""

    def __init__(self, arena, s, data=None):
        self.name, self.far, self.width = s.name, far_arena.FarRows(arena, s), s.stride
        self.expect = np.full((s.rows, s.width), SENT, dtype=np.uint16)
        if data is not None:
            self.expect[:] = data
            self.far.upload(self.expect)
        self.planted = []

    @property
    def ptr(self):
        return self.far.ptr

    def rows(self):
        return self.expect

    def plant(self, row, cols, offset=0, width=None):
        assert not cols, "far runs compare bit for bit"

    def check(self):
        try:
            payload = self.far.read()
        finally:
            self.far.wipe()
        differing = int((payload != self.expect).sum())
        print(f"{self.name}: {differing} differing elements of {payload.size}, rows {self.width} elements apart")
        if differing:
            r, c = np.argwhere(payload != self.expect)[0]
            assert False, (f"{self.name}: {differing} differing elements; first at row {r} column {c}: "
                           f"0x{int(payload[r, c]):04X}, expected 0x{int(self.expect[r, c]):04X}")


class Near:
    def rank_rows(self, name, data, host=False):
        total, n = data.shape
        b = Buf(name, total, t.preferred_rank_stride(n), host)
        b.image[1:total + 1, :n] = data
        return b.upload()

    def side_rows(self, name, total, blk, fill=None):
        """an out / in / shard buffer: `total` rows of blk elements, GAP elements behind each"""
        b = Buf(name, total, blk + GAP)
        if fill is not None:
            b.image[1:total + 1, :blk] = fill
        return b.upload()

    def bucket(self, c, i):
        return self


NEAR = Near()


class Far:
    """the sets of one far layout, handed out in the order the layout lists them"""

    def __init__(self, arena, layout):
        self.arena, self.left = arena, list(layout.sets)

    def take(self, name, rows, width):
        s = self.left.pop(0)
        assert (s.name, s.rows, s.width, s.es) == (name, rows, width, 2), (s.name, name)
        return s

    def rank_rows(self, name, data, host=False):
        assert not host
        return FarBuf(self.arena, self.take(name, *data.shape), data)

    def side_rows(self, name, total, blk, fill=None):
        return FarBuf(self.arena, self.take(name, total, blk), fill)

    def bucket(self, c, i):
        return self if i == far_arena.far_bucket(c) else NEAR


class Workspace:
    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.dev = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=DEV) if nbytes else None

    @property
    def ptr(self):
        return self.dev.data_ptr() + GUARD if self.nbytes else None

    def restore(self):
        if self.nbytes:
            self.dev.fill_(0xA5)

    def check(self, content=None):
        if not self.nbytes:
            return
        got = self.dev.cpu().numpy()
        assert (got[:GUARD] == 0xA5).all(), "the guard in front of the workspace was written"
        assert (got[GUARD + self.nbytes:] == 0xA5).all(), "the guard behind the workspace was written"
        return got[GUARD:GUARD + self.nbytes]

    def check_input(self):
        if self.nbytes:
            assert (self.dev.cpu().numpy() == 0xA5).all(), "the workspace was written"


def owner_blocks(a, total, n):
    blk = n // total
    return np.stack([a[b, b * blk:(b + 1) * blk] for b in range(total)])


class Prepared:
    """One case ready to run: bufs (every buffer, expected images final), ws, call(stream),
    launches() (what the plan announces under the current tune keys) and ws_content (what the
    workspace must hold afterwards, where the route defines it)."""

    def __init__(self, bufs, call, launches, plan=None, ws=None, ws_content=None):
        self.bufs, self.call, self.launches, self.plan = [b for b in bufs if b is not None], call, launches, plan
        self.ws, self.ws_content = ws or Workspace(0), ws_content

    def check(self):
        for b in self.bufs:
            b.check()
        inside = self.ws.check()
        if self.ws_content is not None:
            assert np.array_equal(inside.view(np.uint16), self.ws_content), "the workspace holds the reduced vector"

    def stage(self):
        for b in self.bufs:
            b.stage()

    def restore(self):
        """every buffer and the workspace back to the input image, on the current stream"""
        for b in self.bufs:
            b.restore()
        self.ws.restore()

    def sentinel(self):
        for b in self.bufs:
            b.sentinel()
        self.ws.restore()

    def check_input(self):
        for b in self.bufs:
            b.check_input()
        self.ws.check_input()

    def close(self):
        if self.plan is not None:
            self.plan.close()


# ------------------------------------------------------------------ the operations
def prepare_allreduce(c, kind, place=NEAR, seed=SEED):
    total, n = c["total"], c["n"]
    data = dataset(kind, total, n, seed)
    want = reference(kind, VARIANT_NAME[c["variant"]], c["algo"], c["side"], total, n, c["acc"] == route_cases.BF16, seed)
    rows = place.rank_rows("ranks", data, c["host"])
    plan = t.Plan(c["algo"], c["variant"], c["side"], n, total, c["exec"], mem_accum=c["acc"])
    ws = Workspace(plan.workspace_bytes)
    rows.rows()[:, :n] = want
    for r in range(total):
        rows.plant(r, columns(kind, total, n), 0, n)
    holds = c["variant"] == route_cases.MEM and c["exec"] == route_cases.STEPS and kind == "cancel"
    return Prepared([rows], lambda s: plan.execute(rows.ptr, rows.width, ws.ptr, s), lambda: plan.launches, plan, ws,
                    want[0] if holds else None)


def prepare_reduce_scatter(c, kind, place=NEAR, seed=SEED):
    total, n, compact = c["total"], c["n"], c["op"] == "rs_compact"
    blk = n // total
    data = dataset(kind, total, n, seed)
    want = owner_blocks(reference(kind, "bo", c["algo"], c["side"], total, n, seed=seed), total, n)
    rows = place.rank_rows("ranks", data)
    out = place.side_rows("out", total, blk)
    plan = t.Plan(c["algo"], route_cases.BO, c["side"], n, total, route_cases.FUSED)
    for b in range(total):   # block b to rank b's row, or to out row b; everything else keeps its bits
        if compact:
            out.rows()[b, :blk] = want[b]
            out.plant(b, columns(kind, total, n), b * blk, blk)
        else:
            rows.rows()[b, b * blk:(b + 1) * blk] = want[b]
            rows.plant(b, [(col, cls) for col, cls in columns(kind, total, n) if col // blk == b])

    def call(s):
        if compact:
            plan.reduce_scatter(rows.ptr, rows.width, out.ptr, out.width, stream=s)
        else:
            plan.reduce_scatter(rows.ptr, rows.width, stream=s)
    return Prepared([rows, out], call, lambda: len(c["trace"]), plan)


def prepare_all_gather(c, kind, place=NEAR, seed=SEED):
    """a copy: every 16-bit pattern must arrive as it is, so nothing is compared by class"""
    total, n, from_in = c["total"], c["n"], c["op"] == "ag_from_in"
    blk = n // total
    data = dataset(kind, total, n, seed)
    rows = place.rank_rows("ranks", data)
    src = np.stack([data[(b + 1) % total, b * blk:(b + 1) * blk] for b in range(total)])   # not the owners' blocks
    din = place.side_rows("in", total, blk, src)
    plan = t.Plan(c["algo"], route_cases.BO, c["side"], n, total, route_cases.FUSED)
    rows.rows()[:, :n] = (src if from_in else owner_blocks(data, total, n)).reshape(-1)[None, :]

    def call(s):
        if from_in:
            plan.all_gather(rows.ptr, rows.width, din.ptr, din.width, stream=s)
        else:
            plan.all_gather(rows.ptr, rows.width, stream=s)
    return Prepared([rows, din], call, lambda: len(c["trace"]), plan)


def prepare_group(c, kind, place=NEAR, seed=SEED):
    total, op = c["total"], c["op"]
    plan = t.Plan(c["algo"], route_cases.BO, c["side"], c["n"], total, route_cases.FUSED)
    bufs, shards, args = [], [], []
    for i, (n, has_shard) in enumerate(c["buckets"]):
        blk = n // total
        data = dataset(kind, total, n, seed)
        where = place.bucket(c, i)
        rows = where.rank_rows(f"bucket {i} ranks", data)
        src = np.stack([data[(b + 1) % total, b * blk:(b + 1) * blk] for b in range(total)])
        shard = (where.side_rows(f"bucket {i} shard", total, blk, src if op == "shard_ag" else None)
                 if has_shard else None)
        bufs.append(rows)
        shards.append(shard)
        args.append((rows.ptr, rows.width, n, shard.ptr, shard.width) if shard else (rows.ptr, rows.width, n))
        cols = columns(kind, total, n)
        if op == "group_exec":
            rows.rows()[:, :n] = reference(kind, "bo", c["algo"], c["side"], total, n, seed=seed)
            for r in range(total):
                rows.plant(r, cols, 0, n)
        elif op in ("group_rs", "shard_rs"):
            want = owner_blocks(reference(kind, "bo", c["algo"], c["side"], total, n, seed=seed), total, n)
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

    def call(s):
        if op == "group_exec":
            plan.execute_group(plain, s)
        elif op == "group_rs":
            plan.reduce_scatter_group(plain, s)
        elif op == "shard_rs":
            plan.reduce_scatter_shards(args, s)
        else:
            plan.all_gather_shards(args, s)

    def dry():
        if op == "group_exec":
            return plan.group_launches(plain)
        # the in-place reduce-scatter list is the shard list without shards
        return plan.shards_launches(plain if op == "group_rs" else args,
                                    t.OP_ALL_GATHER if op == "shard_ag" else t.OP_REDUCE_SCATTER)
    return Prepared(bufs + shards, call, dry, plan)


def prepare_tree_bcast(c, kind, place=NEAR, seed=SEED):
    """tree 0 of `cur` over the whole vector to cur_out (= the LO value of rank 0), prev_src to every row of prev"""
    total, n = c["total"], c["n"]
    data = dataset(kind, total, n, seed)
    want = reference(kind, "lo", c["algo"], c["side"], total, n, seed=seed)[0]
    cur = place.rank_rows("cur", data)
    prev = place.rank_rows("prev", dataset("cancel" if kind == "nonfinite" else "nonfinite", total, n, seed))
    src_bits = np.random.default_rng(seed + n).integers(0, 0x10000, n).astype(np.uint16)   # any pattern: a copy
    src = place.side_rows("prev_src", 1, n, src_bits)
    out = place.side_rows("cur_out", 1, n)
    assert cur.width == prev.width
    out.rows()[0, :n] = want
    out.plant(0, columns(kind, total, n), 0, n)
    prev.rows()[:, :n] = src_bits[None, :]

    def call(s):
        t.tree_broadcast_pipelined(cur.ptr, prev.ptr, cur.width, n, c["algo"], c["side"], total, out.ptr, src.ptr, s)
    return Prepared([cur, prev, src, out], call, lambda: len(c["trace"]))


PREPARE = {"allreduce": prepare_allreduce, "rs_inplace": prepare_reduce_scatter, "rs_compact": prepare_reduce_scatter,
           "ag_inplace": prepare_all_gather, "ag_from_in": prepare_all_gather, "group_exec": prepare_group,
           "group_rs": prepare_group, "shard_rs": prepare_group, "shard_ag": prepare_group,
           "tree_bcast": prepare_tree_bcast}


def check_trace(c, trace, launches):
    """the launch trace of the call is the case's, and its count what the plan announced"""
    print(f"{c['id']}: {trace.kernels} grids {trace.grids}; {launches} launches expected")
    assert trace.kernels == c["trace"]
    assert trace.count == launches == len(c["trace"])
