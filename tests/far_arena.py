"""Rank rows and side buffers at a FAR stride: row offsets beyond 2^31 and 2^32 elements (helper, no tests).

The layout half is plain arithmetic (no torch, no GPU): tests/test_far_layout.py holds it to its
rules on the CPU.  The device half carves the sets of one layout from one arena.

One arena, in bytes from its start:
    [0, FRONT)        front pad, at least 4 GiB: an offset read as a negative int32 lands here
    row region        the rank-row sets of the case, all at ONE stride, side by side in columns
    SIDE_SKEW         keeps a misread side offset off the rank rows it would otherwise meet
    side region       out / in / shard sets, each at the stride its own row count gives
    TAIL              tail pad
Everything is sentinel bytes except the payload rows while a test runs.  A test compares every
payload row with GUARD bytes on both sides on the host, writes the sentinel back over those
windows and then asserts ON THE DEVICE, in chunks, that the whole arena is sentinel again.
"""
import numpy as np

GiB = 1 << 30
SENT_BYTE = 0xA5
GUARD = 4096               # bytes of guard window in front of and behind every payload row
FRONT = 4 * GiB
SIDE_SKEW = 32 * (1 << 20) + 5 * GUARD
TAIL = 16 * (1 << 20)
CAP = 32 * GiB
CHUNK = GiB                # the largest tensor any device operation of this module touches
SKEW = 8 * 17              # elements: rows 16-byte aligned and no more
F32_SKEW = 64              # floats: the same, for fp32 rows


def roundup(x, m):
    return (x + m - 1) // m * m


def far_stride(rows):
    """elements between the rows of a bf16 set of `rows` rows"""
    if rows >= 4:   # the last row starts beyond 2^32 elements, middle rows beyond 2^31 elements = 2^32 bytes
        return roundup(-(-(1 << 32) // (rows - 1)), 8) + SKEW
    if rows == 2:   # row 1 beyond 2^31 elements = 2^32 bytes
        return (1 << 31) + SKEW
    raise ValueError(f"no far stride for {rows} rows")


def far_stride_f32(rows):
    """floats between the rows of an fp32 set: (rows - 1) * stride crosses 2^32 floats"""
    return roundup(-(-(1 << 32) // (rows - 1)), 4) + F32_SKEW


def column_pitch(nbytes):
    """bytes from one set of a region to the next: the payload, its guards, and room for the last row's
    offset read in 32 bits, which lands up to 63 * (skew + rounding) elements behind row 0 of its own set"""
    return roundup(2 * nbytes + 2 * GUARD, 16) + (1 << 16) + 16 * 17


class Set:
    """`rows` payload rows of `width` elements of `es` bytes, row r at base + es * r * stride bytes of the arena"""

    def __init__(self, name, base, stride, es, rows, width):
        self.name, self.base, self.stride, self.es, self.rows, self.width = name, base, stride, es, rows, width

    def offset(self, r):       # elements, what a kernel computes as r * stride
        return r * self.stride

    def payload(self, r):      # bytes of the arena
        a = self.base + self.es * r * self.stride
        return a, a + self.es * self.width

    def window(self, r):       # the payload with its guards
        a, b = self.payload(r)
        return a - GUARD, b + GUARD


class Layout:
    def __init__(self):
        self.sets = []
        self.row_stride = None
        self.col = 0            # bytes: the next free column of the row region
        self.row_end = FRONT
        self.side_end = None

    def _column(self, es, width):
        col = self.col
        self.col += column_pitch(es * width)
        return col

    def rows(self, name, rows, width, stride=None, es=2):
        """a rank-row set; every one of a layout has the same stride and sits in a column of its own"""
        assert self.side_end is None, "row sets come first"
        stride = far_stride(rows) if stride is None else stride
        assert self.row_stride in (None, (stride, es)) and (stride * es) % 16 == 0
        self.row_stride = (stride, es)
        s = Set(name, FRONT + self._column(es, width), stride, es, rows, width)
        assert self.col < es * stride, "the columns of the row region fit between two rows"
        # the library takes [row 0, row 0 + rows * stride) as the footprint no side buffer may sit in
        self.row_end = max(self.row_end, s.window(rows - 1)[1], s.base + es * rows * stride)
        self.sets.append(s)
        return s

    def side(self, name, rows, width, stride=None, es=2):
        """an out / in / shard set in the side region, behind everything placed so far"""
        if stride is None:
            stride = far_stride(rows) if rows >= 2 else roundup(width, 8) + SKEW
        assert (stride * es) % 16 == 0
        start = roundup(self.row_end, GUARD) + SIDE_SKEW if self.side_end is None else roundup(self.side_end, 16) + 16 * 17
        s = Set(name, start + GUARD, stride, es, rows, width)
        self.side_end = s.window(rows - 1)[1]
        self.sets.append(s)
        return s

    @property
    def nbytes(self):
        return roundup(self.row_end if self.side_end is None else self.side_end, GUARD) + TAIL

    def windows(self):
        return [(s, r) + s.window(r) for s in self.sets for r in range(s.rows)]


def sext32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def misreadings(o, es):
    """the byte offsets four 32-bit misreadings of the element offset o give; (name, bytes) where they differ"""
    true = es * o
    all4 = [("uint32 elements", es * (o & 0xFFFFFFFF)), ("uint32 bytes", true & 0xFFFFFFFF),
            ("int32 elements", es * sext32(o)), ("int32 bytes", sext32(true))]
    return [(name, m) for name, m in all4 if m != true]


# ------------------------------------------------------------------ the layouts of the route cases
def far_bucket(c):
    """the bucket of a grouped case that sits in the arena: the middle one of the list"""
    return (len(c["buckets"]) - 1) // 2


def route_layout(c):
    """the sets tests/route_run.py asks for when case c runs far, in the order it asks"""
    L, P, n = Layout(), c["total"], c["n"]
    op = c["op"]
    if op == "allreduce":
        L.rows("ranks", P, n)
    elif op in ("rs_inplace", "rs_compact"):
        L.rows("ranks", P, n)
        L.side("out", P, n // P)
    elif op in ("ag_inplace", "ag_from_in"):
        L.rows("ranks", P, n)
        L.side("in", P, n // P)
    elif op == "tree_bcast":
        L.rows("cur", P, n)
        L.rows("prev", P, n)
        L.side("prev_src", 1, n)
        L.side("cur_out", 1, n)
    else:
        i = far_bucket(c)
        bn, has_shard = c["buckets"][i]
        L.rows(f"bucket {i} ranks", P, bn)
        if has_shard:
            L.side(f"bucket {i} shard", P, bn // P)
    return L


def far_cases(cases):
    """the route cases that run far: at least two ranks (one row has no stride), rows in device memory"""
    return [c for c in cases if c["total"] >= 2 and not c["host"]]


# ------------------------------------------------------------------ the layout of the fp32 shard tests
F32_TOTAL = 64
F32_TILES = (1, 3)   # 256-float tiles per block of the two buckets
F32_FAR_ROWS = 1     # the bucket whose rank rows are far: a grouped list takes no two buckets whose row footprints
                     # [row 0, row 0 + P * stride) meet, and two far footprints and the flat buffer pass the cap


def f32_layout(planes=1):
    """8x8 Swing: the bf16 rank rows of bucket F32_FAR_ROWS far, and for every bucket `planes` fp32 planes of
    64 blocks in ONE flat fp32 buffer of row stride F, every bucket and plane at a column offset of its own"""
    L, P = Layout(), F32_TOTAL
    L.rows(f"bucket {F32_FAR_ROWS} ranks", P, 256 * F32_TILES[F32_FAR_ROWS] * P)
    F = far_stride_f32(P)
    flat = roundup(L.row_end, GUARD) + SIDE_SKEW + GUARD
    col = 0
    for i, k in enumerate(F32_TILES):
        for p in range(planes):
            s = Set(f"bucket {i} plane {p}", flat + col, F, 4, P, 256 * k)
            col += column_pitch(4 * 256 * k)
            L.sets.append(s)
            L.side_end = max(L.side_end or 0, s.window(P - 1)[1])
    assert col < 4 * F
    return L


# ------------------------------------------------------------------ the device half
class Arena:
    """`nbytes` of device memory, sentinel-filled once, never touched as one tensor"""

    def __init__(self, nbytes, device="cuda:0"):
        import torch
        assert nbytes <= CAP, f"a far arena of {nbytes} bytes is above the cap of {CAP}"
        self.torch, self.nbytes = torch, nbytes
        self.mem = torch.empty(nbytes, dtype=torch.uint8, device=device)
        for a in range(0, nbytes, CHUNK):
            self.mem[a:min(a + CHUNK, nbytes)].fill_(SENT_BYTE)
        torch.cuda.synchronize()

    def bytes(self, a, b):
        assert 0 <= a <= b <= self.nbytes and b - a <= CHUNK
        return self.mem[a:b]

    def ptr(self, a):
        assert 0 <= a < self.nbytes
        return self.mem.data_ptr() + a

    def assert_sentinel(self):
        """the whole arena holds the sentinel: compared on the device, chunk by chunk"""
        torch = self.torch
        want = int.from_bytes(bytes([SENT_BYTE] * 8), "little", signed=True)
        bad = torch.stack([self.mem[a:min(a + CHUNK, self.nbytes)].view(torch.int64).ne(want).any()
                           for a in range(0, self.nbytes, CHUNK)]).cpu().numpy()
        if bad.any():
            a = int(bad.argmax()) * CHUNK
            chunk = self.mem[a:min(a + CHUNK, self.nbytes)]
            first = a + int(chunk.ne(SENT_BYTE).to(torch.uint8).argmax())
            n = sum(int(self.mem[x:min(x + CHUNK, self.nbytes)].ne(SENT_BYTE).sum()) for x in range(0, self.nbytes, CHUNK))
            for x in range(0, self.nbytes, CHUNK):   # later tests start from a clean arena
                self.mem[x:min(x + CHUNK, self.nbytes)].fill_(SENT_BYTE)
            assert False, f"{n} bytes of the arena outside every payload window were written; first at byte {first}"

    def close(self):
        self.mem = None
        self.torch.cuda.empty_cache()


class FarRows:
    """one Set of a layout in an arena: upload rows, read every window back, put the sentinel back"""

    def __init__(self, arena, s):
        assert s.window(0)[0] >= 0 and s.window(s.rows - 1)[1] <= arena.nbytes
        self.arena, self.set = arena, s

    @property
    def ptr(self):
        return self.arena.ptr(self.set.base)

    def upload(self, host):
        """host: (rows, width) of uint16 (es 2) or of 4-byte elements (es 4)"""
        torch, s = self.arena.torch, self.set
        assert host.shape == (s.rows, s.width) and host.dtype.itemsize == s.es
        dev = torch.from_numpy(np.ascontiguousarray(host).view("u1").reshape(s.rows, -1).copy()).to(self.arena.mem.device)
        for r in range(s.rows):
            self.arena.bytes(*s.payload(r)).copy_(dev[r])

    def windows(self):
        """(rows, GUARD + es * width + GUARD) bytes on the host"""
        torch, s = self.arena.torch, self.set
        return torch.stack([self.arena.bytes(*s.window(r)) for r in range(s.rows)]).cpu().numpy()

    def read(self):
        """the payload rows, (rows, width) of uint16 or uint32, once the guards around every one proved untouched"""
        got, s = self.windows(), self.set
        bad = int((got[:, :GUARD] != SENT_BYTE).sum() + (got[:, -GUARD:] != SENT_BYTE).sum())
        assert bad == 0, f"{s.name}: {bad} guard bytes around the payload rows were written"
        return np.ascontiguousarray(got[:, GUARD:-GUARD]).view(np.uint16 if s.es == 2 else np.uint32)

    def wipe(self):
        s = self.set
        for r in range(s.rows):
            self.arena.bytes(*s.window(r)).fill_(SENT_BYTE)


class F32Far:
    """f32_layout(planes) in an arena of its own: rows[i] the bf16 rank rows of bucket i — far for bucket
    F32_FAR_ROWS, the others in a small arena of their own —, planes[i][p] its fp32 planes, all of them
    blocks of the one flat fp32 buffer"""

    def __init__(self, planes):
        self.layout = f32_layout(planes)
        self.arena = Arena(self.layout.nbytes)
        sets, P = self.layout.sets, F32_TOTAL
        near, at = [], GUARD
        for i, k in enumerate(F32_TILES):
            if i != F32_FAR_ROWS:   # rows a guard window and a skew apart
                n = 256 * k * P
                near.append(Set(f"bucket {i} ranks", at, n + GUARD + SKEW, 2, P, n))
                at = roundup(near[-1].window(P - 1)[1], GUARD) + GUARD
        self.near = Arena(at)
        near = iter(near)
        self.rows = [FarRows(self.arena, sets[0]) if i == F32_FAR_ROWS else FarRows(self.near, next(near))
                     for i in range(len(F32_TILES))]
        self.planes = [[FarRows(self.arena, sets[1 + i * planes + p]) for p in range(planes)] for i in range(len(F32_TILES))]
        self.stride_f32 = far_stride_f32(P)

    def bucket(self, i):
        """(ranks_ptr, rank_stride, elems_per_rank) of bucket i"""
        s = self.rows[i].set
        return self.rows[i].ptr, s.stride, s.width

    def wipe(self):
        for f in self.rows + [p for ps in self.planes for p in ps]:
            f.wipe()

    def assert_sentinel(self):
        self.arena.assert_sentinel()
        self.near.assert_sentinel()

    def close(self):
        self.arena.close()
        self.near.close()
