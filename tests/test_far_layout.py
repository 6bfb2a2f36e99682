"""The far layouts of tests/far_arena.py, on the CPU: a kernel that computed a row offset in 32 bits
would fail a compare of tests/test_gpu_routes_far.py (or of the far fp32 shard tests), not fault.

For every far case, every set of its layout and every row whose offset o = r * stride crosses a
threshold, each of the four 32-bit misreadings of o

    o truncated to uint32 elements        o * size truncated to uint32 bytes
    o sign-extended from int32 elements   o * size sign-extended from int32 bytes

is applied to the pointer the library gets (row 0 of the set).  The row's payload, moved there,
must lie (a) inside the arena and (b) on no payload or guard window of the case, so the misread
access meets only sentinel bytes the test compares on the device, and the true row — never
written, or reduced from sentinels — fails its bit-for-bit compare.

(b) has one exception the stride rule itself makes, and the test pins it down exactly.  With
stride = roundup8(ceil(2^32 / (P-1))) + skew (two rows: 2^31 + skew) the LAST row starts (P-1) * skew
(+ rounding) elements beyond 2^32 elements (two rows: beyond 2^32 bytes), so its offset read in 32
bits lands that many elements into row 0 OF THE SAME SET: at a different, nonzero column of a
window that is compared whole.  The true last row still stays sentinel, so the compare still fails;
nothing is outside the arena.  No other overlap is allowed.
"""
import pytest

import far_arena as fa
import route_cases

FAR = fa.far_cases(route_cases.CASES)
T31, T32, T33 = 1 << 31, 1 << 32, 1 << 33


def overlaps(a0, a1, b0, b1):
    return a0 < b1 and b0 < a1


def check_layout(L, label):
    """(a) and (b) for every crossing row of every set; returns the number of misread rows checked"""
    nbytes = L.nbytes
    assert nbytes <= fa.CAP, f"{label}: an arena of {nbytes} bytes"
    windows = L.windows()
    for s, r, a, b in windows:   # the layout itself: inside the arena, behind the front pad, no two windows meeting
        assert fa.FRONT - fa.GUARD <= a < b <= nbytes - fa.TAIL, (label, s.name, r)
    spans = sorted((a, b) for _, _, a, b in windows)
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:])), f"{label}: two windows overlap"
    checked = 0
    for s in L.sets:
        for r in range(s.rows):
            o = s.offset(r)
            for name, m in fa.misreadings(o, s.es):
                checked += 1
                a, b = s.base + m, s.base + m + s.es * s.width
                assert 0 <= a and b <= nbytes, f"{label}: {s.name} row {r} read as {name} leaves the arena"
                for s2, r2, w0, w1 in windows:
                    if not overlaps(a, b, w0, w1):
                        continue
                    # the one overlap the stride rule makes: the last row onto row 0 of its own set, shifted
                    shift = m // s.es
                    assert s2 is s and r2 == 0 and r == s.rows - 1, \
                        f"{label}: {s.name} row {r} read as {name} lands on {s2.name} row {r2}"
                    assert 0 < shift <= (s.rows - 1) * (fa.SKEW + 8), (label, s.name, name, shift)
    return checked


def crossings(s):
    """which thresholds the row offsets of a set cross: in elements and in bytes"""
    offs = [s.offset(r) for r in range(s.rows)]
    return {"2^31 elements": any(T31 <= o < T32 for o in offs), "2^32 elements": any(o >= T32 for o in offs),
            "2^31 bytes": any(s.es * o >= T31 for o in offs), "2^32 bytes": any(s.es * o >= T32 for o in offs),
            "2^33 bytes": any(s.es * o >= T33 for o in offs)}


@pytest.mark.parametrize("c", FAR, ids=[c["id"] for c in FAR])
def test_route_layout_turns_a_32_bit_offset_into_a_failed_compare(c):
    L = fa.route_layout(c)
    P = c["total"]
    for s in L.sets:
        assert (s.base % 16, s.stride % 8) == (0, 0), "what the library asks of rows: 16-byte aligned"
        if s.rows < 2:   # prev_src / cur_out of the tree broadcast: one row, no stride to misread
            continue
        assert s.rows == P
        x = crossings(s)
        assert x["2^31 elements"] and x["2^32 bytes"], (c["id"], s.name)
        assert x["2^32 elements"] == x["2^33 bytes"] == (P >= 4), (c["id"], s.name)
    assert check_layout(L, c["id"]) > 0


def test_the_stride_rule():
    assert fa.far_stride(2) == (1 << 31) + 136
    for P in (4, 8, 16, 32, 64):
        st = fa.far_stride(P)
        assert st % 8 == 0 and st == (-(-(1 << 32) // (P - 1)) + 7) // 8 * 8 + 136
        assert (P - 1) * st >= T32 > (P - 1) * (st - 136 - 8)
    F = fa.far_stride_f32(64)
    assert F % 4 == 0 and F == (-(-(1 << 32) // 63) + 3) // 4 * 4 + 64 and 63 * F >= T32


def test_the_largest_arena_is_under_the_cap():
    sizes = {c["id"]: fa.route_layout(c).nbytes for c in FAR}
    worst = max(sizes, key=sizes.get)
    print(f"largest route arena: {sizes[worst] / fa.GiB:.2f} GiB ({worst})")
    assert fa.FRONT >= 4 * fa.GiB and max(sizes.values()) <= fa.CAP == 32 * fa.GiB
    assert next(c for c in FAR if c["id"] == worst)["total"] == 4   # P = 4 with a side buffer is the worst
    for planes in (1, 4):
        assert fa.f32_layout(planes).nbytes <= fa.CAP


def test_no_route_drops_out():
    """the stream module runs every case; the far module every case but one-rank and pinned-host ones"""
    ids = [c["id"] for c in route_cases.CASES]
    far = [c["id"] for c in FAR]
    out = [c["id"] for c in route_cases.CASES if c["total"] < 2 or c["host"]]
    assert sorted(far + out) == sorted(ids) and not set(far) & set(out)
    assert out == ["bo-fused-reg-1", "bo-fused-pipe-host-16", "rs-inplace-one-rank", "rs-compact-reg-1",
                   "ag-inplace-one-rank", "ag-from-in-1", "lo-one-rank-butterfly", "lo-one-rank-tree"]
    assert {c["total"] for c in FAR} == {2, 4, 8, 16, 32, 64}
    grouped = [c for c in FAR if c["buckets"]]
    assert all(fa.far_bucket(c) == 1 and len(c["buckets"]) in (3, 4) for c in grouped)   # the middle of the list
    with_far_shard = sorted(c["id"] for c in grouped if c["buckets"][1][1])
    assert with_far_shard == sorted([f"shard-rs-{P}" for P in route_cases.R8_64] + ["shard-ag-mixed-64"])


@pytest.mark.parametrize("planes", [1, 4], ids=["shards", "adamw"])
def test_f32_layout_turns_a_32_bit_offset_into_a_failed_compare(planes):
    L = fa.f32_layout(planes)
    rows = [s for s in L.sets if s.es == 2]
    flat = [s for s in L.sets if s.es == 4]
    assert len(rows) == 1 and len(flat) == planes * len(fa.F32_TILES)
    for s in rows:
        x = crossings(s)
        assert x["2^31 elements"] and x["2^32 elements"]
    for s in flat:
        assert s.stride == fa.far_stride_f32(64) and s.base % 16 == 0
        offs = [s.offset(r) for r in range(s.rows)]
        assert offs[-1] >= T32 and any(1 << 30 <= o < T31 for o in offs) and any(T31 <= o < T32 for o in offs)
    assert check_layout(L, f"f32 x{planes}") > 0
