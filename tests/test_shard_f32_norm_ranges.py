"""csrc/shard_f32_norm_ranges.hpp against brute force, on the CPU, in the style of
tests/test_shard_f32_ranges.py: a stand-alone C++ program (its own main) compiled with g++ under
AddressSanitizer and UBSan and run directly; nothing is loaded into Python.

shard_f32_norm_disjoint is the extra check of allred_plan_reduce_scatter_shards_f32_norm: the
`total` floats of norm_sq and the workspace are two plain byte intervals that may share no byte
with each other, with a bucket's rank-row interval [ranks, ranks + 2 total stride) or with any
fp32 shard block [shard + 4 b shard_stride, + 4 blk).  The brute force writes that out in
unsigned 128-bit arithmetic, every block of every bucket compared.

Lists: accepted ones of 1 .. 64 buckets at 8 / 16 / 64 ranks, compact, flat and wide (the list
itself passes shard_f32_lists_disjoint first, as in engine.cpp).  norm_sq / norm_ws: far away
(accepted); their FIRST byte on the last byte of a rank row, of a stride skew and of a shard block,
and their LAST byte on the first byte of each (refused); in the gap of a wide stride, filling it
exactly (accepted) and two bytes off either way (refused); overlapping each other by one byte, one
inside the other, and touching (accepted); at the top of the address space.
"""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "shard_f32_norm_ranges.hpp"

typedef unsigned __int128 u128;
using tsa::ShardF32Range;

static unsigned long long g_checks = 0, g_accepted = 0, g_refused = 0;

struct Rng {   // a fixed 64-bit LCG: the same lists on every run
    uint64_t s;
    uint64_t next(uint64_t n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (s >> 33) % n;
    }
};

static const void* at(uint64_t a) { return reinterpret_cast<const void*>((uintptr_t)a); }
static uint64_t addr(const void* p) { return (uint64_t)(uintptr_t)p; }

struct I { u128 lo, hi; };

// the rule, written out: the two intervals against each other and against every interval of the list
static bool brute(const std::vector<ShardF32Range>& list, uint64_t total, uint64_t sq, uint64_t sq_bytes, uint64_t ws,
                  uint64_t ws_bytes) {
    const I x[2] = {{(u128)sq, (u128)sq + sq_bytes}, {(u128)ws, (u128)ws + ws_bytes}};
    for (const I& i : x)
        if (i.hi > (u128)UINTPTR_MAX) return false;
    if (sq_bytes && ws_bytes && x[0].lo < x[1].hi && x[1].lo < x[0].hi) return false;
    std::vector<I> v;
    for (const ShardF32Range& s : list) {
        v.push_back(I{(u128)addr(s.ranks), (u128)addr(s.ranks) + (u128)2 * total * s.stride});
        if (!s.shard) continue;
        for (uint64_t b = 0; b < total; ++b) {
            const u128 lo = (u128)addr(s.shard) + (u128)4 * b * s.shard_stride;
            v.push_back(I{lo, lo + (u128)4 * (s.n / total)});
        }
    }
    for (const I& i : x)
        for (const I& j : v)
            if (i.hi > i.lo && j.hi > j.lo && i.lo < j.hi && j.lo < i.hi) return false;
    return true;
}

// want: 1 must be accepted, 0 must be refused, -1 whatever brute force says
static void check(const char* what, const std::vector<ShardF32Range>& list, uint64_t total, uint64_t sq, uint64_t sq_bytes,
                  uint64_t ws, uint64_t ws_bytes, int want) {
    if (!tsa::shard_f32_lists_disjoint(list.data(), (int)list.size(), total)) {
        std::printf("MISMATCH %s: the list itself is refused\n", what);
        std::exit(1);
    }
    const bool got = tsa::shard_f32_norm_disjoint(list.data(), (int)list.size(), total, at(sq), sq_bytes, at(ws), ws_bytes);
    const bool ref = brute(list, total, sq, sq_bytes, ws, ws_bytes);
    ++g_checks;
    ++(ref ? g_accepted : g_refused);
    if (got != ref || (want >= 0 && ref != (want == 1))) {
        std::printf("MISMATCH %s: count=%zu total=%llu norm_sq=%llx+%llu norm_ws=%llx+%llu got=%d brute=%d want=%d\n", what,
                    list.size(), (unsigned long long)total, (unsigned long long)sq, (unsigned long long)sq_bytes,
                    (unsigned long long)ws, (unsigned long long)ws_bytes, (int)got, (int)ref, want);
        for (const ShardF32Range& s : list)
            std::printf("  ranks=%llx stride=%llu n=%llu shard=%llx shard_stride=%llu\n", (unsigned long long)addr(s.ranks),
                        (unsigned long long)s.stride, (unsigned long long)s.n, (unsigned long long)addr(s.shard),
                        (unsigned long long)s.shard_stride);
        std::exit(1);
    }
}

enum Layout { COMPACT, FLAT, WIDE, LAYOUTS };

// an accepted list of whole-tile buckets: rank rows in buffers of their own (every other one with a
// stride skew), fp32 shards in `layout`; *end: the first byte behind everything
static std::vector<ShardF32Range> make(Rng& rng, int count, uint64_t total, Layout layout, uint64_t* end) {
    std::vector<ShardF32Range> list((size_t)count);
    uint64_t cursor = (1ull << 40) + 16 * rng.next(1000);
    for (int i = 0; i < count; ++i) {
        ShardF32Range& s = list[(size_t)i];
        s.n = 256 * total * (1 + rng.next(5));
        s.stride = s.n + (i % 2 ? 64 : 0);
        s.ranks = at(cursor);
        cursor += 2 * total * s.stride + 16 * rng.next(8);
    }
    if (layout == FLAT) {
        uint64_t F = 0, off = 0;
        for (int i = 0; i < count; ++i) F += list[(size_t)i].n / total;
        for (int i = 0; i < count; ++i) {
            list[(size_t)i].shard = at(cursor + 4 * off);
            list[(size_t)i].shard_stride = F;
            off += list[(size_t)i].n / total;
        }
        cursor += 4 * total * F;
    } else {
        for (int i = 0; i < count; ++i) {
            ShardF32Range& s = list[(size_t)i];
            s.shard = at(cursor);
            s.shard_stride = s.n / total + (layout == WIDE ? 64 : 0);   // WIDE: a gap of 256 bytes behind every block
            cursor += 4 * total * s.shard_stride + 16 * rng.next(4);
        }
    }
    *end = cursor;
    return list;
}

static uint64_t ws_bytes_of(const std::vector<ShardF32Range>& list) {
    uint64_t tiles = 0;
    for (const ShardF32Range& s : list) tiles += s.n / 256;
    return 64 + 4 * tiles;
}

// one of the two intervals put at `where`, the other far away; which: 0 norm_sq, 1 norm_ws
static void place(const char* what, const std::vector<ShardF32Range>& list, uint64_t total, uint64_t far, int which,
                  uint64_t first_byte, int want) {
    const uint64_t sq_bytes = 4 * total, ws_bytes = ws_bytes_of(list);
    const uint64_t far_sq = far, far_ws = far + (1ull << 20);
    check(what, list, total, which == 0 ? first_byte : far_sq, sq_bytes, which == 1 ? first_byte : far_ws, ws_bytes, want);
}

static void mutants(Rng& rng, const std::vector<ShardF32Range>& good, uint64_t total, uint64_t far) {
    const uint64_t len[2] = {4 * total, ws_bytes_of(good)};
    for (int which = 0; which < 2; ++which) {
        const ShardF32Range& t = good[rng.next(good.size())];
        const uint64_t r = rng.next(total), b = rng.next(total), blk = t.n / total;
        // the LAST byte of a rank row's data, and the interval's last byte on the row's FIRST
        place("on the last byte of a rank row", good, total, far, which, addr(t.ranks) + 2 * (r * t.stride + t.n) - 1, 0);
        place("ending on the first byte of a rank row", good, total, far, which, addr(t.ranks) + 2 * r * t.stride - len[which] + 1, 0);
        // the last byte of a stride skew (the first bucket that has one)
        for (const ShardF32Range& k : good) {
            if (k.stride == k.n) continue;
            place("on the last byte of a skew", good, total, far, which, addr(k.ranks) + 2 * (rng.next(total) + 1) * k.stride - 1, 0);
            break;
        }
        // the last and the first byte of a shard block
        place("on the last byte of a shard block", good, total, far, which, addr(t.shard) + 4 * (b * t.shard_stride + blk) - 1, 0);
        place("ending on the first byte of a shard block", good, total, far, which,
              addr(t.shard) + 4 * b * t.shard_stride - len[which] + 1, 0);
        place("inside a shard block", good, total, far, which, addr(t.shard) + 4 * (b * t.shard_stride + blk / 2), 0);
        place("far away", good, total, far, which, far + (2ull << 20) + 16 * rng.next(64), 1);
    }
}

int main() {
    Rng rng{20251020};
    const uint64_t totals[] = {8, 16, 64};
    for (int rep = 0; rep < 90; ++rep) {
        const uint64_t total = totals[rep % 3];
        const Layout layout = (Layout)((rep / 3) % LAYOUTS);
        const int count = rep < 9 ? 64 : 1 + (int)rng.next(64);
        uint64_t end;
        const std::vector<ShardF32Range> good = make(rng, count, total, layout, &end);
        const uint64_t far = end + (1ull << 30);
        for (int m = 0; m < 3; ++m) mutants(rng, good, total, far);
        // random places all over the list's span: whatever brute force says
        for (int m = 0; m < 40; ++m) {
            const uint64_t span = end - (1ull << 40);
            check("anywhere", good, total, (1ull << 40) + 4 * rng.next(span / 4), 4 * total, far, ws_bytes_of(good), -1);
            check("anywhere", good, total, far, 4 * total, (1ull << 40) + 16 * rng.next(span / 16), ws_bytes_of(good), -1);
        }
    }
    // A wide stride's gap filled exactly: 8 blocks of 256 floats (1024 bytes) 512 floats (2048 bytes) apart: the gap
    // behind block b is 1024 bytes.  That bucket has 8 tiles per rank row; a second one of 232 (in buffers of its own)
    // makes T = 240: a workspace of 64 + 960 = 1024 bytes, the whole gap.  norm_sq is 32 bytes.
    {
        const uint64_t big = 1ull << 40, shard = 1ull << 41, far = 1ull << 43;
        std::vector<ShardF32Range> wide = {ShardF32Range{at(big), 2048, 2048, at(shard), 512},
                                           ShardF32Range{at(big + (1ull << 30)), 232 * 256, 232 * 256, at(shard + (1ull << 30)), 8192}};
        const uint64_t ws_bytes = ws_bytes_of(wide);
        if (ws_bytes != 1024) {
            std::printf("MISMATCH the gap case's workspace is %llu bytes\n", (unsigned long long)ws_bytes);
            return 1;
        }
        for (uint64_t b : {0, 3, 6}) {
            const uint64_t gap = shard + 4 * (b * 512 + 256);
            for (int d : {0, 2, -2}) {
                check("norm_ws fills a gap", wide, 8, far, 32, gap + (uint64_t)(int64_t)d, ws_bytes, d == 0 ? 1 : 0);
                // norm_sq at the gap's head and at its tail
                check("norm_sq at the head of a gap", wide, 8, gap + (uint64_t)(int64_t)d, 32, far, ws_bytes, d >= 0 ? 1 : 0);
                check("norm_sq at the tail of a gap", wide, 8, gap + 1024 - 32 + (uint64_t)(int64_t)d, 32, far, ws_bytes, d <= 0 ? 1 : 0);
            }
        }
        // norm_sq and norm_ws against each other
        check("touching, norm_sq first", wide, 8, far, 32, far + 32, ws_bytes, 1);
        check("touching, norm_ws first", wide, 8, far + ws_bytes, 32, far, ws_bytes, 1);
        check("norm_sq's last byte on norm_ws's first", wide, 8, far, 32, far + 31, ws_bytes, 0);
        check("norm_ws's last byte on norm_sq's first", wide, 8, far + ws_bytes - 1, 32, far, ws_bytes, 0);
        check("norm_sq inside norm_ws", wide, 8, far + 64, 32, far, ws_bytes, 0);
        check("the same address", wide, 8, far, 32, far, ws_bytes, 0);
        // an empty list (count == 0): only the two against each other
        std::vector<ShardF32Range> none;
        check("count == 0, apart", none, 8, far, 32, far + 64, 64, 1);
        check("count == 0, norm_sq on the counter", none, 8, far + 32, 32, far, 64, 0);
        // the top of the address space
        const uint64_t top = (uint64_t)UINTPTR_MAX;
        for (int64_t d : {-16, -1, 0, 1, 16}) {
            check("norm_sq at the top", wide, 8, top - 32 + (uint64_t)d, 32, far, ws_bytes, d <= 0 ? 1 : 0);
            check("norm_ws at the top", wide, 8, far, 32, top - ws_bytes + (uint64_t)d, ws_bytes, d <= 0 ? 1 : 0);
        }
    }
    if (g_accepted < 200 || g_refused < 1000) {
        std::printf("MISMATCH the checks do not reach both verdicts: %llu accepted, %llu refused\n", g_accepted, g_refused);
        return 1;
    }
    std::printf("shard_f32_norm_ranges ok: %llu checks, %llu accepted, %llu refused\n", g_checks, g_accepted, g_refused);
    return 0;
}
"""


def test_norm_entry_points_refuse_before_any_hip_call():
    """no GPU here: a call that got as far as HIP would not return ALLRED_ERR_ARG, nor the size query 0"""
    from tenstorrentallreduce_amd import _lib
    lib = _lib.lib
    arr = (_lib.ShardBucketF32 * 1)((1 << 40, 2048, 2048, 1 << 41, 256))
    assert lib.allred_plan_reduce_scatter_shards_f32_norm(None, arr, 1, 1.0, 0, 1 << 42, 1 << 43, None) == _lib.ERR_ARG
    assert lib.allred_plan_shards_f32_norm_workspace_bytes(None, arr, 1) == 0
    assert lib.allred_plan_shards_f32_norm_workspace_bytes.restype is C.c_size_t


def test_shard_f32_norm_disjoint_matches_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the shard_f32_norm_ranges check"
    src = tmp_path / "shard_f32_norm_ranges_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "shard_f32_norm_ranges_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "shard_f32_norm_ranges ok" in run.stdout
