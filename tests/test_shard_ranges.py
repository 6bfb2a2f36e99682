"""csrc/shard_ranges.hpp against brute force, on the CPU.

A stand-alone C++ program (its own main) is compiled with g++ under AddressSanitizer and
UBSan and run directly.  For every list it compares shard_lists_disjoint — the disjointness
rule of allred_plan_reduce_scatter_shards / allred_plan_all_gather_shards — with the rule
written out in unsigned 128-bit arithmetic: every bucket's rank rows are ONE interval
[ranks, ranks + 2 total stride), every shard is its `total` SEPARATE block intervals
[shard + 2 b shard_stride, + 2 blk); a list is accepted when every interval ends at or below
UINTPTR_MAX and no two of them (an O(N^2) pairwise test) share a byte.

Lists: random ones of 1 .. 64 buckets at 8 / 16 / 64 ranks, the addresses made up (nothing
is dereferenced), in the layouts the interface is for:
  compact     every shard a buffer of its own, shard_stride = blk;
  flat        ONE rank-major buffer, one row of F elements per rank, bucket i's shard at
              flat + off_i with shard_stride = F: the enclosing ranges interleave;
  wide        shard_stride = blk + a gap, the blocks of other buckets lying in the gaps;
buckets without a shard mixed in.  Each of them must be ACCEPTED.  Each also has mutated
copies that move one shard so that one of its blocks covers a byte of a rank row, of a stride
skew, of another shard's block, or that give the same shard twice: each must be REFUSED.
Then addresses within blk of UINTPTR_MAX and strides whose products pass 2^64: refused where
an interval would wrap, accepted where it ends at UINTPTR_MAX.  Every verdict, accepted or
refused, must equal brute force's.
"""
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

#include "shard_ranges.hpp"

typedef unsigned __int128 u128;
using tsa::ShardRange;

static unsigned long long g_lists = 0, g_accepted = 0, g_refused = 0;

struct Rng {   // a fixed 64-bit LCG: the same lists on every run
    uint64_t s;
    uint64_t next(uint64_t n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (s >> 33) % n;
    }
};

static const void* at(uint64_t a) { return reinterpret_cast<const void*>((uintptr_t)a); }
static uint64_t addr(const void* p) { return (uint64_t)(uintptr_t)p; }

// the rule, written out: 128-bit intervals, every pair compared
static bool brute(const std::vector<ShardRange>& list, uint64_t total) {
    struct I { u128 lo, hi; };
    std::vector<I> v;
    for (const ShardRange& s : list) {
        v.push_back(I{(u128)addr(s.ranks), (u128)addr(s.ranks) + (u128)2 * total * s.stride});
        if (!s.shard) continue;
        const uint64_t blk = s.n / total;
        for (uint64_t b = 0; b < total; ++b) {
            const u128 lo = (u128)addr(s.shard) + (u128)2 * b * s.shard_stride;
            v.push_back(I{lo, lo + (u128)2 * blk});
        }
    }
    for (const I& i : v)
        if (i.hi > i.lo && i.hi > (u128)UINTPTR_MAX) return false;
    for (size_t i = 0; i < v.size(); ++i)
        for (size_t j = i + 1; j < v.size(); ++j)
            if (v[i].lo < v[j].hi && v[j].lo < v[i].hi) return false;
    return true;
}

// compares the verdicts; want: 1 must be accepted, 0 must be refused, -1 whatever brute force says
static void check(const char* what, const std::vector<ShardRange>& list, uint64_t total, int want) {
    const bool got = tsa::shard_lists_disjoint(list.data(), (int)list.size(), total);
    const bool ref = brute(list, total);
    ++g_lists;
    ++(ref ? g_accepted : g_refused);
    if (got != ref || (want >= 0 && ref != (want == 1))) {
        std::printf("MISMATCH %s: count=%zu total=%llu got=%d brute=%d want=%d\n", what, list.size(),
                    (unsigned long long)total, (int)got, (int)ref, want);
        for (const ShardRange& s : list)
            std::printf("  ranks=%llx stride=%llu n=%llu shard=%llx shard_stride=%llu\n", (unsigned long long)addr(s.ranks),
                        (unsigned long long)s.stride, (unsigned long long)s.n, (unsigned long long)addr(s.shard),
                        (unsigned long long)s.shard_stride);
        std::exit(1);
    }
}

enum Layout { COMPACT, FLAT, WIDE, LAYOUTS };

// an accepted list: rank rows in buffers of their own (every other one with a stride skew), the
// shards in `layout`; every fourth bucket (not the first) without a shard
static std::vector<ShardRange> make(Rng& rng, int count, uint64_t total, Layout layout) {
    std::vector<ShardRange> list((size_t)count);
    uint64_t cursor = (1ull << 40) + 16 * rng.next(1000);
    for (int i = 0; i < count; ++i) {
        ShardRange& s = list[(size_t)i];
        s.n = 8 * total * (1 + rng.next(40));
        s.stride = s.n + (i % 2 ? 64 : 0);
        s.ranks = at(cursor);
        cursor += 2 * total * s.stride + 16 * rng.next(8);
        s.shard = nullptr;
        s.shard_stride = 0;
    }
    auto has_shard = [](int i) { return i % 4 != 3; };
    if (layout == COMPACT) {
        for (int i = 0; i < count; ++i) {
            if (!has_shard(i)) continue;
            ShardRange& s = list[(size_t)i];
            s.shard = at(cursor);
            s.shard_stride = s.n / total;
            cursor += 2 * s.n + 16 * rng.next(4);
        }
    } else if (layout == FLAT) {   // one row of F elements per rank, bucket i's blocks at column off_i
        uint64_t F = 0;
        for (int i = 0; i < count; ++i)
            if (has_shard(i)) F += list[(size_t)i].n / total;
        F += 8 * rng.next(3);   // a row may be longer than its blocks
        uint64_t off = 0;
        for (int i = 0; i < count; ++i) {
            if (!has_shard(i)) continue;
            ShardRange& s = list[(size_t)i];
            s.shard = at(cursor + 2 * off);
            s.shard_stride = F;
            off += s.n / total;
        }
        cursor += 2 * total * F;
    } else {   // WIDE: groups of up to three buckets share one region, each in the gaps of the others
        for (int i = 0; i < count;) {
            int members[3], m = 0;
            uint64_t pitch = 0;
            while (i < count && m < 3) {
                if (has_shard(i)) {
                    members[m++] = i;
                    pitch += list[(size_t)i].n / total;
                }
                ++i;
            }
            pitch += 64;   // and a gap nobody uses
            uint64_t off = 0;
            for (int k = 0; k < m; ++k) {
                ShardRange& s = list[(size_t)members[k]];
                s.shard = at(cursor + 2 * off);
                s.shard_stride = pitch;
                off += s.n / total;
            }
            cursor += 2 * total * pitch;
        }
    }
    return list;
}

// bucket i's shard moved so that its block b covers the byte `target`
static void move_block_onto(ShardRange& s, uint64_t b, uint64_t target, uint64_t total, Rng& rng) {
    const uint64_t blk = s.n / total;
    const uint64_t inside = 2 * rng.next(blk);   // the byte's offset inside the block
    s.shard = at(target - inside - 2 * b * s.shard_stride);
}

static void mutants(Rng& rng, const std::vector<ShardRange>& good, uint64_t total) {
    std::vector<int> with;
    for (size_t i = 0; i < good.size(); ++i)
        if (good[i].shard) with.push_back((int)i);
    if (with.empty()) return;
    const int i = with[rng.next(with.size())];
    const uint64_t b = rng.next(total);
    {   // a byte of a rank row's data, of any bucket (its own included)
        std::vector<ShardRange> bad = good;
        const ShardRange& t = good[rng.next(good.size())];
        move_block_onto(bad[(size_t)i], b, addr(t.ranks) + 2 * (rng.next(total) * t.stride + rng.next(t.n)), total, rng);
        check("block on a rank row", bad, total, 0);
    }
    for (const ShardRange& t : good) {   // a byte of a stride skew (the first bucket that has one)
        if (t.stride == t.n) continue;
        std::vector<ShardRange> bad = good;
        move_block_onto(bad[(size_t)i], b, addr(t.ranks) + 2 * (rng.next(total) * t.stride + t.n + rng.next(t.stride - t.n)),
                        total, rng);
        check("block on a skew", bad, total, 0);
        break;
    }
    if (with.size() > 1) {   // a byte of another shard's block
        int k = i;
        while (k == i) k = with[rng.next(with.size())];
        const ShardRange& t = good[(size_t)k];
        std::vector<ShardRange> bad = good;
        move_block_onto(bad[(size_t)i], b, addr(t.shard) + 2 * (rng.next(total) * t.shard_stride + rng.next(t.n / total)),
                        total, rng);
        check("block on another shard's block", bad, total, 0);
    }
    {   // the same shard twice: another bucket (a new one when there is none) names bucket i's shard
        std::vector<ShardRange> bad = good;
        if (bad.size() > 1) {
            const size_t k = ((size_t)i + 1 + rng.next(bad.size() - 1)) % bad.size();
            bad[k].shard = bad[(size_t)i].shard;
            bad[k].shard_stride = bad[(size_t)i].shard_stride > bad[k].n / total ? bad[(size_t)i].shard_stride : bad[k].n / total;
        } else {
            ShardRange twin = bad[0];
            twin.ranks = at(addr(twin.ranks) - 2 * total * twin.stride - 64);
            bad.push_back(twin);
        }
        check("the same shard twice", bad, total, 0);
    }
}

int main() {
    Rng rng{20250311};
    const uint64_t totals[] = {8, 16, 64};
    for (int rep = 0; rep < 90; ++rep) {
        const uint64_t total = totals[rep % 3];
        const Layout layout = (Layout)((rep / 3) % LAYOUTS);
        const int count = rep < 9 ? 64 : 1 + (int)rng.next(64);
        const std::vector<ShardRange> good = make(rng, count, total, layout);
        check(layout == COMPACT ? "compact" : layout == FLAT ? "flat" : "wide", good, total, 1);
        for (int m = 0; m < 3; ++m) mutants(rng, good, total);
    }
    // one bucket, no shard; an empty list
    {
        std::vector<ShardRange> one = {ShardRange{at(1ull << 40), 1024, 1024, nullptr, 0}};
        check("one bucket", one, 8, 1);
        if (!tsa::shard_lists_disjoint(nullptr, 0, 8)) {
            std::printf("MISMATCH an empty list refused\n");
            return 1;
        }
    }
    // a shard_stride below blk: the shard's own blocks overlap
    {
        std::vector<ShardRange> self = {ShardRange{at(1ull << 40), 1024, 1024, at(1ull << 41), 120}};
        check("shard_stride < blk", self, 8, 0);
    }
    // two rank-row ranges overlapping, with and without shards elsewhere in the list
    {
        std::vector<ShardRange> rows = {ShardRange{at(1ull << 40), 1024, 1024, nullptr, 0},
                                        ShardRange{at((1ull << 40) + 2 * 1024 * 3), 1024, 1024, nullptr, 0}};
        check("rank rows overlap", rows, 8, 0);
        rows.push_back(ShardRange{at(1ull << 42), 1024, 1024, at(1ull << 43), 128});
        check("rank rows overlap, a shard elsewhere", rows, 8, 0);
    }
    // one bucket's rank rows inside a gap of another bucket's wide shard: accepted; a byte further, on a block: refused
    {
        const uint64_t big = 1ull << 40, shard = 1ull << 41;   // 8 blocks of 128 elements, 4096 elements apart
        for (int64_t d : {0, 2, -2}) {
            const uint64_t rows_at = shard + 2 * 128 + (uint64_t)(d < 0 ? d : 0);   // right behind block 0
            const uint64_t stride = (4096 - 128) / 8 + (uint64_t)(d > 0 ? 8 : 0);   // 8 rows fill the gap exactly
            std::vector<ShardRange> gap = {ShardRange{at(big), 1024, 1024, at(shard), 4096},
                                           ShardRange{at(rows_at), stride, 64, nullptr, 0}};
            check("rank rows in a shard's gap", gap, 8, d == 0 ? 1 : 0);
        }
    }
    // the top of the address space: the last block, or the last row, ending at, before and past UINTPTR_MAX
    for (uint64_t total : totals) {
        const uint64_t n = 256 * total, blk = 256, top = (uint64_t)UINTPTR_MAX;
        for (uint64_t ss : {blk, blk + 64, (uint64_t)4096}) {
            const uint64_t span = 2 * ((total - 1) * ss + blk);
            for (int64_t d : {-32, -2, -1, 0, 1, 2, 16, 2 * 256 - 2, 2 * 256, 2 * 256 + 16}) {
                std::vector<ShardRange> edge = {ShardRange{at(1ull << 40), n, n, at(top - span + (uint64_t)d), ss}};
                check("shard at the top", edge, total, d <= 0 ? 1 : 0);
            }
        }
        for (int64_t d : {-16, -1, 0, 1, 16}) {
            std::vector<ShardRange> edge = {ShardRange{at(top - 2 * total * n + (uint64_t)d), n, n, nullptr, 0}};
            check("rank rows at the top", edge, total, d <= 0 ? 1 : 0);
        }
        // products past 2^64: they must be refused, not wrap into a small range
        std::vector<ShardRange> wrap = {ShardRange{at(1ull << 40), n, n, at(1ull << 41), (1ull << 63) / total * 2}};
        check("shard_stride wraps", wrap, total, 0);
        wrap[0].shard_stride = ~0ull - 7;
        check("shard_stride near 2^64", wrap, total, 0);
        wrap[0] = ShardRange{at(1ull << 40), (1ull << 63) / total + 8, n, nullptr, 0};
        check("rank_stride wraps", wrap, total, 0);
    }
    if (g_accepted < 90 || g_refused < 300) {
        std::printf("MISMATCH the lists do not reach both verdicts: %llu accepted, %llu refused\n", g_accepted, g_refused);
        return 1;
    }
    std::printf("shard_ranges ok: %llu lists, %llu accepted, %llu refused\n", g_lists, g_accepted, g_refused);
    return 0;
}
"""


LAYOUT = r"""
#include <cstddef>
#include <cstdio>
#include "allred.h"
int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %d %d\n", sizeof(allred_shard_bucket), offsetof(allred_shard_bucket, ranks),
                offsetof(allred_shard_bucket, rank_stride), offsetof(allred_shard_bucket, elems_per_rank),
                offsetof(allred_shard_bucket, shard), offsetof(allred_shard_bucket, shard_stride),
                ALLRED_OP_REDUCE_SCATTER, ALLRED_OP_ALL_GATHER);
    return 0;
}
"""


def test_shard_bucket_binding_matches_the_header(tmp_path):
    """_lib.ShardBucket mirrors allred_shard_bucket, and the two op constants agree."""
    import ctypes as C

    from tenstorrentallreduce_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    b = _lib.ShardBucket
    assert out == [C.sizeof(b), b.ranks.offset, b.rank_stride.offset, b.elems_per_rank.offset, b.shard.offset,
                   b.shard_stride.offset, _lib.OP_REDUCE_SCATTER, _lib.OP_ALL_GATHER]


def test_shard_lists_disjoint_matches_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the shard_ranges check"
    src = tmp_path / "shard_ranges_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "shard_ranges_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "shard_ranges ok" in run.stdout
