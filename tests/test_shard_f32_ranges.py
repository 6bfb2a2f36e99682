"""csrc/shard_f32_ranges.hpp against brute force, on the CPU.

A stand-alone C++ program (its own main) is compiled with g++ under AddressSanitizer and UBSan
and run directly.  For every list of fp32-shard buckets it compares shard_f32_lists_disjoint —
the disjointness rule of allred_plan_reduce_scatter_shards_f32 / allred_plan_all_gather_shards_f32
— with the rule written out in unsigned 128-bit arithmetic: every bucket's rank rows are ONE
interval [ranks, ranks + 2 total stride) (bf16), every shard is its `total` SEPARATE block
intervals [shard + 4 b shard_stride, + 4 blk) (fp32); a list is accepted when every interval
ends at or below UINTPTR_MAX and no two of them (every pair is tested) share a byte.

Lists: random ones of 1 .. 64 buckets at 8 / 16 / 64 ranks, the addresses made up (nothing is
dereferenced), compact (shard_stride = blk), wide (the blocks of other buckets in the gaps) and
flat (one rank-major fp32 buffer, shard_stride = F): accepted.  Mutants that move one fp32
block onto the LAST byte of another block, of a rank row or of a stride skew, or that name one
shard twice: refused.  A rank row that fills a wide shard's gap exactly, in bytes: accepted;
the same row two bytes off, either way: refused.  Shards within 4 blk bytes of the top of the
address space, and strides whose doubling or products pass 2^64.
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

#include "shard_f32_ranges.hpp"

typedef unsigned __int128 u128;
using tsa::ShardF32Range;

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

// the rule, written out: 128-bit byte intervals, every pair compared
static bool brute(const std::vector<ShardF32Range>& list, uint64_t total) {
    struct I { u128 lo, hi; };
    std::vector<I> v;
    for (const ShardF32Range& s : list) {
        v.push_back(I{(u128)addr(s.ranks), (u128)addr(s.ranks) + (u128)2 * total * s.stride});
        if (!s.shard) continue;
        const uint64_t blk = s.n / total;
        for (uint64_t b = 0; b < total; ++b) {
            const u128 lo = (u128)addr(s.shard) + (u128)4 * b * s.shard_stride;
            v.push_back(I{lo, lo + (u128)4 * blk});
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
static void check(const char* what, const std::vector<ShardF32Range>& list, uint64_t total, int want) {
    const bool got = tsa::shard_f32_lists_disjoint(list.data(), (int)list.size(), total);
    const bool ref = brute(list, total);
    ++g_lists;
    ++(ref ? g_accepted : g_refused);
    if (got != ref || (want >= 0 && ref != (want == 1))) {
        std::printf("MISMATCH %s: count=%zu total=%llu got=%d brute=%d want=%d\n", what, list.size(),
                    (unsigned long long)total, (int)got, (int)ref, want);
        for (const ShardF32Range& s : list)
            std::printf("  ranks=%llx stride=%llu n=%llu shard=%llx shard_stride=%llu\n", (unsigned long long)addr(s.ranks),
                        (unsigned long long)s.stride, (unsigned long long)s.n, (unsigned long long)addr(s.shard),
                        (unsigned long long)s.shard_stride);
        std::exit(1);
    }
}

enum Layout { COMPACT, FLAT, WIDE, LAYOUTS };

// an accepted list: rank rows in buffers of their own (every other one with a stride skew), every
// bucket with an fp32 shard in `layout`
static std::vector<ShardF32Range> make(Rng& rng, int count, uint64_t total, Layout layout) {
    std::vector<ShardF32Range> list((size_t)count);
    uint64_t cursor = (1ull << 40) + 16 * rng.next(1000);
    for (int i = 0; i < count; ++i) {
        ShardF32Range& s = list[(size_t)i];
        s.n = 8 * total * (1 + rng.next(40));
        s.stride = s.n + (i % 2 ? 64 : 0);
        s.ranks = at(cursor);
        cursor += 2 * total * s.stride + 16 * rng.next(8);
    }
    if (layout == COMPACT) {
        for (int i = 0; i < count; ++i) {
            ShardF32Range& s = list[(size_t)i];
            s.shard = at(cursor);
            s.shard_stride = s.n / total;
            cursor += 4 * s.n + 16 * rng.next(4);
        }
    } else if (layout == FLAT) {   // one row of F floats per rank, bucket i's blocks at column off_i
        uint64_t F = 0;
        for (int i = 0; i < count; ++i) F += list[(size_t)i].n / total;
        F += 4 * rng.next(3);   // a row may be longer than its blocks
        uint64_t off = 0;
        for (int i = 0; i < count; ++i) {
            ShardF32Range& s = list[(size_t)i];
            s.shard = at(cursor + 4 * off);
            s.shard_stride = F;
            off += s.n / total;
        }
        cursor += 4 * total * F;
    } else {   // WIDE: groups of up to three buckets share one region, each in the gaps of the others
        for (int i = 0; i < count;) {
            int members[3], m = 0;
            uint64_t pitch = 0;
            while (i < count && m < 3) {
                members[m++] = i;
                pitch += list[(size_t)i].n / total;
                ++i;
            }
            pitch += 64;   // and a gap nobody uses
            uint64_t off = 0;
            for (int k = 0; k < m; ++k) {
                ShardF32Range& s = list[(size_t)members[k]];
                s.shard = at(cursor + 4 * off);
                s.shard_stride = pitch;
                off += s.n / total;
            }
            cursor += 4 * total * pitch;
        }
    }
    return list;
}

// the shard moved so that the FIRST byte of its block b is the byte `target`: target the last byte of
// something else, the two share exactly that byte
static void first_byte_onto(ShardF32Range& s, uint64_t b, uint64_t target) {
    s.shard = at(target - 4 * b * s.shard_stride);
}

static void mutants(Rng& rng, const std::vector<ShardF32Range>& good, uint64_t total) {
    const size_t i = rng.next(good.size());
    const uint64_t b = rng.next(total);
    {   // the last byte of a rank row's data, of any bucket (its own included)
        std::vector<ShardF32Range> bad = good;
        const ShardF32Range& t = good[rng.next(good.size())];
        first_byte_onto(bad[i], b, addr(t.ranks) + 2 * (rng.next(total) * t.stride + t.n) - 1);
        check("block on the last byte of a rank row", bad, total, 0);
    }
    for (const ShardF32Range& t : good) {   // the last byte of a stride skew (the first bucket that has one)
        if (t.stride == t.n) continue;
        std::vector<ShardF32Range> bad = good;
        first_byte_onto(bad[i], b, addr(t.ranks) + 2 * (rng.next(total) + 1) * t.stride - 1);
        check("block on the last byte of a skew", bad, total, 0);
        break;
    }
    if (good.size() > 1) {   // the last byte of another shard's block
        size_t k = i;
        while (k == i) k = rng.next(good.size());
        const ShardF32Range& t = good[k];
        std::vector<ShardF32Range> bad = good;
        first_byte_onto(bad[i], b, addr(t.shard) + 4 * (rng.next(total) * t.shard_stride + t.n / total) - 1);
        check("block on the last byte of another block", bad, total, 0);
    }
    {   // the same shard twice: another bucket (a new one when there is none) names bucket i's shard
        std::vector<ShardF32Range> bad = good;
        if (bad.size() > 1) {
            const size_t k = (i + 1 + rng.next(bad.size() - 1)) % bad.size();
            bad[k].shard = bad[i].shard;
            bad[k].shard_stride = bad[i].shard_stride > bad[k].n / total ? bad[i].shard_stride : bad[k].n / total;
        } else {
            ShardF32Range twin = bad[0];
            twin.ranks = at(addr(twin.ranks) - 2 * total * twin.stride - 64);
            bad.push_back(twin);
        }
        check("the same shard twice", bad, total, 0);
    }
}

int main() {
    Rng rng{20250917};
    const uint64_t totals[] = {8, 16, 64};
    for (int rep = 0; rep < 90; ++rep) {
        const uint64_t total = totals[rep % 3];
        const Layout layout = (Layout)((rep / 3) % LAYOUTS);
        const int count = rep < 9 ? 64 : 1 + (int)rng.next(64);
        const std::vector<ShardF32Range> good = make(rng, count, total, layout);
        check(layout == COMPACT ? "compact" : layout == FLAT ? "flat" : "wide", good, total, 1);
        for (int m = 0; m < 3; ++m) mutants(rng, good, total);
    }
    // an empty list; a bucket without a shard maps to its rows alone
    {
        if (!tsa::shard_f32_lists_disjoint(nullptr, 0, 8)) {
            std::printf("MISMATCH an empty list refused\n");
            return 1;
        }
        std::vector<ShardF32Range> one = {ShardF32Range{at(1ull << 40), 1024, 1024, nullptr, 0}};
        check("rows alone", one, 8, 1);
    }
    // the mapping itself: two ShardRanges per bucket, the doublings where they belong
    {
        std::vector<ShardF32Range> one = {ShardF32Range{at(1ull << 40), 1088, 1024, at(1ull << 41), 132}};
        std::vector<tsa::ShardRange> out;
        if (!tsa::shard_f32_as_ranges(one.data(), 1, &out) || out.size() != 2 || out[0].ranks != one[0].ranks ||
            out[0].stride != 1088 || out[0].n != 1024 || out[0].shard || out[1].ranks || out[1].stride != 0 ||
            out[1].n != 2048 || out[1].shard != one[0].shard || out[1].shard_stride != 264) {
            std::printf("MISMATCH the 2-byte view of one bucket\n");
            return 1;
        }
    }
    // a shard_stride below blk: the shard's own blocks overlap (by one float)
    {
        std::vector<ShardF32Range> self = {ShardF32Range{at(1ull << 40), 1024, 1024, at(1ull << 41), 127}};
        check("shard_stride < blk", self, 8, 0);
    }
    // A rank row region that fills a wide shard's gap exactly, in bytes: 8 blocks of 128 floats (512
    // bytes) 4096 floats (16384 bytes) apart; the gap behind block 0 is 15872 bytes = 8 rows of 992
    // bf16.  Accepted; two bytes earlier (on block 0's last two bytes) or one stride step longer (on
    // block 1's first bytes): refused.
    {
        const uint64_t big = 1ull << 40, shard = 1ull << 41;
        for (int d : {0, 2, -2}) {
            const uint64_t rows_at = shard + 4 * 128 - (d < 0 ? 2 : 0);
            const uint64_t stride = (2 * 4096 - 2 * 128) / 8 + (d > 0 ? 8 : 0);
            std::vector<ShardF32Range> gap = {ShardF32Range{at(big), 1024, 1024, at(shard), 4096},
                                              ShardF32Range{at(rows_at), stride, 64, nullptr, 0}};
            check("rank rows in an fp32 shard's gap", gap, 8, d == 0 ? 1 : 0);
        }
        // ... and an fp32 block of another bucket in that gap, ending where block 1 begins: accepted; 4 bytes on: refused
        for (int d : {0, 4}) {
            std::vector<ShardF32Range> gap = {ShardF32Range{at(big), 1024, 1024, at(shard), 4096},
                                              ShardF32Range{at(big << 2), 512, 512, at(shard + 4 * (4096 - 64) + d), 4096}};
            check("an fp32 block in an fp32 shard's gap", gap, 8, d == 0 ? 1 : 0);
        }
    }
    // the top of the address space: the last block ending at, before and past UINTPTR_MAX
    for (uint64_t total : totals) {
        const uint64_t n = 256 * total, blk = 256, top = (uint64_t)UINTPTR_MAX;
        for (uint64_t ss : {blk, blk + 64, (uint64_t)4096}) {
            const uint64_t span = 4 * ((total - 1) * ss + blk);
            for (int64_t d : {-32, -4, -1, 0, 1, 4, 16, 4 * 256 - 4, 4 * 256, 4 * 256 + 16}) {
                std::vector<ShardF32Range> edge = {ShardF32Range{at(1ull << 40), n, n, at(top - span + (uint64_t)d), ss}};
                check("shard at the top", edge, total, d <= 0 ? 1 : 0);
            }
        }
        {   // a one-block view: total = 1 is not a grouped plan, but the rule holds — the shard within 4 blk of the top
            for (int64_t d : {-4, 0, 4, 1020, 1024}) {
                std::vector<ShardF32Range> edge = {ShardF32Range{at(1ull << 40), 256, 256, at(top - 4 * 256 + (uint64_t)d), 256}};
                check("one block at the top", edge, 1, d <= 0 ? 1 : 0);
            }
        }
        // doublings and products past 2^64: refused, not wrapped into a small range
        std::vector<ShardF32Range> wrap = {ShardF32Range{at(1ull << 40), n, n, at(1ull << 41), 1ull << 63}};
        check("2 shard_stride wraps", wrap, total, 0);
        wrap[0].shard_stride = (1ull << 62) / total * 2;
        check("4 total shard_stride wraps", wrap, total, 0);
        wrap[0].shard_stride = ~0ull - 3;
        check("shard_stride near 2^64", wrap, total, 0);
        wrap[0] = ShardF32Range{at(1ull << 40), (1ull << 63) / total + 8, n, at(1ull << 41), 256};
        check("rank_stride wraps", wrap, total, 0);
    }
    if (g_accepted < 90 || g_refused < 300) {
        std::printf("MISMATCH the lists do not reach both verdicts: %llu accepted, %llu refused\n", g_accepted, g_refused);
        return 1;
    }
    std::printf("shard_f32_ranges ok: %llu lists, %llu accepted, %llu refused\n", g_lists, g_accepted, g_refused);
    return 0;
}
"""


LAYOUT = r"""
#include <cstddef>
#include <cstdio>
#include "allred.h"
int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(allred_shard_bucket_f32), offsetof(allred_shard_bucket_f32, ranks),
                offsetof(allred_shard_bucket_f32, rank_stride), offsetof(allred_shard_bucket_f32, elems_per_rank),
                offsetof(allred_shard_bucket_f32, shard), offsetof(allred_shard_bucket_f32, shard_stride),
                ALLRED_SHARD_ACCUMULATE);
    return 0;
}
"""


def test_shard_bucket_f32_binding_matches_the_header(tmp_path):
    """_lib.ShardBucketF32 mirrors allred_shard_bucket_f32, and the flag agrees."""
    import ctypes as C

    from tenstorrentallreduce_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    b = _lib.ShardBucketF32
    assert out == [C.sizeof(b), b.ranks.offset, b.rank_stride.offset, b.elems_per_rank.offset, b.shard.offset,
                   b.shard_stride.offset, _lib.SHARD_ACCUMULATE]


def test_fp32_entry_points_refuse_before_any_hip_call():
    """no GPU here: a call that got as far as HIP would not return ALLRED_ERR_ARG"""
    from tenstorrentallreduce_amd import _lib
    lib = _lib.lib
    arr = (_lib.ShardBucketF32 * 1)((1 << 40, 2048, 2048, 1 << 41, 256))
    assert lib.allred_plan_reduce_scatter_shards_f32(None, arr, 1, 1.0, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_f32(None, arr, 1, None) == _lib.ERR_ARG
    assert lib.allred_plan_shards_f32_launches(None, arr, 1, _lib.OP_ALL_GATHER) == _lib.ERR_ARG


def test_shard_f32_lists_disjoint_matches_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the shard_f32_ranges check"
    src = tmp_path / "shard_f32_ranges_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "shard_f32_ranges_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "shard_f32_ranges ok" in run.stdout
