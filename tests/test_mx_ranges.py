"""csrc/mx_ranges.hpp against brute force, on the CPU.

A stand-alone C++ program (its own main) is compiled with g++ under AddressSanitizer and UBSan and run
directly.  For every list of MXFP8 buckets it compares mx_lists_disjoint — the disjointness rule of
allred_plan_all_gather_shards_mxfp8 — with the rule written out in unsigned 128-bit arithmetic: per
bucket the element rows are ONE interval [rows, rows + total row_stride), the scale rows ONE interval
[scales, scales + total scale_stride), the shard its `total` SEPARATE block intervals
[shard + 4 b shard_stride, + 4 blk); a list is accepted when every interval ends at or below
UINTPTR_MAX and no two of them (every pair is tested) share a byte.

Lists: random ones of 1 .. 32 buckets at 8 / 16 / 64 ranks, the addresses made up (nothing is
dereferenced), with the shards compact, flat (one rank-major buffer) or wide — and then the element
rows or the scale rows of a bucket inside the gap of its own wide shard: accepted.  Mutants: scale rows
moved onto the last byte of their own or another bucket's element rows, of a stride skew, of a shard
block; element rows onto scale rows; one bucket's scales onto another's rows: refused.  Rows that fill
a gap exactly and one byte-quantum off, the top of the address space, strides whose doubling or
products pass 2^64 — and every argument rule of mx_list_verdict that needs no plan.
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

#include "mx_ranges.hpp"

typedef unsigned __int128 u128;
using tsa::MxRange;

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
static bool brute(const std::vector<MxRange>& list, uint64_t total) {
    struct I { u128 lo, hi; };
    std::vector<I> v;
    for (const MxRange& s : list) {
        v.push_back(I{(u128)addr(s.rows), (u128)addr(s.rows) + (u128)total * s.row_stride});
        v.push_back(I{(u128)addr(s.scales), (u128)addr(s.scales) + (u128)total * s.scale_stride});
        const uint64_t blk = s.n / total;
        if (total > 1 && s.shard_stride < blk) return false;
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

static void dump(const std::vector<MxRange>& list) {
    for (const MxRange& s : list)
        std::printf("  rows=%llx/%llu scales=%llx/%llu n=%llu shard=%llx/%llu\n", (unsigned long long)addr(s.rows),
                    (unsigned long long)s.row_stride, (unsigned long long)addr(s.scales), (unsigned long long)s.scale_stride,
                    (unsigned long long)s.n, (unsigned long long)addr(s.shard), (unsigned long long)s.shard_stride);
}

// compares the verdicts; want: 1 must be accepted, 0 must be refused, -1 whatever brute force says
static void check(const char* what, const std::vector<MxRange>& list, uint64_t total, int want) {
    const bool got = tsa::mx_lists_disjoint(list.data(), (int)list.size(), total);
    const bool ref = brute(list, total);
    ++g_lists;
    ++(ref ? g_accepted : g_refused);
    if (got != ref || (want >= 0 && ref != (want == 1))) {
        std::printf("MISMATCH %s: count=%zu total=%llu got=%d brute=%d want=%d\n", what, list.size(), (unsigned long long)total,
                    (int)got, (int)ref, want);
        dump(list);
        std::exit(1);
    }
}

// mx_list_verdict: the disjointness verdict must be brute force's whenever the argument rules hold
static void verdict(const char* what, const std::vector<MxRange>& list, uint64_t total, tsa::MxVerdict want) {
    const tsa::MxVerdict got = tsa::mx_list_verdict(list.data(), (int)list.size(), total);
    ++g_lists;
    ++(got == tsa::kMxOk ? g_accepted : g_refused);
    if (got != want) {
        std::printf("MISMATCH verdict %s: got=%d want=%d\n", what, (int)got, (int)want);
        dump(list);
        std::exit(1);
    }
}

enum Layout { COMPACT, FLAT, WIDE, LAYOUTS };

// an accepted list: element rows and scale rows in buffers of their own (every other one with a stride
// skew), the shards in `layout`; WIDE: a bucket's own rows or scales sit in the gap behind its block 0
static std::vector<MxRange> make(Rng& rng, int count, uint64_t total, Layout layout) {
    std::vector<MxRange> list((size_t)count);
    uint64_t cursor = (1ull << 40) + 16 * rng.next(1000);
    for (int i = 0; i < count; ++i) {
        MxRange& s = list[(size_t)i];
        s.n = 256 * total * (1 + rng.next(6));
        s.row_stride = s.n + (i % 2 ? 16 * (1 + rng.next(4)) : 0);
        s.scale_stride = s.n / 32 + (i % 3 == 1 ? 8 * (1 + rng.next(4)) : 0);
        s.rows = at(cursor);
        cursor += total * s.row_stride + 16 * rng.next(8);
        s.scales = at(cursor);
        cursor += total * s.scale_stride;
        cursor = (cursor + 15) / 16 * 16 + 16 * rng.next(8);
    }
    if (layout == COMPACT) {
        for (int i = 0; i < count; ++i) {
            MxRange& s = list[(size_t)i];
            s.shard = at(cursor);
            s.shard_stride = s.n / total;
            cursor += 4 * s.n + 16 * rng.next(4);
        }
    } else if (layout == FLAT) {   // one row of F floats per rank, bucket i's blocks at column off_i
        uint64_t F = 0;
        for (int i = 0; i < count; ++i) F += list[(size_t)i].n / total;
        F += 4 * rng.next(3);
        uint64_t off = 0;
        for (int i = 0; i < count; ++i) {
            MxRange& s = list[(size_t)i];
            s.shard = at(cursor + 4 * off);
            s.shard_stride = F;
            off += s.n / total;
        }
        cursor += 4 * total * F;
    } else {   // WIDE: the gap behind block 0 holds the bucket's whole element-row or scale-row interval
        for (int i = 0; i < count; ++i) {
            MxRange& s = list[(size_t)i];
            const uint64_t blk = s.n / total;
            const bool rows_in = i % 2 == 0;
            const uint64_t inner = rows_in ? total * s.row_stride : total * s.scale_stride;   // bytes, a multiple of 16 / 8
            s.shard = at(cursor);
            s.shard_stride = blk + (inner + 15) / 16 * 4 + 4 * rng.next(3);
            (rows_in ? s.rows : s.scales) = at(cursor + 4 * blk);
            cursor += 4 * total * s.shard_stride + 16 * rng.next(4);
        }
    }
    return list;
}

static void mutants(Rng& rng, const std::vector<MxRange>& good, uint64_t total) {
    const size_t i = rng.next(good.size()), k = rng.next(good.size());
    const MxRange& t = good[k];
    const uint64_t r = rng.next(total);
    {   // scale rows whose FIRST byte is the last byte of an element row's data (its own bucket's when k == i)
        std::vector<MxRange> bad = good;
        bad[i].scales = at(addr(t.rows) + r * t.row_stride + t.n - 1);
        check("scales on the last byte of a row", bad, total, 0);
    }
    {   // ... the last byte of the whole row interval (data or skew)
        std::vector<MxRange> bad = good;
        bad[i].scales = at(addr(t.rows) + total * t.row_stride - 1);
        check("scales on the last byte of a row interval", bad, total, 0);
    }
    {   // element rows that END one byte inside a scale-row interval
        std::vector<MxRange> bad = good;
        bad[i].rows = at(addr(t.scales) + 1 - total * bad[i].row_stride);
        check("rows ending on the first byte of scales", bad, total, 0);
    }
    {   // scale rows on the last byte of a shard block
        std::vector<MxRange> bad = good;
        bad[i].scales = at(addr(t.shard) + 4 * (r * t.shard_stride + t.n / total) - 1);
        check("scales on the last byte of a shard block", bad, total, 0);
    }
    {   // a shard block on the last byte of a scale row interval
        std::vector<MxRange> bad = good;
        bad[i].shard = at(addr(t.scales) + total * t.scale_stride - 1 - 4 * r * bad[i].shard_stride);
        check("a shard block on the last byte of scales", bad, total, 0);
    }
    if (good.size() > 1 && k != i) {   // one bucket's scales ARE another's rows
        std::vector<MxRange> bad = good;
        bad[i].scales = t.rows;
        check("one bucket's scales on another's rows", bad, total, 0);
        bad = good;
        bad[i].scales = t.scales;
        check("the same scale rows twice", bad, total, 0);
    }
    {   // rows on scales inside one bucket
        std::vector<MxRange> bad = good;
        bad[i].rows = bad[i].scales;
        check("a bucket's rows on its scales", bad, total, 0);
    }
}

int main() {
    Rng rng{20260117};
    const uint64_t totals[] = {8, 16, 64};
    for (int rep = 0; rep < 90; ++rep) {
        const uint64_t total = totals[rep % 3];
        const Layout layout = (Layout)((rep / 3) % LAYOUTS);
        const int count = rep < 9 ? 32 : 1 + (int)rng.next(32);
        const std::vector<MxRange> good = make(rng, count, total, layout);
        check(layout == COMPACT ? "compact" : layout == FLAT ? "flat" : "wide", good, total, 1);
        verdict("a good list", good, total, tsa::kMxOk);
        for (int m = 0; m < 3; ++m) mutants(rng, good, total);
    }
    if (!tsa::mx_lists_disjoint(nullptr, 0, 8) || tsa::mx_list_verdict(nullptr, 0, 8) != tsa::kMxOk) {
        std::printf("MISMATCH an empty list refused\n");
        return 1;
    }
    // the mapping itself: three ShardRanges per bucket, the halvings and doublings where they belong
    {
        const MxRange one{at(1ull << 40), 2064, at(1ull << 41), 72, 2048, at(1ull << 42), 260};
        std::vector<tsa::ShardRange> out;
        if (!tsa::mx_as_ranges(&one, 1, &out) || out.size() != 3 || out[0].ranks != one.rows || out[0].stride != 1032 ||
            out[0].n != 1024 || out[0].shard || out[1].ranks != one.scales || out[1].stride != 36 || out[1].n != 32 ||
            out[1].shard || out[2].ranks || out[2].stride != 0 || out[2].n != 4096 || out[2].shard != one.shard ||
            out[2].shard_stride != 520) {
            std::printf("MISMATCH the 2-byte view of one bucket\n");
            return 1;
        }
    }
    // Scale rows that fill a wide shard's gap exactly: 8 blocks of 256 floats (1024 bytes) 384 floats (1536
    // bytes) apart; the gap behind block 0 is 512 bytes = the 8 scale rows of 64 bytes of a bucket of n = 2048.
    // Accepted; 8 bytes earlier (on block 0's tail) or a scale_stride 8 longer (on block 1's head): refused.
    {
        const uint64_t shard = 1ull << 41;
        for (int d : {0, 8, -8}) {
            std::vector<MxRange> gap = {MxRange{at(1ull << 40), 2048, at(1ull << 39), 64, 2048, at(shard), 384},
                                        MxRange{at(1ull << 38), 2048, at(shard + 1024 - (d < 0 ? 8 : 0)), 64u + (d > 0 ? 8 : 0), 2048,
                                                at(1ull << 37), 256}};
            check("another bucket's scale rows in a shard's gap", gap, 8, d == 0 ? 1 : 0);
            verdict("another bucket's scale rows in a shard's gap", gap, 8, d == 0 ? tsa::kMxOk : tsa::kMxArg);
        }
        // ... and a bucket's element rows in its OWN shard's gap: stride 256 + 4096 floats, the gap 16384 bytes = 8 rows
        // of 2048 bytes
        for (int d : {0, 16, -16}) {
            std::vector<MxRange> gap = {MxRange{at(shard + 1024 - (d < 0 ? 16 : 0)), 2048u + (d > 0 ? 16 : 0), at(1ull << 39), 64, 2048,
                                                at(shard), 256 + 4096}};
            check("a bucket's element rows in its own shard's gap", gap, 8, d == 0 ? 1 : 0);
            verdict("a bucket's element rows in its own shard's gap", gap, 8, d == 0 ? tsa::kMxOk : tsa::kMxArg);
        }
    }
    // the top of the address space: the scale rows, the element rows and the last shard block ending at,
    // before and past UINTPTR_MAX
    for (uint64_t total : totals) {
        const uint64_t n = 256 * total, top = (uint64_t)UINTPTR_MAX;
        for (int64_t d : {-64, -8, -1, 0, 1, 8, 64}) {
            std::vector<MxRange> edge = {MxRange{at(1ull << 40), n, at(top - total * (n / 32) + (uint64_t)d), n / 32, n, at(1ull << 41), 256}};
            check("scales at the top", edge, total, d <= 0 ? 1 : 0);
            edge = {MxRange{at(top - total * n + (uint64_t)d), n, at(1ull << 40), n / 32, n, at(1ull << 41), 256}};
            check("rows at the top", edge, total, d <= 0 ? 1 : 0);
            const uint64_t span = 4 * ((total - 1) * 320 + 256);
            edge = {MxRange{at(1ull << 40), n, at(1ull << 39), n / 32, n, at(top - span + (uint64_t)d), 320}};
            check("shard at the top", edge, total, d <= 0 ? 1 : 0);
        }
        // doublings and products past 2^64: refused, not wrapped into a small range
        std::vector<MxRange> wrap = {MxRange{at(1ull << 40), n, at(1ull << 39), n / 32, n, at(1ull << 41), 1ull << 63}};
        check("2 shard_stride wraps", wrap, total, 0);
        wrap[0].shard_stride = (1ull << 62) / total * 2;
        check("4 total shard_stride wraps", wrap, total, 0);
        wrap[0].shard_stride = 256;
        wrap[0].row_stride = (1ull << 63) / total * 2 + 16;
        check("total row_stride wraps", wrap, total, 0);
        wrap[0].row_stride = n;
        wrap[0].scale_stride = (1ull << 63) / total * 2 + 8;
        check("total scale_stride wraps", wrap, total, 0);
        wrap[0].scale_stride = n / 32;
        wrap[0].n = 1ull << 63;
        wrap[0].row_stride = wrap[0].n;
        wrap[0].scale_stride = wrap[0].n / 32;
        wrap[0].shard_stride = wrap[0].n / total;
        check("2 n wraps", wrap, total, 0);
        verdict("n past the tile cap", wrap, total, tsa::kMxArg);
    }
    // every argument rule that needs no plan
    {
        const uint64_t total = 8, n = 2048;
        const MxRange ok{at(1ull << 40), n, at(1ull << 39), n / 32, n, at(1ull << 41), 256};
        auto with = [&](auto&& change) {
            MxRange m = ok;
            change(m);
            return std::vector<MxRange>{m};
        };
        verdict("the plain bucket", with([](MxRange&) {}), total, tsa::kMxOk);
        verdict("rows NULL", with([](MxRange& m) { m.rows = nullptr; }), total, tsa::kMxArg);
        verdict("scales NULL", with([](MxRange& m) { m.scales = nullptr; }), total, tsa::kMxArg);
        verdict("shard NULL", with([](MxRange& m) { m.shard = nullptr; }), total, tsa::kMxArg);
        verdict("rows 8-byte aligned only", with([](MxRange& m) { m.rows = at((1ull << 40) + 8); }), total, tsa::kMxArg);
        verdict("scales 4-byte aligned only", with([](MxRange& m) { m.scales = at((1ull << 39) + 4); }), total, tsa::kMxArg);
        verdict("scales 8-byte aligned", with([](MxRange& m) { m.scales = at((1ull << 39) + 8); }), total, tsa::kMxOk);
        verdict("shard 8-byte aligned only", with([](MxRange& m) { m.shard = at((1ull << 41) + 8); }), total, tsa::kMxArg);
        verdict("n == 0", with([](MxRange& m) { m.n = 0; }), total, tsa::kMxArg);
        verdict("n % (8 total) != 0", with([](MxRange& m) { m.n = 2048 + 32; m.row_stride = 4096; m.scale_stride = 128; m.shard_stride = 512; }), total, tsa::kMxArg);
        verdict("row_stride < n", with([](MxRange& m) { m.row_stride = 2048 - 16; }), total, tsa::kMxArg);
        verdict("row_stride % 16 != 0", with([](MxRange& m) { m.row_stride = 2048 + 8; }), total, tsa::kMxArg);
        verdict("row_stride wide", with([](MxRange& m) { m.row_stride = 2048 + 16; }), total, tsa::kMxOk);
        verdict("scale_stride < n / 32", with([](MxRange& m) { m.scale_stride = 56; }), total, tsa::kMxArg);
        verdict("scale_stride % 8 != 0", with([](MxRange& m) { m.scale_stride = 68; }), total, tsa::kMxArg);
        verdict("scale_stride wide", with([](MxRange& m) { m.scale_stride = 72; }), total, tsa::kMxOk);
        verdict("shard_stride < blk", with([](MxRange& m) { m.shard_stride = 252; }), total, tsa::kMxArg);
        verdict("shard_stride % 4 != 0", with([](MxRange& m) { m.shard_stride = 258; }), total, tsa::kMxArg);
        verdict("not whole tiles", with([](MxRange& m) { m.n = 1024; }), total, tsa::kMxUnsupported);
        verdict("total < 8", with([](MxRange& m) { m.n = 1024; m.shard_stride = 256; }), 4, tsa::kMxUnsupported);
        verdict("an empty list", {}, total, tsa::kMxOk);
        if (tsa::mx_list_verdict(&ok, -1, total) != tsa::kMxArg || tsa::mx_list_verdict(nullptr, 1, total) != tsa::kMxArg ||
            tsa::mx_list_verdict(&ok, 1, 0) != tsa::kMxArg) {
            std::printf("MISMATCH count < 0, a NULL list or total == 0 accepted\n");
            return 1;
        }
        // an ARG fault wins over the shape: a bucket that is not whole tiles AND overlaps
        verdict("not whole tiles and rows on scales",
                with([](MxRange& m) { m.n = 1024; m.scales = m.rows; }), total, tsa::kMxArg);
        // the tile cap: two buckets of 2^30 tiles fit, a third tile more does not (addresses far apart; nothing is touched)
        const uint64_t big = 256ull << 30;
        std::vector<MxRange> cap = {MxRange{at(1ull << 50), big, at(1ull << 49), big / 32, big, at(1ull << 52), big / 8},
                                    MxRange{at(1ull << 54), big - 2048, at(1ull << 48), big / 32, big - 2048, at(1ull << 56), big / 8}};
        verdict("2^31 - 8 tiles", cap, total, tsa::kMxOk);
        cap.push_back(MxRange{at(1ull << 58), 2048, at(1ull << 47), 64, 2048, at(1ull << 59), 256});
        verdict("2^31 tiles", cap, total, tsa::kMxArg);
        if (!tsa::mx_flags_ok(0) || !tsa::mx_flags_ok(1) || tsa::mx_flags_ok(2) || tsa::mx_flags_ok(3) || tsa::mx_flags_ok(-2) ||
            tsa::mx_flags_ok(0x100)) {
            std::printf("MISMATCH the flag rule\n");
            return 1;
        }
    }
    if (g_accepted < 180 || g_refused < 1000) {
        std::printf("MISMATCH the lists do not reach both verdicts: %llu accepted, %llu refused\n", g_accepted, g_refused);
        return 1;
    }
    std::printf("mx_ranges ok: %llu lists, %llu accepted, %llu refused\n", g_lists, g_accepted, g_refused);
    return 0;
}
"""


LAYOUT = r"""
#include <cstddef>
#include <cstdio>
#include "allred.h"
int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(allred_mx_bucket_f32), offsetof(allred_mx_bucket_f32, rows),
                offsetof(allred_mx_bucket_f32, row_stride), offsetof(allred_mx_bucket_f32, scales),
                offsetof(allred_mx_bucket_f32, scale_stride), offsetof(allred_mx_bucket_f32, elems_per_rank),
                offsetof(allred_mx_bucket_f32, shard), offsetof(allred_mx_bucket_f32, shard_stride),
                ALLRED_MX_GROUP_MAX, ALLRED_MX_SCALE_RCEIL);
    return 0;
}
"""


def test_mx_bucket_binding_matches_the_header(tmp_path):
    """_lib.MxBucketF32 mirrors allred_mx_bucket_f32, and the constants agree."""
    import ctypes as C

    from tenstorrentallreduce_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    b = _lib.MxBucketF32
    assert out == [C.sizeof(b), b.rows.offset, b.row_stride.offset, b.scales.offset, b.scale_stride.offset,
                   b.elems_per_rank.offset, b.shard.offset, b.shard_stride.offset, _lib.MX_GROUP_MAX, _lib.MX_SCALE_RCEIL]


def test_mxfp8_entry_points_refuse_before_any_hip_call():
    """no GPU here: a call that got as far as HIP would not return ALLRED_ERR_ARG"""
    from tenstorrentallreduce_amd import _lib
    lib = _lib.lib
    arr = (_lib.MxBucketF32 * 1)((1 << 40, 2048, 1 << 39, 64, 2048, 1 << 41, 256))
    assert lib.allred_plan_all_gather_shards_mxfp8(None, arr, 1, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8(None, arr, 1, 2, None) == _lib.ERR_ARG
    assert lib.allred_plan_all_gather_shards_mxfp8_launches(None, arr, 1) == _lib.ERR_ARG


def test_mx_lists_disjoint_matches_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the mx_ranges check"
    src = tmp_path / "mx_ranges_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "mx_ranges_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mx_ranges ok" in run.stdout
