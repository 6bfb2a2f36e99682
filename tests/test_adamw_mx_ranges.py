"""csrc/adamw_mx_ranges.hpp against brute force, on the CPU, on tests/test_mx_ranges.py's model: a
stand-alone C++ program (its own main) compiled with g++ under AddressSanitizer and UBSan and run
directly; host code only, nothing is loaded into Python.

For every list of AdamW-MXFP8 buckets it compares adamw_mx_lists_disjoint and adamw_mx_list_verdict — the
rules of allred_plan_adamw_all_gather_shards_mxfp8 — with the rule written out in unsigned 128-bit
arithmetic: per bucket the element rows are ONE interval [rows, rows + total row_stride), the scale rows
ONE interval [scales, scales + total scale_stride), each of the four planes `total` SEPARATE block
intervals [plane + 4 b shard_stride, + 4 blk); against those [hyper, + 32 G), [norm_sq, + 4 total) and
[info, + 16); a list is accepted when every interval ends at or below UINTPTR_MAX and no two of them
(every pair is tested) share a byte.

Lists: random ones of 1 .. 12 buckets at 8 / 16 / 64 ranks, the addresses made up (nothing is
dereferenced), the planes compact, flat (four rank-major buffers) or wide.  Mutants: scales on the last
byte of a plane block; rows ending on info; hyper[G - 1] on a scale row; one bucket's scales on another's
exp_avg_sq; rows, scales and the three small buffers filling a gap exactly and one quantum off; the top
of the address space; products past 2^64 — and every argument rule of adamw_mx_list_verdict and
adamw_mx_pointers_ok that needs no plan.
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

#include "adamw_mx_ranges.hpp"

typedef unsigned __int128 u128;
using tsa::AdamwMxRange;

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

struct Small {   // 0: not given
    uint64_t hyper, G, norm_sq, info;
};
struct I { u128 lo, hi; };

// the rule, written out: 128-bit byte intervals, every pair compared
static bool brute(const std::vector<AdamwMxRange>& list, uint64_t total, const Small& sm) {
    std::vector<I> v;
    if (sm.hyper) v.push_back(I{(u128)sm.hyper, (u128)sm.hyper + (u128)32 * sm.G});
    if (sm.norm_sq) v.push_back(I{(u128)sm.norm_sq, (u128)sm.norm_sq + (u128)4 * total});
    if (sm.info) v.push_back(I{(u128)sm.info, (u128)sm.info + 16});
    for (const AdamwMxRange& s : list) {
        v.push_back(I{(u128)addr(s.rows), (u128)addr(s.rows) + (u128)total * s.row_stride});
        v.push_back(I{(u128)addr(s.scales), (u128)addr(s.scales) + (u128)total * s.scale_stride});
        const uint64_t blk = s.n / total;
        if (total > 1 && s.shard_stride < blk) return false;
        for (int k = 0; k < 4; ++k)
            for (uint64_t b = 0; b < total; ++b) {
                const u128 lo = (u128)addr(s.plane[k]) + (u128)4 * b * s.shard_stride;
                v.push_back(I{lo, lo + (u128)4 * blk});
            }
    }
    for (const I& i : v)
        if (i.hi > i.lo && i.hi > (u128)UINTPTR_MAX) return false;
    for (size_t i = 0; i < v.size(); ++i)
        for (size_t j = i + 1; j < v.size(); ++j)
            if (v[i].hi > v[i].lo && v[j].hi > v[j].lo && v[i].lo < v[j].hi && v[j].lo < v[i].hi) return false;
    return true;
}

static void dump(const std::vector<AdamwMxRange>& list, const Small& sm) {
    std::printf("  hyper=%llx x %llu norm_sq=%llx info=%llx\n", (unsigned long long)sm.hyper, (unsigned long long)sm.G,
                (unsigned long long)sm.norm_sq, (unsigned long long)sm.info);
    for (const AdamwMxRange& s : list)
        std::printf("  rows=%llx/%llu scales=%llx/%llu n=%llu planes=%llx %llx %llx %llx /%llu\n", (unsigned long long)addr(s.rows),
                    (unsigned long long)s.row_stride, (unsigned long long)addr(s.scales), (unsigned long long)s.scale_stride,
                    (unsigned long long)s.n, (unsigned long long)addr(s.plane[0]), (unsigned long long)addr(s.plane[1]),
                    (unsigned long long)addr(s.plane[2]), (unsigned long long)addr(s.plane[3]), (unsigned long long)s.shard_stride);
}

// compares the verdicts; want: 1 must be accepted, 0 must be refused, -1 whatever brute force says.  The
// lists that come here pass every other rule, so the verdict of the whole list says the same.
static void check(const char* what, const std::vector<AdamwMxRange>& list, uint64_t total, const Small& sm, int want,
                  bool with_verdict = true) {
    const bool got = tsa::adamw_mx_lists_disjoint(list.data(), (int)list.size(), total, at(sm.hyper), at(sm.norm_sq), at(sm.info), 32 * sm.G);
    const bool ref = brute(list, total, sm);
    const bool ver = with_verdict ? tsa::adamw_mx_list_verdict(list.data(), (int)list.size(), total, at(sm.hyper), at(sm.norm_sq),
                                                               at(sm.info), 32 * sm.G) == tsa::kAdamwMxOk
                                  : ref;
    ++g_checks;
    ++(ref ? g_accepted : g_refused);
    if (got != ref || ver != ref || (want >= 0 && ref != (want == 1))) {
        std::printf("MISMATCH %s: count=%zu total=%llu got=%d verdict=%d brute=%d want=%d\n", what, list.size(),
                    (unsigned long long)total, (int)got, (int)ver, (int)ref, want);
        dump(list, sm);
        std::exit(1);
    }
}

static void verdict(const char* what, const std::vector<AdamwMxRange>& list, uint64_t total, const Small& sm, tsa::AdamwMxVerdict want) {
    const tsa::AdamwMxVerdict got = tsa::adamw_mx_list_verdict(list.data(), (int)list.size(), total, at(sm.hyper), at(sm.norm_sq),
                                                               at(sm.info), 32 * sm.G);
    ++g_checks;
    ++(got == tsa::kAdamwMxOk ? g_accepted : g_refused);
    if (got != want) {
        std::printf("MISMATCH verdict %s: got=%d want=%d\n", what, (int)got, (int)want);
        dump(list, sm);
        std::exit(1);
    }
}

static void expect(const char* what, bool ok) {
    ++g_checks;
    if (!ok) {
        std::printf("MISMATCH %s\n", what);
        std::exit(1);
    }
}

enum Layout { COMPACT, FLAT, WIDE, LAYOUTS };
constexpr uint64_t kGap = 64;   // floats behind every block of a WIDE plane: 256 bytes

// an accepted list: element rows and scale rows in buffers of their own (every other one with a stride
// skew), the planes in `layout`; *end: the first byte behind everything
static std::vector<AdamwMxRange> make(Rng& rng, int count, uint64_t total, Layout layout, uint64_t* end) {
    std::vector<AdamwMxRange> list((size_t)count);
    uint64_t cursor = (1ull << 40) + 16 * rng.next(1000);
    for (int i = 0; i < count; ++i) {
        AdamwMxRange& s = list[(size_t)i];
        s.n = 256 * total * (1 + rng.next(4));
        s.row_stride = s.n + (i % 2 ? 16 * (1 + rng.next(4)) : 0);
        s.scale_stride = s.n / 32 + (i % 3 == 1 ? 8 * (1 + rng.next(4)) : 0);
        s.rows = at(cursor);
        cursor += total * s.row_stride + 16 * rng.next(8);
        s.scales = at(cursor);
        cursor += total * s.scale_stride;
        cursor = (cursor + 15) / 16 * 16 + 16 * rng.next(8);
    }
    if (layout == FLAT) {   // four rank-major buffers of F floats per rank, bucket i's blocks at column off_i
        uint64_t F = 0;
        for (int i = 0; i < count; ++i) F += list[(size_t)i].n / total;
        F += 4 * rng.next(3);
        for (int k = 0; k < 4; ++k) {
            uint64_t off = 0;
            for (int i = 0; i < count; ++i) {
                AdamwMxRange& s = list[(size_t)i];
                s.plane[k] = at(cursor + 4 * off);
                s.shard_stride = F;
                off += s.n / total;
            }
            cursor += 4 * total * F + 16 * rng.next(4);
        }
    } else {
        for (int i = 0; i < count; ++i) {
            AdamwMxRange& s = list[(size_t)i];
            s.shard_stride = s.n / total + (layout == WIDE ? kGap : 0);
            for (int k = 0; k < 4; ++k) {
                s.plane[k] = at(cursor);
                cursor += 4 * total * s.shard_stride + 16 * rng.next(4);
            }
        }
    }
    *end = cursor;
    return list;
}

static void mutants(Rng& rng, const std::vector<AdamwMxRange>& good, uint64_t total, const Small& sm, Layout layout) {
    const size_t i = rng.next(good.size()), j = rng.next(good.size());
    const AdamwMxRange& t = good[j];
    const uint64_t r = rng.next(total), blk = t.n / total, G = sm.G;
    const int k = (int)rng.next(4);
    const uint64_t block = addr(t.plane[k]) + 4 * r * t.shard_stride;
    {   // scale rows whose FIRST byte is the last byte of a plane block (any plane, any block, any bucket)
        std::vector<AdamwMxRange> bad = good;
        bad[i].scales = at(block + 4 * blk - 1);
        check("scales on the last byte of a plane block", bad, total, sm, 0, false);
        bad[i].scales = at(block + 4 * blk - 8);
        check("scales on the last 8 bytes of a plane block", bad, total, sm, 0);
    }
    {   // element rows that END on info's first byte, and up to it
        std::vector<AdamwMxRange> bad = good;
        bad[i].rows = at(sm.info + 16 - total * bad[i].row_stride);
        check("rows ending on info", bad, total, sm, 0);
        bad[i].rows = at(sm.info - total * bad[i].row_stride);
        check("rows ending at info", bad, total, sm, -1);
    }
    {   // the LAST hyper set on a scale row, the sets before it clear of it
        Small s2 = sm;
        s2.hyper = addr(t.scales) + 16 - 32 * G;
        check("hyper[G - 1] on the first bytes of the scale rows", good, total, s2, G > 1 || j > 0 ? -1 : 0);
        s2.hyper = addr(t.scales) + total * t.scale_stride - 8 - 32 * (G - 1);
        s2.hyper -= s2.hyper % 16;
        check("hyper[G - 1] on the last bytes of the scale rows", good, total, s2, 0);
        s2.hyper = addr(t.rows) + r * t.row_stride;
        check("hyper on an element row", good, total, s2, 0);
        s2 = sm;
        s2.norm_sq = addr(t.scales) + total * t.scale_stride - 4;
        check("norm_sq on the last bytes of the scale rows", good, total, s2, 0);
        s2 = sm;
        s2.info = block + 4 * blk - 16;
        check("info on the last 16 bytes of a plane block", good, total, s2, 0);
    }
    if (i != j) {   // one bucket's scales on another's exp_avg_sq; its rows on another's scales
        std::vector<AdamwMxRange> bad = good;
        bad[i].scales = at(addr(t.plane[3]) + 4 * r * t.shard_stride);
        check("one bucket's scales on another's exp_avg_sq", bad, total, sm, 0);
        bad = good;
        bad[i].scales = t.scales;
        check("the same scale rows twice", bad, total, sm, 0);
        bad = good;
        bad[i].rows = at(addr(t.scales) + 16 - total * bad[i].row_stride);
        check("rows ending inside another bucket's scales", bad, total, sm, 0);
        bad = good;
        bad[i].plane[k] = t.plane[(k + 1) % 4];
        check("a plane of another bucket", bad, total, sm, layout == FLAT ? -1 : 0);
    }
    {   // inside one bucket
        std::vector<AdamwMxRange> bad = good;
        bad[i].rows = bad[i].scales;
        check("a bucket's rows on its scales", bad, total, sm, 0);
        bad = good;
        bad[i].plane[1] = bad[i].plane[0];
        check("param == grad", bad, total, sm, 0);
        bad = good;
        bad[i].plane[2] = bad[i].rows;
        check("exp_avg on the bucket's rows", bad, total, sm, 0);
    }
    if (layout == WIDE && r + 1 < total) {   // the 256-byte gap behind block r of plane k of bucket j
        const uint64_t gap = block + 4 * blk, next = gap + 4 * kGap;
        Small s2 = sm;
        s2.hyper = gap;
        check("the hyper array at the head of a gap", good, total, s2, 1);
        s2.hyper = next - 32 * G;
        check("the hyper array at the tail of a gap", good, total, s2, 1);
        s2.hyper = next - 32 * G + 16;
        check("the last set on the next block's head", good, total, s2, 0);
        s2.hyper = gap - 16;
        check("the first set on the block's tail", good, total, s2, 0);
        s2 = sm;
        s2.norm_sq = next - 4 * total;
        s2.info = gap;
        check("norm_sq and info in one gap", good, total, s2, 4 * total + 16 <= 4 * kGap ? 1 : 0);
        s2.norm_sq = next - 4 * total + 4;
        check("norm_sq one float into the next block", good, total, s2, 0);
        s2 = sm;
        s2.info = gap - 16;
        check("info on the block's tail", good, total, s2, 0);
    }
}

int main() {
    Rng rng{20261021};
    const uint64_t totals[] = {8, 16, 64};
    for (int rep = 0; rep < 54; ++rep) {
        const uint64_t total = totals[rep % 3];
        const Layout layout = (Layout)((rep / 3) % LAYOUTS);
        const int count = rep < 9 ? 12 : 1 + (int)rng.next(12);
        uint64_t end;
        const std::vector<AdamwMxRange> good = make(rng, count, total, layout, &end);
        const uint64_t far = (end + 4095) / 4096 * 4096 + (1ull << 30);
        const Small sm{far, 1 + rng.next(8), far + 4096, far + 8192};
        check(layout == COMPACT ? "compact" : layout == FLAT ? "flat" : "wide", good, total, sm, 1);
        check("without norm_sq and info", good, total, Small{far, sm.G, 0, 0}, 1);
        Small s2 = sm;
        s2.info = far + 32 * sm.G - 16;
        check("info inside the last set", good, total, s2, 0);
        s2.info = far + 32 * sm.G;
        check("info behind the last set", good, total, s2, 1);
        s2 = sm;
        s2.norm_sq = sm.info - 4 * total + 4;
        check("norm_sq on info", good, total, s2, 0);
        for (int m = 0; m < 4; ++m) mutants(rng, good, total, sm, layout);
        const uint64_t span = end - (1ull << 40);
        for (int m = 0; m < 6; ++m) {
            s2 = sm;
            s2.hyper = (1ull << 40) + 16 * rng.next(span / 16);
            check("the hyper array anywhere", good, total, s2, -1);
            s2 = sm;
            s2.info = (1ull << 40) + 16 * rng.next(span / 16);
            check("info anywhere", good, total, s2, -1);
        }
    }
    expect("an empty list", tsa::adamw_mx_lists_disjoint(nullptr, 0, 8, at(1ull << 44), nullptr, nullptr) &&
                                tsa::adamw_mx_list_verdict(nullptr, 0, 8, at(1ull << 44), nullptr, nullptr) == tsa::kAdamwMxOk);
    {   // count == 0: the small intervals still go against each other
        std::vector<AdamwMxRange> none;
        const uint64_t far = 1ull << 44;
        check("count == 0, apart", none, 8, Small{far, 8, far + 256, far + 512}, 1);
        check("count == 0, info inside the eighth set", none, 8, Small{far, 8, far + 1024, far + 240}, 0);
        check("count == 0, seven sets", none, 8, Small{far, 7, far + 1024, far + 240}, 1);
    }
    // the mapping itself: six ShardRanges per bucket, the halvings and doublings where they belong
    {
        const AdamwMxRange one{at(1ull << 40), 2064, at(1ull << 41), 72, 2048, {at(1ull << 42), at(1ull << 43), at(1ull << 44), at(1ull << 45)}, 260};
        std::vector<tsa::ShardRange> out;
        bool ok = tsa::adamw_mx_as_ranges(&one, 1, &out) && out.size() == 6 && out[0].ranks == one.rows && out[0].stride == 1032 &&
                  out[0].n == 1024 && !out[0].shard && out[1].ranks == one.scales && out[1].stride == 36 && out[1].n == 32 && !out[1].shard;
        for (int k = 0; ok && k < 4; ++k)
            ok = !out[2 + k].ranks && out[2 + k].stride == 0 && out[2 + k].n == 4096 && out[2 + k].shard == one.plane[k] &&
                 out[2 + k].shard_stride == 520;
        expect("the 2-byte view of one bucket", ok);
    }
    // Rows, scales and the three small buffers filling ONE gap exactly: 8 blocks of 256 floats (1024 bytes) at a
    // stride of 256 + 4260 floats; the gap of 17040 bytes behind block 0 of param = 8 rows of 2048 bytes, 8 scale
    // rows of 64, three hyper sets (96), norm_sq (32) and info (16), in that order.  Accepted; every one of the
    // five one quantum off either way: refused.
    {
        const uint64_t total = 8, n = 2048, base = 1ull << 41, gap = base + 1024;
        const uint64_t rows = gap, scales = rows + 16384, hyper = scales + 512, norm_sq = hyper + 96, info = norm_sq + 32;
        auto list = [&](uint64_t r, uint64_t rs, uint64_t s, uint64_t ss) {
            return std::vector<AdamwMxRange>{AdamwMxRange{at(r), rs, at(s), ss, n, {at(base), at(1ull << 42), at(1ull << 43), at(1ull << 44)}, 256 + 4260}};
        };
        expect("the gap is filled exactly", info + 16 == base + 4 * (256 + 4260));
        const Small sm{hyper, 3, norm_sq, info};
        check("everything in one gap", list(rows, n, scales, 64), total, sm, 1);
        check("rows 16 bytes early", list(rows - 16, n, scales, 64), total, sm, 0);
        check("rows 16 bytes wider", list(rows, n + 16, scales, 64), total, sm, 0);
        check("scales 8 bytes early", list(rows, n, scales - 8, 64), total, sm, 0);
        check("scales 8 bytes wider", list(rows, n, scales, 72), total, sm, 0);
        check("hyper 16 bytes early", list(rows, n, scales, 64), total, Small{hyper - 16, 3, norm_sq, info}, 0);
        check("a fourth hyper set", list(rows, n, scales, 64), total, Small{hyper, 4, norm_sq, info}, 0);
        check("norm_sq 4 bytes early", list(rows, n, scales, 64), total, Small{hyper, 3, norm_sq - 4, info}, 0);
        check("norm_sq 4 bytes late", list(rows, n, scales, 64), total, Small{hyper, 3, norm_sq + 4, info}, 0);
        check("info 16 bytes late: on block 1", list(rows, n, scales, 64), total, Small{hyper, 3, norm_sq, info + 16}, 0);
        check("info 16 bytes early: on norm_sq", list(rows, n, scales, 64), total, Small{hyper, 3, norm_sq, info - 16}, 0);
    }
    // the top of the address space
    for (uint64_t total : totals) {
        const uint64_t n = 256 * total, top = (uint64_t)UINTPTR_MAX, far = 1ull << 50;
        const Small sm{far, 2, far + 4096, far + 8192};
        auto one = [&]() { return AdamwMxRange{at(1ull << 40), n, at(1ull << 39), n / 32, n, {at(1ull << 41), at(1ull << 42), at(1ull << 43), at(1ull << 44)}, 320}; };
        for (int64_t d : {-64, -16, 0, 16}) {   // 16: the interval ends past the top (the address itself does not wrap)
            AdamwMxRange m = one();
            m.scales = at(top - 7 - total * (n / 32) + (uint64_t)d);
            check("scales at the top", {m}, total, sm, d <= 0 ? 1 : 0);
            m = one();
            m.rows = at(top - 15 - total * n + (uint64_t)d);
            check("rows at the top", {m}, total, sm, d <= 0 ? 1 : 0);
            m = one();
            m.plane[3] = at(top - 15 - 4 * ((total - 1) * 320 + 256) + (uint64_t)d);
            check("exp_avg_sq at the top", {m}, total, sm, d <= 0 ? 1 : 0);
            Small s2 = sm;
            s2.hyper = top - 15 - 64 + (uint64_t)d;
            check("the hyper array at the top", {one()}, total, s2, d <= 0 ? 1 : 0);
            s2 = sm;
            s2.info = top - 15 - 16 + (uint64_t)d;
            check("info at the top", {one()}, total, s2, d <= 0 ? 1 : 0);
        }
        // products past 2^64: refused, not wrapped into a small range
        AdamwMxRange w = one();
        w.shard_stride = 1ull << 63;
        check("2 shard_stride wraps", {w}, total, sm, 0);
        w.shard_stride = (1ull << 62) / total * 2;
        check("4 total shard_stride wraps", {w}, total, sm, 0);
        w = one();
        w.row_stride = (1ull << 63) / total * 2 + 16;
        check("total row_stride wraps", {w}, total, sm, 0);
        w = one();
        w.scale_stride = (1ull << 63) / total * 2 + 8;
        check("total scale_stride wraps", {w}, total, sm, 0);
        w = one();
        w.n = 1ull << 63;
        w.row_stride = w.n;
        w.scale_stride = w.n / 32;
        w.shard_stride = w.n / total;
        check("2 n wraps", {w}, total, sm, 0, false);
        verdict("n past the tile cap", {w}, total, sm, tsa::kAdamwMxArg);
    }
    // every argument rule that needs no plan
    {
        const uint64_t total = 8, n = 2048, far = 1ull << 50;
        const Small sm{far, 3, far + 4096, far + 8192};
        const AdamwMxRange ok{at(1ull << 40), n, at(1ull << 39), n / 32, n, {at(1ull << 41), at(1ull << 42), at(1ull << 43), at(1ull << 44)}, 256};
        auto with = [&](auto&& change) {
            AdamwMxRange m = ok;
            change(m);
            return std::vector<AdamwMxRange>{m};
        };
        typedef AdamwMxRange R;
        verdict("the plain bucket", with([](R&) {}), total, sm, tsa::kAdamwMxOk);
        verdict("rows NULL", with([](R& m) { m.rows = nullptr; }), total, sm, tsa::kAdamwMxArg);
        verdict("scales NULL", with([](R& m) { m.scales = nullptr; }), total, sm, tsa::kAdamwMxArg);
        verdict("rows 8-byte aligned only", with([](R& m) { m.rows = at((1ull << 40) + 8); }), total, sm, tsa::kAdamwMxArg);
        verdict("scales 4-byte aligned only", with([](R& m) { m.scales = at((1ull << 39) + 4); }), total, sm, tsa::kAdamwMxArg);
        verdict("scales 8-byte aligned", with([](R& m) { m.scales = at((1ull << 39) + 8); }), total, sm, tsa::kAdamwMxOk);
        for (int k = 0; k < 4; ++k) {
            verdict("a plane NULL", with([k](R& m) { m.plane[k] = nullptr; }), total, sm, tsa::kAdamwMxArg);
            verdict("a plane 8-byte aligned only", with([k](R& m) { m.plane[k] = at(addr(m.plane[k]) + 8); }), total, sm, tsa::kAdamwMxArg);
        }
        verdict("n == 0", with([](R& m) { m.n = 0; }), total, sm, tsa::kAdamwMxArg);
        verdict("n % (8 total) != 0", with([](R& m) { m.n = 2048 + 32; m.row_stride = 4096; m.scale_stride = 128; m.shard_stride = 512; }), total, sm, tsa::kAdamwMxArg);
        verdict("row_stride < n", with([](R& m) { m.row_stride = 2048 - 16; }), total, sm, tsa::kAdamwMxArg);
        verdict("row_stride % 16 != 0", with([](R& m) { m.row_stride = 2048 + 8; }), total, sm, tsa::kAdamwMxArg);
        verdict("row_stride wide", with([](R& m) { m.row_stride = 2048 + 16; }), total, sm, tsa::kAdamwMxOk);
        verdict("scale_stride < n / 32", with([](R& m) { m.scale_stride = 56; }), total, sm, tsa::kAdamwMxArg);
        verdict("scale_stride % 8 != 0", with([](R& m) { m.scale_stride = 68; }), total, sm, tsa::kAdamwMxArg);
        verdict("scale_stride wide", with([](R& m) { m.scale_stride = 72; }), total, sm, tsa::kAdamwMxOk);
        verdict("shard_stride < blk", with([](R& m) { m.shard_stride = 252; }), total, sm, tsa::kAdamwMxArg);
        verdict("shard_stride % 4 != 0", with([](R& m) { m.shard_stride = 258; }), total, sm, tsa::kAdamwMxArg);
        verdict("not whole tiles", with([](R& m) { m.n = 1024; }), total, sm, tsa::kAdamwMxUnsupported);
        verdict("total < 8", with([](R& m) { m.n = 1024; m.shard_stride = 256; }), 4, sm, tsa::kAdamwMxUnsupported);
        verdict("an empty list", {}, total, sm, tsa::kAdamwMxOk);
        expect("count < 0, a NULL list or total == 0",
               tsa::adamw_mx_list_verdict(&ok, -1, total, at(far), nullptr, nullptr) == tsa::kAdamwMxArg &&
                   tsa::adamw_mx_list_verdict(nullptr, 1, total, at(far), nullptr, nullptr) == tsa::kAdamwMxArg &&
                   tsa::adamw_mx_list_verdict(&ok, 1, 0, at(far), nullptr, nullptr) == tsa::kAdamwMxArg);
        // an ARG fault wins over the shape: a bucket that is not whole tiles AND overlaps
        verdict("not whole tiles and rows on scales", with([](R& m) { m.n = 1024; m.scales = m.rows; }), total, sm, tsa::kAdamwMxArg);
        verdict("not whole tiles and info on a plane", with([](R& m) { m.n = 1024; }), total, Small{far, 3, far + 4096, 1ull << 43}, tsa::kAdamwMxArg);
        // the tile cap: two buckets of 2^30 tiles fit, a third tile more does not (addresses far apart; nothing is touched)
        const uint64_t big = 256ull << 30;
        auto bigone = [&](uint64_t hi, uint64_t n2) {
            return AdamwMxRange{at(hi << 50), n2, at((hi << 50) + (1ull << 49)), big / 32, n2,
                                {at((hi + 1) << 50), at((hi + 2) << 50), at((hi + 3) << 50), at((hi + 4) << 50)}, big / 8};
        };
        std::vector<AdamwMxRange> cap = {bigone(1, big), bigone(8, big - 2048)};
        const Small top{1ull << 62, 3, (1ull << 62) + 4096, (1ull << 62) + 8192};
        verdict("2^31 - 8 tiles", cap, total, top, tsa::kAdamwMxOk);
        AdamwMxRange third = ok;
        cap.push_back(third);
        verdict("2^31 tiles", cap, total, top, tsa::kAdamwMxArg);
        // flags and the three pointers
        using tsa::adamw_mx_pointers_ok;
        const void *h = at(far), *q = at(far + 4096), *f = at(far + 8192);
        expect("the four flag pairs", adamw_mx_pointers_ok(h, q, f, 0, false) && adamw_mx_pointers_ok(h, q, f, 1, false) &&
                                          adamw_mx_pointers_ok(h, q, f, 2, false) && adamw_mx_pointers_ok(h, q, f, 3, false));
        expect("an unknown flag bit", !adamw_mx_pointers_ok(h, q, f, 4, false) && !adamw_mx_pointers_ok(h, q, f, 7, false) &&
                                          !adamw_mx_pointers_ok(h, q, f, -2, false) && !adamw_mx_pointers_ok(h, q, f, 0x100, false) &&
                                          !adamw_mx_pointers_ok(nullptr, nullptr, nullptr, 4, true));
        expect("hyper NULL", !adamw_mx_pointers_ok(nullptr, q, f, 0, false) && adamw_mx_pointers_ok(nullptr, nullptr, nullptr, 0, true));
        expect("norm_sq and info NULL", adamw_mx_pointers_ok(h, nullptr, nullptr, 3, false));
        expect("hyper 8-byte aligned only", !adamw_mx_pointers_ok(at(far + 8), q, f, 0, false));
        expect("norm_sq 2-byte aligned only", !adamw_mx_pointers_ok(h, at(far + 4098), f, 0, false));
        expect("info 8-byte aligned only", !adamw_mx_pointers_ok(h, q, at(far + 8200), 0, false));
    }
    if (g_accepted < 400 || g_refused < 1500) {
        std::printf("MISMATCH the lists do not reach both verdicts: %llu accepted, %llu refused\n", g_accepted, g_refused);
        return 1;
    }
    std::printf("adamw_mx_ranges ok: %llu checks, %llu accepted, %llu refused\n", g_checks, g_accepted, g_refused);
    return 0;
}
"""


LAYOUT = r"""
#include <cstddef>
#include <cstdio>
#include "allred.h"
int main() {
    typedef allred_adamw_mx_bucket_f32 B;
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(B), offsetof(B, rows), offsetof(B, row_stride),
                offsetof(B, scales), offsetof(B, scale_stride), offsetof(B, elems_per_rank), offsetof(B, param), offsetof(B, grad),
                offsetof(B, exp_avg), offsetof(B, exp_avg_sq), offsetof(B, shard_stride),
                ALLRED_ADAMW_MX_GROUP_MAX, ALLRED_ADAMW_MX_RCEIL, ALLRED_ADAMW_ZERO_GRAD);
    return 0;
}
"""


def test_bucket_binding_matches_the_header(tmp_path):
    """_lib.AdamwMxBucketF32 mirrors allred_adamw_mx_bucket_f32 (80 bytes), and the constants agree."""
    import ctypes as C

    from tenstorrentallreduce_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    b = _lib.AdamwMxBucketF32
    assert out[0] == 80
    assert out == [C.sizeof(b), b.rows.offset, b.row_stride.offset, b.scales.offset, b.scale_stride.offset, b.elems_per_rank.offset,
                   b.param.offset, b.grad.offset, b.exp_avg.offset, b.exp_avg_sq.offset, b.shard_stride.offset,
                   _lib.ADAMW_MX_GROUP_MAX, _lib.ADAMW_MX_RCEIL, _lib.ADAMW_ZERO_GRAD]


def test_entry_points_refuse_before_any_hip_call():
    """no GPU here: a call that got as far as HIP would not return ALLRED_ERR_ARG"""
    import ctypes as C

    from tenstorrentallreduce_amd import _lib
    lib = _lib.lib
    arr = (_lib.AdamwMxBucketF32 * 1)((1 << 40, 2048, 1 << 39, 64, 2048, 1 << 41, 1 << 42, 1 << 43, 3 << 42, 256))
    call = lib.allred_plan_adamw_all_gather_shards_mxfp8
    g0, g1 = (C.c_uint8 * 1)(0), (C.c_uint8 * 1)(1)
    hy = 1 << 44
    assert call(None, arr, g0, 1, hy, 1, None, None, 0, None) == _lib.ERR_ARG      # no plan
    assert call(None, arr, g0, 1, hy, 1, None, None, 4, None) == _lib.ERR_ARG      # an unknown flag bit
    assert call(None, arr, None, 1, hy, 0, None, None, 0, None) == _lib.ERR_ARG    # ngroups 0
    assert call(None, arr, None, 1, hy, 9, None, None, 0, None) == _lib.ERR_ARG    # ngroups 9
    assert call(None, arr, g1, 1, hy, 1, None, None, 3, None) == _lib.ERR_ARG      # a group index equal to ngroups
    assert call(None, None, None, 0, hy + 8, 1, None, None, 0, None) == _lib.ERR_ARG   # hyper misaligned
    assert call(None, None, None, 0, None, 1, None, None, 0, None) == _lib.ERR_ARG     # hyper NULL
    assert lib.allred_plan_adamw_shards_mxfp8_launches(None, arr, 1) == _lib.ERR_ARG


def test_adamw_mx_rules_match_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the adamw_mx_ranges check"
    src = tmp_path / "adamw_mx_ranges_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "adamw_mx_ranges_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "adamw_mx_ranges ok" in run.stdout
