"""csrc/mx2d_ranges.hpp against brute force, on the CPU.

A stand-alone C++ program (its own main) is compiled with g++ under AddressSanitizer and UBSan and run
directly, as tests/test_adamw_mx_ranges.py does.  For every list it compares mx2d_lists_disjoint — the
disjointness rule of allred_plan_all_gather_shards_mxfp8_2d — with the rule written out in unsigned 128-bit
arithmetic: per bucket up to four output intervals [p, p + total stride) — element rows and scale rows (when
given), t element rows, t scale rows — and the shard's `total` SEPARATE block intervals; a list is accepted
when every interval ends at or below UINTPTR_MAX and no two of them (every pair is tested) share a byte.

Lists: random ones of 1 .. 21 buckets at 8 / 16 / 64 ranks, every third bucket without row-wise outputs, the
addresses made up (nothing is dereferenced), the shards compact, flat or wide with all of a bucket's outputs
filling the gap behind its block 0 exactly: accepted.  Mutants: every output moved onto the last byte of every
other kind of interval, of its own and of another bucket; gap fillers one byte quantum off either way: refused.
Then every argument rule of mx2d_list_verdict."""
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

#include "mx2d_ranges.hpp"

typedef unsigned __int128 u128;
using tsa::Mx2dRange;

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

// the four outputs of a bucket as (pointer, stride) pairs: 0 rows, 1 scales, 2 t rows, 3 t scales
static const void*& out_ptr(Mx2dRange& s, int k) { return k == 0 ? s.rows : k == 1 ? s.scales : k == 2 ? s.t_rows : s.t_scales; }
static uint64_t out_stride(const Mx2dRange& s, int k) {
    return k == 0 ? s.row_stride : k == 1 ? s.scale_stride : k == 2 ? s.t_row_stride : s.t_scale_stride;
}

static bool brute(const std::vector<Mx2dRange>& list, uint64_t total) {
    struct I { u128 lo, hi; };
    std::vector<I> v;
    for (Mx2dRange s : list) {
        for (int k = s.rows ? 0 : 2; k < 4; ++k)
            v.push_back(I{(u128)addr(out_ptr(s, k)), (u128)addr(out_ptr(s, k)) + (u128)total * out_stride(s, k)});
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

static void dump(const std::vector<Mx2dRange>& list) {
    for (Mx2dRange s : list) {
        for (int k = 0; k < 4; ++k) std::printf("  out%d=%llx/%llu", k, (unsigned long long)addr(out_ptr(s, k)), (unsigned long long)out_stride(s, k));
        std::printf(" n=%llu cols=%llu shard=%llx/%llu\n", (unsigned long long)s.n, (unsigned long long)s.cols,
                    (unsigned long long)addr(s.shard), (unsigned long long)s.shard_stride);
    }
}

// want: 1 must be accepted, 0 must be refused
static void check(const char* what, const std::vector<Mx2dRange>& list, uint64_t total, int want) {
    const bool got = tsa::mx2d_lists_disjoint(list.data(), (int)list.size(), total);
    const bool ref = brute(list, total);
    ++g_lists;
    ++(ref ? g_accepted : g_refused);
    if (got != ref || ref != (want == 1)) {
        std::printf("MISMATCH %s: count=%zu total=%llu got=%d brute=%d want=%d\n", what, list.size(), (unsigned long long)total,
                    (int)got, (int)ref, want);
        dump(list);
        std::exit(1);
    }
}

static void verdict(const char* what, const std::vector<Mx2dRange>& list, uint64_t total, tsa::Mx2dVerdict want) {
    const tsa::Mx2dVerdict got = tsa::mx2d_list_verdict(list.data(), (int)list.size(), total);
    ++g_lists;
    ++(got == tsa::kMx2dOk ? g_accepted : g_refused);
    if (got != want) {
        std::printf("MISMATCH verdict %s: got=%d want=%d\n", what, (int)got, (int)want);
        dump(list);
        std::exit(1);
    }
}

enum Layout { COMPACT, FLAT, WIDE, LAYOUTS };

// an accepted list.  COMPACT / FLAT: outputs in buffers of their own, some strides skewed.  WIDE: all of a
// bucket's outputs, unskewed, one behind the other, fill the gap behind its shard's block 0 EXACTLY.
static std::vector<Mx2dRange> make(Rng& rng, int count, uint64_t total, Layout layout) {
    std::vector<Mx2dRange> list((size_t)count);
    uint64_t cursor = (1ull << 40) + 16 * rng.next(1000);
    for (int i = 0; i < count; ++i) {
        Mx2dRange& s = list[(size_t)i];
        s.cols = 32 * (1 + rng.next(5));
        s.n = s.cols * 32 * total * (1 + rng.next(3));
        const bool rows = i % 3 != 2;
        const bool skew = layout != WIDE;
        s.row_stride = rows ? s.n + (skew && i % 2 ? 16 * (1 + rng.next(4)) : 0) : 0;
        s.scale_stride = rows ? s.n / 32 + (skew && i % 3 == 1 ? 8 * (1 + rng.next(4)) : 0) : 0;
        s.t_row_stride = s.n + (skew && i % 2 == 0 ? 16 * (1 + rng.next(4)) : 0);
        s.t_scale_stride = s.n / 32 + (skew && i % 4 == 1 ? 8 * (1 + rng.next(4)) : 0);
        if (layout == WIDE) {
            const uint64_t blk = s.n / total;
            uint64_t inner = 0;
            for (int k = rows ? 0 : 2; k < 4; ++k) inner += total * out_stride(s, k);   // a multiple of 8 total >= 64
            s.shard = at(cursor);
            s.shard_stride = blk + inner / 4;
            uint64_t p = cursor + 4 * blk;
            const int order[4] = {0, 2, 1, 3};   // the 16-byte aligned ones first
            for (int k : order) {
                if (!rows && k < 2) continue;
                out_ptr(s, k) = at(p);
                p += total * out_stride(s, k);
            }
            cursor += 4 * total * s.shard_stride + 16 * rng.next(4);
        } else {
            for (int k = rows ? 0 : 2; k < 4; ++k) {
                out_ptr(s, k) = at(cursor);
                cursor += total * out_stride(s, k);
                cursor = (cursor + 15) / 16 * 16 + 16 * rng.next(8);
            }
        }
    }
    if (layout == COMPACT) {
        for (Mx2dRange& s : list) {
            s.shard = at(cursor);
            s.shard_stride = s.n / total;
            cursor += 4 * s.n + 16 * rng.next(4);
        }
    } else if (layout == FLAT) {
        uint64_t F = 0, off = 0;
        for (const Mx2dRange& s : list) F += s.n / total;
        F += 4 * rng.next(3);
        for (Mx2dRange& s : list) {
            s.shard = at(cursor + 4 * off);
            s.shard_stride = F;
            off += s.n / total;
        }
    }
    return list;
}

static void mutants(Rng& rng, const std::vector<Mx2dRange>& good, uint64_t total) {
    const size_t i = rng.next(good.size()), j = rng.next(good.size());
    Mx2dRange t = good[j];
    const uint64_t r = rng.next(total);
    for (int a = good[i].rows ? 0 : 2; a < 4; ++a) {
        for (int b = t.rows ? 0 : 2; b < 4; ++b) {
            if (i == j && a == b) continue;
            std::vector<Mx2dRange> bad = good;   // output a of bucket i BEGINS on the last byte of output b of bucket j
            out_ptr(bad[i], a) = at(addr(out_ptr(t, b)) + total * out_stride(t, b) - 1);
            check("an output on the last byte of another", bad, total, 0);
            bad = good;                          // ... ENDS on its first byte
            out_ptr(bad[i], a) = at(addr(out_ptr(t, b)) + 1 - total * out_stride(bad[i], a));
            check("an output ending on the first byte of another", bad, total, 0);
        }
        std::vector<Mx2dRange> bad = good;       // on the last byte of a shard block
        out_ptr(bad[i], a) = at(addr(t.shard) + 4 * (r * t.shard_stride + t.n / total) - 1);
        check("an output on the last byte of a shard block", bad, total, 0);
        bad = good;                              // a shard block on the last byte of the output
        bad[j].shard = at(addr(out_ptr(bad[i], a)) + total * out_stride(bad[i], a) - 1 - 4 * r * bad[j].shard_stride);
        check("a shard block on the last byte of an output", bad, total, 0);
    }
    if (i != j) {
        std::vector<Mx2dRange> bad = good;
        bad[i].shard = t.shard;
        check("one shard twice", bad, total, 0);
    }
}

int main() {
    Rng rng{20261021};
    const uint64_t totals[] = {8, 16, 64};
    for (int rep = 0; rep < 90; ++rep) {
        const uint64_t total = totals[rep % 3];
        const Layout layout = (Layout)((rep / 3) % LAYOUTS);
        const int count = rep < 9 ? 21 : 1 + (int)rng.next(21);
        const std::vector<Mx2dRange> good = make(rng, count, total, layout);
        check(layout == COMPACT ? "compact" : layout == FLAT ? "flat" : "wide: the outputs fill the gap exactly", good, total, 1);
        verdict("a good list", good, total, tsa::kMx2dOk);
        for (int m = 0; m < 3; ++m) mutants(rng, good, total);
        if (layout == WIDE) {   // one byte quantum off either way: on block 0's tail, or on block 1's head
            const size_t i = rng.next(good.size());
            std::vector<Mx2dRange> bad = good;
            const int first = bad[i].rows ? 0 : 2;
            out_ptr(bad[i], first) = at(addr(out_ptr(bad[i], first)) - 16);
            check("gap filler 16 bytes early", bad, total, 0);
            verdict("gap filler 16 bytes early", bad, total, tsa::kMx2dArg);
            bad = good;
            bad[i].t_scales = at(addr(bad[i].t_scales) + 8);
            check("gap filler 8 bytes late", bad, total, 0);
            verdict("gap filler 8 bytes late", bad, total, tsa::kMx2dArg);
        }
    }
    if (!tsa::mx2d_lists_disjoint(nullptr, 0, 8) || tsa::mx2d_list_verdict(nullptr, 0, 8) != tsa::kMx2dOk ||
        tsa::mx2d_list_verdict(nullptr, -1, 8) != tsa::kMx2dArg || tsa::mx2d_list_verdict(nullptr, 1, 8) != tsa::kMx2dArg) {
        std::printf("MISMATCH the empty / missing list\n");
        return 1;
    }
    // the mapping: five ShardRanges with rows, three without
    {
        const Mx2dRange one{at(1ull << 40), 8208, at(1ull << 41), 264, at(1ull << 42), 8192, at(1ull << 43), 256, 8192, 32, at(1ull << 44), 1028};
        std::vector<tsa::ShardRange> out;
        if (!tsa::mx2d_as_ranges(&one, 1, &out) || out.size() != 5 || out[0].ranks != one.rows || out[0].stride != 4104 || out[1].stride != 132 ||
            out[2].ranks != one.t_rows || out[2].stride != 4096 || out[3].ranks != one.t_scales || out[3].stride != 128 || out[4].ranks ||
            out[4].n != 16384 || out[4].shard != one.shard || out[4].shard_stride != 2056) {
            std::printf("MISMATCH the 2-byte view of one bucket\n");
            return 1;
        }
        Mx2dRange two = one;
        two.rows = two.scales = nullptr;
        out.clear();
        if (!tsa::mx2d_as_ranges(&two, 1, &out) || out.size() != 3 || out[0].ranks != one.t_rows) {
            std::printf("MISMATCH the 2-byte view without rows\n");
            return 1;
        }
    }
    // the argument rules, one at a time on a good bucket: total 8, cols 96, nrows 512
    {
        const uint64_t total = 8, n = 96 * 512;
        const Mx2dRange g{at(1ull << 40), n + 16, at(1ull << 41), n / 32 + 8, at(1ull << 42), n, at(1ull << 43), n / 32, n, 96, at(1ull << 44), n / total + 4};
        verdict("good", {g}, total, tsa::kMx2dOk);
        Mx2dRange c = g;
        c.rows = c.scales = nullptr;
        verdict("column-wise only", {c}, total, tsa::kMx2dOk);
        c.row_stride = c.scale_stride = 3;   // not looked at without rows
        verdict("column-wise only, strides ignored", {c}, total, tsa::kMx2dOk);
#define ARG(what, stmt) { Mx2dRange b = g; stmt; verdict(what, {g0, b}, total, tsa::kMx2dArg); verdict(what, {b, g0}, total, tsa::kMx2dArg); }
#define UNS(what, stmt) { Mx2dRange b = g; stmt; verdict(what, {g0, b}, total, tsa::kMx2dUnsupported); verdict(what, {b, g0}, total, tsa::kMx2dUnsupported); }
        const Mx2dRange g0{at(1ull << 50), n, at(1ull << 51), n / 32, at(1ull << 52), n, at(1ull << 53), n / 32, n, 96, at(1ull << 54), n / total};
        ARG("rows without scales", b.scales = nullptr)
        ARG("scales without rows", b.rows = nullptr)
        ARG("no t rows", b.t_rows = nullptr)
        ARG("no t scales", b.t_scales = nullptr)
        ARG("no shard", b.shard = nullptr)
        ARG("rows 8-byte aligned", b.rows = at(addr(b.rows) + 8))
        ARG("scales 4-byte aligned", b.scales = at(addr(b.scales) + 4))
        ARG("t rows 8-byte aligned", b.t_rows = at(addr(b.t_rows) + 8))
        ARG("t scales 4-byte aligned", b.t_scales = at(addr(b.t_scales) + 4))
        ARG("shard 8-byte aligned", b.shard = at(addr(b.shard) + 8))
        ARG("n == 0", b.n = 0)
        ARG("n % (8 total)", b.n = n + 8)
        ARG("cols == 0", b.cols = 0)
        ARG("n % cols", b.cols = 7 * 32 * 5)
        ARG("row_stride < n", b.row_stride = n - 16)
        ARG("row_stride % 16", b.row_stride = n + 8)
        ARG("scale_stride < n / 32", b.scale_stride = n / 32 - 8)
        ARG("scale_stride % 8", b.scale_stride = n / 32 + 4)
        ARG("t_row_stride < n", b.t_row_stride = n - 16)
        ARG("t_row_stride % 16", b.t_row_stride = n + 8)
        ARG("t_scale_stride < n / 32", b.t_scale_stride = n / 32 - 8)
        ARG("t_scale_stride % 8", b.t_scale_stride = n / 32 + 4)
        ARG("shard_stride < blk", b.shard_stride = n / total - 4)
        ARG("shard_stride % 4", b.shard_stride = n / total + 2)
        ARG("shard_stride doubling overflows", b.shard_stride = 1ull << 63)
        ARG("total * t_row_stride overflows", b.t_row_stride = 1ull << 62)
        ARG("an output at the top of the address space", b.t_scales = at(UINT64_MAX - 7))
        ARG("t rows on rows", b.t_rows = b.rows)
        UNS("cols % 32", b.cols = 48)
        UNS("nrows % (32 total)", b.n = 96 * 128)
        UNS("R % 32", b.n = 96 * 384)
        // an argument error wins over an unsupported shape, wherever either stands
        { Mx2dRange b = g, u = g0; u.cols = 48; b.t_rows = nullptr; verdict("arg before unsupported", {u, b}, total, tsa::kMx2dArg); }
        { Mx2dRange b = g0; b.shard_stride = n / 4; verdict("total < 8", {b}, 4, tsa::kMx2dUnsupported); }
        // the cap on the work items: 2^31 - 1 squares of 1024 elements over the list
        { Mx2dRange b = g0; b.cols = 32; b.n = 1024ull * 0x7fffffffull / 8 * 8; b.row_stride = b.t_row_stride = b.n; b.scale_stride = b.t_scale_stride = b.n / 32; b.shard_stride = b.n / total;
          b.rows = at(1ull << 60); b.scales = at(1ull << 59); b.t_rows = at(3ull << 59); b.t_scales = at(5ull << 58); b.shard = at(7ull << 57);
          if (tsa::mx2d_list_verdict(&b, 1, total) == tsa::kMx2dArg) { std::printf("MISMATCH cap: a list below the cap refused as an argument error\n"); return 1; }
          verdict("one square over the cap", {b, g}, total, tsa::kMx2dArg); }
    }
    std::printf("mx2d_ranges ok: %llu lists, %llu accepted, %llu refused\n", g_lists, g_accepted, g_refused);
    return 0;
}
"""


def test_mx2d_ranges_match_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the mx2d_ranges check"
    src = tmp_path / "mx2d_ranges_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "mx2d_ranges_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mx2d_ranges ok" in run.stdout
