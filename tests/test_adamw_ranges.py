"""csrc/adamw_ranges.hpp against brute force, on the CPU, in the style of
tests/test_shard_f32_norm_ranges.py: a stand-alone C++ program (its own main) compiled with g++
under AddressSanitizer and UBSan and run directly; nothing is loaded into Python.

adamw_lists_disjoint is the disjointness rule of allred_plan_adamw_all_gather_shards_f32: every
bucket's rank-row interval, the 4 P count plane blocks of blk floats, [hyper, + 32),
[norm_sq, + 4 P) and [info, + 16) pairwise disjoint, byte-exact.  The brute force writes that out
in unsigned 128-bit arithmetic, every pair of intervals compared.

Accepted: compact, wide and flat lists (four rank-major flat buffers, one per plane) of 1 .. 32
buckets at 8 / 16 / 64 ranks (the brute force is quadratic, so most lists are short); hyper,
norm_sq or info in the gap of a wide stride.  Refused: a plane block's first byte on another plane's last byte; the same plane named twice; param == grad; info on
a row; hyper inside a plane block; overflow at the top of the address space.  Random placements
all over a list's span: whatever brute force says.

adamw_pointers_ok / adamw_list_verdict are the argument rules of the call that need no plan
(engine.cpp adamw_check applies them before any HIP call); the program holds every one of them.
A plan cannot be made without a device, so through the entry points themselves only the NULL-plan
refusal is reachable here; tests/test_gpu_adamw_shards.py holds every refusal on a real plan.
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

#include "adamw_ranges.hpp"

typedef unsigned __int128 u128;
using tsa::AdamwRange;

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

// the rule, written out: every interval against every other
static bool brute(const std::vector<AdamwRange>& list, uint64_t total, uint64_t hyper, uint64_t norm_sq, uint64_t info) {
    std::vector<I> v;
    if (hyper) v.push_back(I{(u128)hyper, (u128)hyper + 32});
    if (norm_sq) v.push_back(I{(u128)norm_sq, (u128)norm_sq + (u128)4 * total});
    if (info) v.push_back(I{(u128)info, (u128)info + 16});
    for (const AdamwRange& s : list) {
        v.push_back(I{(u128)addr(s.ranks), (u128)addr(s.ranks) + (u128)2 * total * s.stride});
        if (total > 1 && s.shard_stride < s.n / total) return false;
        for (int k = 0; k < 4; ++k)
            for (uint64_t b = 0; b < total; ++b) {
                const u128 lo = (u128)addr(s.plane[k]) + (u128)4 * b * s.shard_stride;
                v.push_back(I{lo, lo + (u128)4 * (s.n / total)});
            }
    }
    for (const I& i : v)
        if (i.hi > (u128)UINTPTR_MAX) return false;
    for (size_t i = 0; i < v.size(); ++i)
        for (size_t j = i + 1; j < v.size(); ++j)
            if (v[i].hi > v[i].lo && v[j].hi > v[j].lo && v[i].lo < v[j].hi && v[j].lo < v[i].hi) return false;
    return true;
}

// want: 1 must be accepted, 0 must be refused, -1 whatever brute force says
static void check(const char* what, const std::vector<AdamwRange>& list, uint64_t total, uint64_t hyper, uint64_t norm_sq,
                  uint64_t info, int want) {
    const bool got = tsa::adamw_lists_disjoint(list.data(), (int)list.size(), total, at(hyper), at(norm_sq), at(info));
    const bool ref = brute(list, total, hyper, norm_sq, info);
    ++g_checks;
    ++(ref ? g_accepted : g_refused);
    if (got != ref || (want >= 0 && ref != (want == 1))) {
        std::printf("MISMATCH %s: count=%zu total=%llu hyper=%llx norm_sq=%llx info=%llx got=%d brute=%d want=%d\n", what,
                    list.size(), (unsigned long long)total, (unsigned long long)hyper, (unsigned long long)norm_sq,
                    (unsigned long long)info, (int)got, (int)ref, want);
        for (const AdamwRange& s : list)
            std::printf("  ranks=%llx stride=%llu n=%llu planes=%llx %llx %llx %llx shard_stride=%llu\n",
                        (unsigned long long)addr(s.ranks), (unsigned long long)s.stride, (unsigned long long)s.n,
                        (unsigned long long)addr(s.plane[0]), (unsigned long long)addr(s.plane[1]),
                        (unsigned long long)addr(s.plane[2]), (unsigned long long)addr(s.plane[3]),
                        (unsigned long long)s.shard_stride);
        std::exit(1);
    }
}

enum Layout { COMPACT, FLAT, WIDE, LAYOUTS };

// an accepted list of whole-tile buckets: rank rows in buffers of their own (every other one with a
// stride skew), the four planes in `layout`; *end: the first byte behind everything
static std::vector<AdamwRange> make(Rng& rng, int count, uint64_t total, Layout layout, uint64_t* end) {
    std::vector<AdamwRange> list((size_t)count);
    uint64_t cursor = (1ull << 40) + 16 * rng.next(1000);
    for (int i = 0; i < count; ++i) {
        AdamwRange& s = list[(size_t)i];
        s.n = 256 * total * (1 + rng.next(5));
        s.stride = s.n + (i % 2 ? 64 : 0);
        s.ranks = at(cursor);
        cursor += 2 * total * s.stride + 16 * rng.next(8);
    }
    if (layout == FLAT) {   // four rank-major flat buffers of F floats per rank, one per plane
        uint64_t F = 0;
        for (int i = 0; i < count; ++i) F += list[(size_t)i].n / total;
        for (int k = 0; k < 4; ++k) {
            uint64_t off = 0;
            for (int i = 0; i < count; ++i) {
                list[(size_t)i].plane[k] = at(cursor + 4 * off);
                list[(size_t)i].shard_stride = F;
                off += list[(size_t)i].n / total;
            }
            cursor += 4 * total * F + 16 * rng.next(4);
        }
    } else {
        for (int i = 0; i < count; ++i) {
            AdamwRange& s = list[(size_t)i];
            s.shard_stride = s.n / total + (layout == WIDE ? 64 : 0);   // WIDE: a gap of 256 bytes behind every block
            for (int k = 0; k < 4; ++k) {
                s.plane[k] = at(cursor);
                cursor += 4 * total * s.shard_stride + 16 * rng.next(4);
            }
        }
    }
    *end = cursor;
    return list;
}

static void expect(const char* what, bool ok) {
    ++g_checks;
    if (!ok) {
        std::printf("MISMATCH %s\n", what);
        std::exit(1);
    }
}

static void mutants(Rng& rng, const std::vector<AdamwRange>& good, uint64_t total, uint64_t far, Layout layout) {
    const uint64_t hyper = far, norm_sq = far + 4096, info = far + 8192;
    check("the list with the three far away", good, total, hyper, norm_sq, info, 1);
    check("without norm_sq and info", good, total, hyper, 0, 0, 1);
    const size_t i = rng.next(good.size()), j = rng.next(good.size());
    const AdamwRange& t = good[i];
    const uint64_t b = rng.next(total), blk = t.n / total;
    const int k = (int)rng.next(4), k2 = (k + 1 + (int)rng.next(3)) % 4;
    // a plane block's first byte on another plane's last byte (of any bucket)
    {
        std::vector<AdamwRange> bad = good;
        const AdamwRange& o = good[j];
        const uint64_t last = addr(o.plane[k2]) + 4 * (rng.next(total) * o.shard_stride + o.n / total) - 1;
        // block b of plane k starts at `last` rounded down to 16 bytes: it covers that byte
        bad[i].plane[k] = at((last & ~15ull) - 4 * b * t.shard_stride);
        check("a plane block on another plane's last byte", bad, total, hyper, norm_sq, info, 0);
    }
    {
        std::vector<AdamwRange> bad = good;
        bad[i].plane[k] = bad[i].plane[k2];
        check("the same plane named twice", bad, total, hyper, norm_sq, info, 0);
        bad = good;
        bad[i].plane[1] = bad[i].plane[0];
        check("param == grad", bad, total, hyper, norm_sq, info, 0);
        if (good.size() > 1 && i != j) {
            bad = good;
            bad[i].plane[k] = good[j].plane[k];
            check("another bucket's plane", bad, total, hyper, norm_sq, info, layout == FLAT && good[i].n != 0 ? -1 : 0);
        }
    }
    // info on a row: its data, its last byte, the skew
    const uint64_t r = rng.next(total);
    check("info on a row", good, total, hyper, norm_sq, addr(t.ranks) + 2 * r * t.stride + 16 * rng.next(t.n / 8), 0);
    check("info on the last 16 bytes of a row's data", good, total, hyper, norm_sq, addr(t.ranks) + 2 * (r * t.stride + t.n) - 16, 0);
    if (t.stride > t.n) check("info in a row's skew", good, total, hyper, norm_sq, addr(t.ranks) + 2 * (r * t.stride + t.n), 0);
    // hyper / norm_sq inside a plane block, at its head and on its tail
    const uint64_t block = addr(t.plane[k]) + 4 * b * t.shard_stride;
    check("hyper inside a plane block", good, total, block + 16 * rng.next(blk / 4 - 1), norm_sq, info, 0);
    check("hyper on the last 16 bytes of a plane block", good, total, block + 4 * blk - 16, norm_sq, info, 0);
    check("hyper ending on a plane block's first 16 bytes", good, total, block - 16, norm_sq, info,
          layout == WIDE && b > 0 ? 0 : -1);
    check("norm_sq on the last float of a plane block", good, total, hyper, block + 4 * blk - 4, info, 0);
    // in the gap of a wide stride (256 bytes behind every block): accepted, all three at once
    if (layout == WIDE) {
        const uint64_t gap = block + 4 * blk;
        check("hyper, info and norm_sq in one gap", good, total, gap, total <= 48 ? gap + 48 : norm_sq, gap + 32, 1);
        check("hyper at the tail of a gap", good, total, gap + 256 - 32, norm_sq, info, 1);
        check("hyper over the end of a gap", good, total, gap + 256 - 16, norm_sq, info, b + 1 < total ? 0 : -1);
        check("info at the tail of a gap", good, total, hyper, norm_sq, gap + 256 - 16, 1);
    }
    // the three against each other
    check("info inside hyper", good, total, hyper, norm_sq, hyper + 16, 0);
    check("info behind hyper", good, total, hyper, norm_sq, hyper + 32, 1);
    check("norm_sq's last float on info", good, total, hyper, info - 4 * total + 4, info, 0);
    check("norm_sq up to info", good, total, hyper, info - 4 * total, info, 1);
    check("norm_sq on hyper's last float", good, total, hyper, hyper + 28, info, 0);
}

int main() {
    Rng rng{20261020};
    const uint64_t totals[] = {8, 16, 64};
    for (int rep = 0; rep < 72; ++rep) {
        const uint64_t total = totals[rep % 3];
        const Layout layout = (Layout)((rep / 3) % LAYOUTS);
        // the brute force is quadratic in count x total: the full launch of 32 buckets at 8 and 16 ranks, 12 at 64
        const int count = rep < 2 ? 32 : rep == 2 ? 12 : 1 + (int)rng.next(6);
        const int rounds = rep < 3 ? 1 : 3;
        uint64_t end;
        const std::vector<AdamwRange> good = make(rng, count, total, layout, &end);
        const uint64_t far = end + (1ull << 30);
        for (int m = 0; m < rounds; ++m) mutants(rng, good, total, far, layout);
        const uint64_t span = end - (1ull << 40);
        for (int m = 0; m < 4 * rounds; ++m) {   // anywhere over the list's span: whatever brute force says
            check("hyper anywhere", good, total, (1ull << 40) + 16 * rng.next(span / 16), far, far + 4096, -1);
            check("norm_sq anywhere", good, total, far, (1ull << 40) + 4 * rng.next(span / 4), far + 4096, -1);
            check("info anywhere", good, total, far, far + 4096, (1ull << 40) + 16 * rng.next(span / 16), -1);
        }
        // a plane moved anywhere inside the span, 16-byte aligned
        for (int m = 0; m < 2 * rounds; ++m) {
            std::vector<AdamwRange> moved = good;
            moved[rng.next(moved.size())].plane[rng.next(4)] = at((1ull << 40) + 16 * rng.next(span / 16));
            check("a plane anywhere", moved, total, far, far + 4096, far + 8192, -1);
        }
    }
    // the top of the address space
    {
        const uint64_t top = (uint64_t)UINTPTR_MAX, total = 8, far = 1ull << 44;
        std::vector<AdamwRange> one = {AdamwRange{at(1ull << 40), 2048, 2048, {at(1ull << 41), at(1ull << 42), at(1ull << 43), at(3ull << 42)}, 256}};
        check("the list", one, total, far, far + 64, far + 128, 1);
        for (int64_t d : {-16, 0, 16}) {
            check("hyper at the top", one, total, top - 31 - 16 + (uint64_t)d, far, far + 128, d <= 0 ? 1 : 0);
            check("info at the top", one, total, far, far + 64, top - 15 - 16 + (uint64_t)d, d <= 0 ? 1 : 0);
        }
        check("norm_sq ending at the top", one, total, far, top - 31 - 4, far + 128, 1);
        check("norm_sq past the top", one, total, far, top - 27, far + 128, 0);
        std::vector<AdamwRange> bad = one;
        bad[0].plane[3] = at(top - 15 - 4 * (7 * 256 + 256) + 16);   // the last block ends 1 past the top
        check("a plane past the top", bad, total, far, far + 64, far + 128, 0);
        bad[0].plane[3] = at(top - 15 - 4 * (7 * 256 + 256));
        check("a plane ending at the top", bad, total, far, far + 64, far + 128, 1);
        bad = one;
        bad[0].shard_stride = 1ull << 62;
        check("a stride that overflows", bad, total, far, far + 64, far + 128, 0);
        bad[0].shard_stride = 1ull << 63;
        check("a stride that overflows in the doubling", bad, total, far, far + 64, far + 128, 0);
        std::vector<AdamwRange> none;
        check("count == 0, apart", none, total, far, far + 64, far + 128, 1);
        check("count == 0, info on hyper", none, total, far, far + 64, far + 16, 0);

        // the argument rules that need no plan
        using namespace tsa;
        expect("pointers ok", adamw_pointers_ok(at(far), at(far + 64), at(far + 128), 0, false));
        expect("pointers ok with the flag, without norm_sq and info", adamw_pointers_ok(at(far), nullptr, nullptr, 1, false));
        for (int flags : {2, 3, 0x100, -2}) expect("an unknown flag bit", !adamw_pointers_ok(at(far), nullptr, nullptr, flags, false));
        expect("hyper NULL", !adamw_pointers_ok(nullptr, nullptr, nullptr, 0, false));
        expect("hyper NULL in the launch count's query", adamw_pointers_ok(nullptr, nullptr, nullptr, 0, true));
        expect("hyper 8-byte aligned", !adamw_pointers_ok(at(far + 8), nullptr, nullptr, 0, false));
        expect("norm_sq 2-byte aligned", !adamw_pointers_ok(at(far), at(far + 66), nullptr, 0, false));
        expect("norm_sq 4-byte aligned", adamw_pointers_ok(at(far), at(far + 68), nullptr, 0, false));
        expect("info 8-byte aligned", !adamw_pointers_ok(at(far), nullptr, at(far + 136), 0, false));
        auto verdict = [&](const std::vector<AdamwRange>& l, uint64_t tot) {
            return adamw_list_verdict(l.data(), (int)l.size(), tot, at(far), at(far + 64), at(far + 128));
        };
        expect("the list is fine", verdict(one, total) == kAdamwOk);
        expect("an empty list is fine", verdict(none, total) == kAdamwOk);
        for (int k = 0; k < 4; ++k) {
            bad = one;
            bad[0].plane[k] = nullptr;
            expect("a NULL plane", verdict(bad, total) == kAdamwArg);
            bad[0].plane[k] = at(addr(one[0].plane[k]) + 4);
            expect("a plane off by one float", verdict(bad, total) == kAdamwArg);
            bad[0].plane[k] = at(addr(one[0].plane[k]) + 8);
            expect("a plane 8-byte aligned", verdict(bad, total) == kAdamwArg);
            bad[0].plane[k] = at(addr(one[0].plane[k]) + 16);
            expect("a plane 16 bytes on", verdict(bad, total) == kAdamwOk);
        }
        bad = one;
        bad[0].shard_stride = 252;
        expect("shard_stride < blk", verdict(bad, total) == kAdamwArg);
        bad[0].shard_stride = 258;
        expect("shard_stride % 4 != 0", verdict(bad, total) == kAdamwArg);
        bad[0].shard_stride = 260;
        expect("a wide stride", verdict(bad, total) == kAdamwOk);
        bad[0].shard_stride = 1ull << 62;
        expect("overflow", verdict(bad, total) == kAdamwArg);
        bad = one;
        bad[0].plane[1] = bad[0].plane[0];
        expect("param == grad", verdict(bad, total) == kAdamwArg);
        // not whole tiles: unsupported for the whole list, wherever the bucket stands — and an argument error wins
        std::vector<AdamwRange> two = one;
        two.push_back(AdamwRange{at(5ull << 40), 8 * 8 * 3, 8 * 8 * 3, {at(20ull << 40), at(21ull << 40), at(22ull << 40), at(23ull << 40)}, 24});
        expect("a part tile behind", verdict(two, total) == kAdamwUnsupported);
        std::swap(two[0], two[1]);
        expect("a part tile in front", verdict(two, total) == kAdamwUnsupported);
        two[1].plane[2] = nullptr;
        expect("an argument error wins", verdict(two, total) == kAdamwArg);
        std::vector<AdamwRange> four = {AdamwRange{at(1ull << 40), 1024, 1024, {at(1ull << 41), at(1ull << 42), at(1ull << 43), at(3ull << 42)}, 256}};
        expect("below 8 ranks", verdict(four, 4) == kAdamwUnsupported);
    }
    if (g_accepted < 300 || g_refused < 1000) {
        std::printf("MISMATCH the checks do not reach both verdicts: %llu accepted, %llu refused\n", g_accepted, g_refused);
        return 1;
    }
    std::printf("adamw_ranges ok: %llu checks, %llu accepted, %llu refused\n", g_checks, g_accepted, g_refused);
    return 0;
}
"""

LAYOUT = r"""
#include <cstddef>
#include <cstdio>
#include "allred.h"
int main() {
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(allred_adamw_bucket_f32),
                offsetof(allred_adamw_bucket_f32, ranks), offsetof(allred_adamw_bucket_f32, rank_stride),
                offsetof(allred_adamw_bucket_f32, elems_per_rank), offsetof(allred_adamw_bucket_f32, param),
                offsetof(allred_adamw_bucket_f32, grad), offsetof(allred_adamw_bucket_f32, exp_avg),
                offsetof(allred_adamw_bucket_f32, exp_avg_sq), offsetof(allred_adamw_bucket_f32, shard_stride),
                sizeof(allred_adamw_hyper), ALLRED_ADAMW_GROUP_MAX, ALLRED_ADAMW_ZERO_GRAD);
    return 0;
}
"""


def test_adamw_bucket_binding_matches_the_header(tmp_path):
    """_lib.AdamwBucketF32 mirrors allred_adamw_bucket_f32; the constants and adamw_hyper's 32 bytes agree."""
    import ctypes as C

    import numpy as np

    import tenstorrentallreduce_amd as t
    from tenstorrentallreduce_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    b = _lib.AdamwBucketF32
    h = t.adamw_hyper(1e-3, (0.9, 0.999), 1e-8, 0.01, 3, 1.0)
    assert out == [C.sizeof(b), b.ranks.offset, b.rank_stride.offset, b.elems_per_rank.offset, b.param.offset, b.grad.offset,
                   b.exp_avg.offset, b.exp_avg_sq.offset, b.shard_stride.offset, h.nbytes, _lib.ADAMW_GROUP_MAX,
                   _lib.ADAMW_ZERO_GRAD]
    assert out[0] == 64 and h.dtype == np.float32 and h.shape == (8,)
    # the bias corrections: float64, rounded once
    assert h[5] == np.float32(1.0 - 0.9 ** 3) and h[6] == np.float32(np.sqrt(np.float64(1.0 - 0.999 ** 3)))
    assert np.isinf(t.adamw_hyper(1e-3, (0.9, 0.999), 1e-8, 0.01, 1)[7])


def test_adamw_entry_points_refuse_before_any_hip_call():
    """no GPU here: a call that got as far as HIP would not return ALLRED_ERR_ARG"""
    from tenstorrentallreduce_amd import _lib
    lib = _lib.lib
    arr = (_lib.AdamwBucketF32 * 1)((1 << 40, 2048, 2048, 1 << 41, 1 << 42, 1 << 43, 3 << 42, 256))
    assert lib.allred_plan_adamw_all_gather_shards_f32(None, arr, 1, 1 << 44, None, None, 0, None) == _lib.ERR_ARG
    assert lib.allred_plan_adamw_all_gather_shards_f32(None, arr, 1, None, None, None, 2, None) == _lib.ERR_ARG
    assert lib.allred_plan_adamw_shards_f32_launches(None, arr, 1) == _lib.ERR_ARG


def test_adamw_lists_disjoint_matches_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the adamw_ranges check"
    src = tmp_path / "adamw_ranges_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "adamw_ranges_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "adamw_ranges ok" in run.stdout
