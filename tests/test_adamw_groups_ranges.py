"""csrc/adamw_ranges.hpp as extended for allred_plan_adamw_all_gather_shards_f32_groups, against
brute force, on the CPU, on tests/test_adamw_ranges.py's model: a stand-alone C++ program (its own
main) compiled with g++ under AddressSanitizer and UBSan and run directly; host code only, nothing
is loaded into Python.

The call reads an ARRAY of ngroups hyper sets, so hyper's interval is [hyper, + 32 ngroups): the
defaulted hyper_bytes argument of adamw_lists_disjoint / adamw_list_verdict.  Checked against a
pairwise brute force in unsigned 128-bit arithmetic for every ngroups 1 .. 8: the array far away; in
the gap of a wide stride (256 bytes: exactly eight sets) at its head, at its tail and one set over
its end; the LAST set's 32 bytes on the first bytes of a plane block, of norm_sq and on info, while
the first sets are clear — a rule that still assumed 32 bytes would accept these —; random
placements all over a list's span.  The default is still the one set's 32 bytes.

adamw_groups_ok is the two group rules: 1 <= ngroups <= 8, every group_of[i] < ngroups;
group_of == NULL is every bucket in group 0.  A plan cannot be made without a device, so through the
entry point itself only refusals that come before the plan is looked at are reachable here.
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

// the rule, written out: every interval against every other; hyper's is 32 G bytes
static bool brute(const std::vector<AdamwRange>& list, uint64_t total, uint64_t hyper, uint64_t G, uint64_t norm_sq, uint64_t info) {
    std::vector<I> v;
    if (hyper) v.push_back(I{(u128)hyper, (u128)hyper + (u128)32 * G});
    if (norm_sq) v.push_back(I{(u128)norm_sq, (u128)norm_sq + (u128)4 * total});
    if (info) v.push_back(I{(u128)info, (u128)info + 16});
    for (const AdamwRange& s : list) {
        v.push_back(I{(u128)addr(s.ranks), (u128)addr(s.ranks) + (u128)2 * total * s.stride});
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
static void check(const char* what, const std::vector<AdamwRange>& list, uint64_t total, uint64_t hyper, uint64_t G,
                  uint64_t norm_sq, uint64_t info, int want) {
    const bool got = tsa::adamw_lists_disjoint(list.data(), (int)list.size(), total, at(hyper), at(norm_sq), at(info), 32 * G);
    const bool ref = brute(list, total, hyper, G, norm_sq, info);
    // the verdict of the whole list says the same: these lists pass every other rule
    const bool ver = tsa::adamw_list_verdict(list.data(), (int)list.size(), total, at(hyper), at(norm_sq), at(info), 32 * G) == tsa::kAdamwOk;
    ++g_checks;
    ++(ref ? g_accepted : g_refused);
    if (got != ref || ver != ref || (want >= 0 && ref != (want == 1))) {
        std::printf("MISMATCH %s: count=%zu total=%llu G=%llu hyper=%llx norm_sq=%llx info=%llx got=%d verdict=%d brute=%d want=%d\n",
                    what, list.size(), (unsigned long long)total, (unsigned long long)G, (unsigned long long)hyper,
                    (unsigned long long)norm_sq, (unsigned long long)info, (int)got, (int)ver, (int)ref, want);
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

// an accepted WIDE list of whole-tile buckets: rank rows in buffers of their own, every plane with a
// gap of 256 bytes behind every block; *end: the first byte behind everything
static std::vector<AdamwRange> make(Rng& rng, int count, uint64_t total, uint64_t* end) {
    std::vector<AdamwRange> list((size_t)count);
    uint64_t cursor = (1ull << 40) + 16 * rng.next(1000);
    for (int i = 0; i < count; ++i) {
        AdamwRange& s = list[(size_t)i];
        s.n = 256 * total * (1 + rng.next(3));
        s.stride = s.n + (i % 2 ? 64 : 0);
        s.ranks = at(cursor);
        cursor += 2 * total * s.stride + 16 * rng.next(8);
        s.shard_stride = s.n / total + 64;
        for (int k = 0; k < 4; ++k) {
            s.plane[k] = at(cursor);
            cursor += 4 * total * s.shard_stride + 16 * rng.next(4);
        }
    }
    *end = cursor;
    return list;
}

int main() {
    Rng rng{20261021};
    const uint64_t totals[] = {8, 16, 64};
    for (int rep = 0; rep < 9; ++rep) {
        const uint64_t total = totals[rep % 3];
        uint64_t end;
        const std::vector<AdamwRange> good = make(rng, 1 + (int)rng.next(4), total, &end);
        const uint64_t far = end + (1ull << 30), norm_sq = far + 4096, info = far + 8192, span = end - (1ull << 40);
        for (uint64_t G = 1; G <= 8; ++G) {
            const uint64_t len = 32 * G;
            check("the array far away", good, total, far, G, norm_sq, info, 1);
            check("without norm_sq and info", good, total, far, G, 0, 0, 1);
            const AdamwRange& t = good[rng.next(good.size())];
            const int k = (int)rng.next(4);
            const uint64_t b = rng.next(total - 1), blk = t.n / total;   // not the last block: another follows its gap
            const uint64_t block = addr(t.plane[k]) + 4 * b * t.shard_stride, gap = block + 4 * blk, next = gap + 256;
            // in the gap (256 bytes = eight sets)
            check("the array at the head of a gap", good, total, gap, G, norm_sq, info, 1);
            check("the array at the tail of a gap", good, total, next - len, G, norm_sq, info, 1);
            check("the last set on the next block's first 16 bytes", good, total, next - len + 16, G, norm_sq, info, 0);
            check("the last set over the next block's first 32 bytes", good, total, next - len + 32, G, norm_sq, info, 0);
            check("the first set on a block's last 16 bytes", good, total, gap - 16, G, norm_sq, info, 0);
            if (gap + len + 16 + 4 * total <= next)
                check("the array, info behind it and norm_sq in one gap", good, total, gap, G, next - 4 * total, gap + len, 1);
            // the last set's bytes touching norm_sq and info, the sets before it clear
            check("info inside the last set", good, total, far, G, norm_sq, far + len - 16, 0);
            check("info on the last set's first half", good, total, far, G, norm_sq, far + len - 32, 0);
            check("info behind the last set", good, total, far, G, norm_sq, far + len, 1);
            check("norm_sq on the last set's last float", good, total, far, G, far + len - 4, info, 0);
            check("norm_sq behind the last set", good, total, far, G, far + len, info, 1);
            check("the array up to norm_sq", good, total, norm_sq - len, G, norm_sq, info, 1);
            check("the last set's last 16 bytes on norm_sq", good, total, norm_sq - len + 16, G, norm_sq, info, 0);
            check("the array up to info", good, total, info - len, G, norm_sq, info, norm_sq + 4 * total <= info - len ? 1 : -1);
            check("the last set's last 16 bytes on info", good, total, info - len + 16, G, norm_sq, info, 0);
            // a plane block / a row on the last set
            check("the last set on a plane block's first bytes", good, total, block - len + 16, G, norm_sq, info, b > 0 || G > 1 ? -1 : 0);
            check("the last set on a row's first bytes", good, total, addr(t.ranks) - len + 16, G, norm_sq, info, -1);
            for (int m = 0; m < 6; ++m)
                check("the array anywhere", good, total, (1ull << 40) + 16 * rng.next(span / 16), G, norm_sq, info, -1);
            // the top of the address space
            const uint64_t top = (uint64_t)UINTPTR_MAX;
            check("the array ending at the top", good, total, top - 15 - len, G, norm_sq, info, 1);
            check("the array past the top", good, total, top - 15 - len + 32, G, norm_sq, info, 0);
        }
        // the default is the one set's 32 bytes
        const bool one = tsa::adamw_lists_disjoint(good.data(), (int)good.size(), total, at(far), at(far + 32), at(info));
        const bool two = tsa::adamw_lists_disjoint(good.data(), (int)good.size(), total, at(far), at(far + 32), at(info), 64);
        expect("norm_sq behind ONE set: accepted by default, refused with two sets", one && !two);
        expect("the default verdict", tsa::adamw_list_verdict(good.data(), (int)good.size(), total, at(far), at(far + 32), at(info)) == tsa::kAdamwOk);
        expect("the verdict with two sets", tsa::adamw_list_verdict(good.data(), (int)good.size(), total, at(far), at(far + 32), at(info), 64) == tsa::kAdamwArg);
    }
    // count == 0: the small intervals still go against each other
    {
        std::vector<AdamwRange> none;
        const uint64_t far = 1ull << 44;
        check("count == 0, apart", none, 8, far, 8, far + 256, far + 512, 1);
        check("count == 0, info inside the eighth set", none, 8, far, 8, far + 1024, far + 240, 0);
        check("count == 0, info inside what would be the eighth set, seven sets", none, 8, far, 7, far + 1024, far + 240, 1);
    }
    // the group rules
    {
        using tsa::adamw_groups_ok;
        static_assert(tsa::kAdamwParamGroupsMax == 8, "ALLRED_ADAMW_PARAM_GROUPS_MAX");
        const std::vector<uint8_t> g012 = {0, 1, 2, 1};
        for (int n : {-1, 0, 9, 10, 255, 256, 1 << 20}) {
            expect("ngroups out of bounds, no list", !adamw_groups_ok(nullptr, 0, n));
            expect("ngroups out of bounds, a list", !adamw_groups_ok(g012.data(), 4, n));
        }
        for (int n = 1; n <= 8; ++n) {
            expect("ngroups in bounds, group_of NULL", adamw_groups_ok(nullptr, 4, n));
            expect("ngroups in bounds, group_of NULL, no list", adamw_groups_ok(nullptr, 0, n));
            expect("ngroups in bounds, count == 0: group_of is not read", adamw_groups_ok(g012.data(), 0, n));
            expect("ngroups in bounds, count < 0: group_of is not read", adamw_groups_ok(g012.data(), -1, n));
            expect("groups 0 .. 2", adamw_groups_ok(g012.data(), 4, n) == (n >= 3));
            for (int where = 0; where < 4; ++where) {   // a group index equal to ngroups, anywhere in the list
                std::vector<uint8_t> bad(4, 0);
                bad[(size_t)where] = (uint8_t)n;
                expect("a group index equal to ngroups", !adamw_groups_ok(bad.data(), 4, n));
                expect("... behind the list's end: not read", adamw_groups_ok(bad.data(), where, n));
                bad[(size_t)where] = (uint8_t)(n - 1);
                expect("the last group", adamw_groups_ok(bad.data(), 4, n));
                bad[(size_t)where] = 255;
                expect("group 255", !adamw_groups_ok(bad.data(), 4, n));
            }
        }
        std::vector<uint8_t> all(65);   // a list of three launches
        for (size_t i = 0; i < all.size(); ++i) all[i] = (uint8_t)(i % 3);
        expect("65 buckets, i % 3", adamw_groups_ok(all.data(), 65, 3) && !adamw_groups_ok(all.data(), 65, 2));
        all[64] = 3;
        expect("the 65th bucket's group", !adamw_groups_ok(all.data(), 65, 3) && adamw_groups_ok(all.data(), 64, 3));
    }
    if (g_accepted < 300 || g_refused < 300) {
        std::printf("MISMATCH the checks do not reach both verdicts: %llu accepted, %llu refused\n", g_accepted, g_refused);
        return 1;
    }
    std::printf("adamw_groups_ranges ok: %llu checks, %llu accepted, %llu refused\n", g_checks, g_accepted, g_refused);
    return 0;
}
"""

LAYOUT = r"""
#include <cstdio>
#include "allred.h"
int main() {
    std::printf("%d %d\n", ALLRED_ADAMW_PARAM_GROUPS_MAX, ALLRED_ADAMW_GROUP_MAX);
    return 0;
}
"""


def test_constants_and_hyper_groups_match_the_header(tmp_path):
    import numpy as np

    import tenstorrentallreduce_amd as t
    from tenstorrentallreduce_amd import _lib
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [_lib.ADAMW_PARAM_GROUPS_MAX, _lib.ADAMW_GROUP_MAX] and t.ADAMW_PARAM_GROUPS_MAX == 8
    groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)]
    h = t.adamw_hyper_groups(groups, step=3, max_norm=0.5)
    assert h.shape == (2, 8) and h.dtype == np.float32 and h.nbytes == 64 and h.flags["C_CONTIGUOUS"]
    for row, g in zip(h, groups):
        assert np.array_equal(row, t.adamw_hyper(g["lr"], g["betas"], g["eps"], g["weight_decay"], 3, 0.5))
    assert np.isinf(t.adamw_hyper_groups(groups)[:, 7]).all()
    for bad in ([], groups * 5):
        try:
            t.adamw_hyper_groups(bad)
        except ValueError:
            continue
        raise AssertionError(f"{len(bad)} groups accepted")


def test_groups_entry_point_refuses_before_any_hip_call():
    """no GPU here: a call that got as far as HIP would not return ALLRED_ERR_ARG"""
    import ctypes as C

    from tenstorrentallreduce_amd import _lib
    lib = _lib.lib
    arr = (_lib.AdamwBucketF32 * 1)((1 << 40, 2048, 2048, 1 << 41, 1 << 42, 1 << 43, 3 << 42, 256))
    call = lib.allred_plan_adamw_all_gather_shards_f32_groups
    g0, g1 = (C.c_uint8 * 1)(0), (C.c_uint8 * 1)(1)
    assert call(None, arr, g0, 1, 1 << 44, 1, None, None, 0, None) == _lib.ERR_ARG      # no plan
    assert call(None, arr, None, 1, 1 << 44, 0, None, None, 0, None) == _lib.ERR_ARG    # ngroups 0
    assert call(None, arr, None, 1, 1 << 44, 9, None, None, 0, None) == _lib.ERR_ARG    # ngroups 9
    assert call(None, arr, g1, 1, 1 << 44, 1, None, None, 0, None) == _lib.ERR_ARG      # a group index equal to ngroups
    assert call(None, None, None, 0, (1 << 44) + 8, 1, None, None, 0, None) == _lib.ERR_ARG   # hyper misaligned
    assert call(None, None, None, 0, 1 << 44, 3, None, (1 << 44) + 80, 0, None) == _lib.ERR_ARG   # no plan (the overlap comes later)


def test_hyper_array_interval_and_group_rules_match_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the adamw_ranges check"
    src = tmp_path / "adamw_groups_ranges_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "adamw_groups_ranges_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "adamw_groups_ranges ok" in run.stdout
