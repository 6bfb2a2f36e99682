"""csrc/group_batch.hpp against a brute-force partition, on the CPU.

A stand-alone C++ program (its own main, g++ under AddressSanitizer and UBSan) reads bucket lists
from a file, walks each with group_batch<32> or group_batch<64> and prints what its callbacks saw,
in order: an own-route bucket when `add` routes it, a launch with its index, tile offset, grid, the
list positions of its members (read back out of the GroupSpan) and the state of the side table.
The expectation is written here without a pending counter: the grouped buckets, numbered r = 0, 1,
.. in list order, form launch r // CAP; that launch goes out right behind its member CAP - 1, the
last, partial one behind the end of the list; an own-route bucket appears at its place in the
list, in front of a launch still pending.  Lists: CAP 32 and 64, counts 0, 1, CAP, CAP + 1 and
2 CAP + 1 and random ones, without and with own-route buckets (of 0, 1 and 3 launches); each also
dry, whose return value must be the launches the real walk made; and with a failing launch
callback, which must end the walk.
"""
import os
import random
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tenstorrentallreduce_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
FAIL = -77        # what the failing launch callback returns
GRID_CAP = 24     # grid_of(tiles) = min(tiles, GRID_CAP)

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "group_batch.hpp"

struct Side {
    int who[tsa::kGroupMax];   // list position + 1 of the member in this slot
};

template <int CAP>
static void run(bool dry, int fail_at, const std::vector<long>& tiles, const std::vector<int>& own) {
    Side side{};
    auto add = [&](int i, int slot) {
        if (own[i] >= 0) {
            std::printf(" O %d", i);
            return tsa::BatchAdd::routed(ALLRED_OK, own[i]);
        }
        side.who[slot] = i + 1;
        return tsa::BatchAdd::member(tsa::GroupIn{reinterpret_cast<uint16_t*>((uintptr_t)0x1000 * (uintptr_t)(i + 1)),
                                                  (uint64_t)(7 + i), (uint64_t)tiles[i], 1});
    };
    auto grid_of = [](uint64_t t) { return (unsigned)(t < 24 ? t : 24); };
    auto launch = [&](const tsa::GroupSpan& span, unsigned grid, int index, uint64_t tile_off) {
        std::printf(" L %d %llu %u %u", index, (unsigned long long)tile_off, grid, span.T);
        int members = 0;
        for (int k = 0; k < tsa::kGroupMax && span.b[k].ranks; ++k, ++members) {
            const int i = (int)((uintptr_t)span.b[k].ranks / 0x1000) - 1;
            // the side table holds this launch's members and nothing of an earlier launch
            if (side.who[k] != i + 1 || span.b[k].stride != (uint64_t)(7 + i)) std::printf(" BAD-SLOT");
            std::printf(" %d", i);
        }
        for (int k = members; k < tsa::kGroupMax; ++k)
            if (side.who[k]) std::printf(" STALE-SLOT");
        std::printf(" ;");
        return index == fail_at ? -77 : ALLRED_OK;
    };
    const int r = tsa::group_batch<CAP>((int)tiles.size(), dry, side, add, grid_of, launch);
    std::printf(" = %d\n", r);
}

int main(int argc, char** argv) {
    std::FILE* f = std::fopen(argv[1], "r");
    if (argc < 2 || !f) return 2;
    int cap, dry, fail_at, n;
    while (std::fscanf(f, "%d %d %d %d", &cap, &dry, &fail_at, &n) == 4) {
        std::vector<long> tiles(n);
        std::vector<int> own(n);
        for (int i = 0; i < n; ++i)
            if (std::fscanf(f, "%ld %d", &tiles[i], &own[i]) != 2) return 2;
        if (cap == 32) run<32>(dry != 0, fail_at, tiles, own);
        else run<64>(dry != 0, fail_at, tiles, own);
    }
    std::fclose(f);
    return 0;
}
"""


def expected(cap, dry, fail_at, members):
    """the line the program must print for one list; members: [(tiles, own launches or -1)]"""
    grouped = [i for i, (_, own) in enumerate(members) if own < 0]
    launches = [grouped[k:k + cap] for k in range(0, len(grouped), cap)]
    own_total = sum(own for _, own in members if own >= 0)
    if dry:
        return "".join(" O %d" % i for i, (_, own) in enumerate(members) if own >= 0) + " = %d" % (len(launches) + own_total)
    out = []

    def launch(k):
        tiles = sum(members[i][0] for i in launches[k])
        off = sum(members[i][0] for prev in launches[:k] for i in prev)
        out.append(" L %d %d %d %d" % (k, off, min(tiles, GRID_CAP), tiles) + "".join(" %d" % i for i in launches[k]) + " ;")
        return k == fail_at

    for i, (_, own) in enumerate(members):
        if own >= 0:
            out.append(" O %d" % i)
        elif (grouped.index(i) + 1) % cap == 0 and launch(grouped.index(i) // cap):
            return "".join(out) + " = %d" % FAIL
    if len(grouped) % cap and launch(len(launches) - 1):
        return "".join(out) + " = %d" % FAIL
    return "".join(out) + " = 0"


def events(line):
    """[("O", i) | ("L", index, [members])] of a printed line"""
    out = []
    for part in line.split("=")[0].replace(" L ", " ; L ").replace(" O ", " ; O ").split(";"):
        tok = part.split()
        if tok and tok[0] == "O":
            out.append(("O", int(tok[1])))
        elif tok and tok[0] == "L":
            out.append(("L", int(tok[1]), [int(x) for x in tok[5:]]))
    return out


def cases():
    rng = random.Random(20250611)
    lists = []
    for cap in (32, 64):
        for count in (0, 1, cap, cap + 1, 2 * cap + 1):
            lists.append((cap, [(rng.randint(1, 40), -1) for _ in range(count)]))
            for _ in range(3):   # the same counts of GROUPED buckets with own-route ones strewn in
                members = [(rng.randint(1, 40), -1) for _ in range(count)]
                for _ in range(rng.randint(1, 6)):
                    members.insert(rng.randint(0, len(members)), (rng.randint(1, 40), rng.choice((0, 1, 1, 3))))
                lists.append((cap, members))
        for _ in range(12):
            lists.append((cap, [(rng.randint(1, 40), rng.choice((-1, -1, -1, -1, -1, 1, 3))) for _ in range(rng.randint(0, 3 * cap))]))
        lists.append((cap, [(5, 1)] * 3))   # own routes alone: no grouped launch at all
    out = []
    for cap, members in lists:
        out.append((cap, 0, -1, members))
        out.append((cap, 1, -1, members))
        n_launches = -(-sum(1 for _, own in members if own < 0) // cap)
        for fail_at in sorted({0, n_launches - 1} - {-1}):
            if n_launches:
                out.append((cap, 0, fail_at, members))
    return out


def test_group_batch_matches_brute_force(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the group_batch check"
    src = tmp_path / "group_batch_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "group_batch_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-I", INCLUDE, str(src),
                    "-o", str(exe)], check=True)
    todo = cases()
    lists = tmp_path / "lists.txt"
    lists.write_text("".join("%d %d %d %d %s\n" % (cap, dry, fail_at, len(m), " ".join("%d %d" % x for x in m))
                             for cap, dry, fail_at, m in todo))
    run = subprocess.run([str(exe), str(lists)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    got = run.stdout.splitlines()
    assert len(got) == len(todo)
    seen = {"own in front of a pending launch": 0, "stopped short": 0, "dry": 0}
    for line, (cap, dry, fail_at, members) in zip(got, todo):
        assert line == expected(cap, dry, fail_at, members), (cap, dry, fail_at, len(members))
        full = events(expected(cap, 0, -1, members))
        if dry:   # the count without dry: the launches made and the own routes' launches
            assert int(line.split("=")[1]) == sum(e[0] == "L" for e in full) + sum(own for _, own in members if own >= 0)
            seen["dry"] += 1
        elif fail_at >= 0:
            ev = events(line)
            assert ev[-1][0] == "L" and ev[-1][1] == fail_at and int(line.split("=")[1]) == FAIL
            seen["stopped short"] += len(ev) < len(full)
        else:
            for k, e in enumerate(full):
                if e[0] == "O":   # a later launch holds a bucket from in front of this one: it was pending, and stayed so
                    seen["own in front of a pending launch"] += any(l[0] == "L" and l[2][0] < e[1] for l in full[k + 1:])
    assert all(seen.values()), seen
