"""Grouped fused BO allreduce / reduce-scatter against per-bucket calls: 8x8 Swing, 64
ranks, lists of small buckets, one GPU.

Arms, for each bucket list and for allreduce and reduce-scatter, alternated in one process:
  a  the grouped call (Plan.execute_group / Plan.reduce_scatter_group)   one launch
  b  the same buckets through per-bucket plans in a loop                 one launch each
Bucket lists (a tile is 256 elements of every rank; rows at preferred_rank_stride):
  sixteen_64     sixteen buckets of 64 tiles (32 kB per rank)
  mixed          eight buckets of 640, 64, 320, 128, 64, 640, 128, 320 tiles
Bar: a's median below b's minimum on every list, for both collectives.
Informative: one grouped launch of the sixteen 64-tile buckets against ONE plain
k_tree_lds_pipe pass over a single bucket of the same 1024 tiles (fused_form 3): the cost
of the table walk.
Each list's algorithmic bytes / 8 TB/s is recorded as the floor.

Before anything is timed, arm a's output on the pristine data is compared bit for bit with
arm b's ("verified").  A round times each arm over WINDOWS windows of CALLS calls between
device events; the pristine buckets (values near 2^-120, so 32 in-place allreduces of 64
ranks stay finite) are restored before every window, outside the events.  Two modes: eager
(plain calls from Python: what a caller pays, host enqueue included) and graph (the window's
calls captured once into a HIP graph and replayed: the device side alone).  Writes one JSON
(default profiles/group_buckets.json, --out PATH) and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 20
LISTS = {"sixteen_64": [64] * 16, "mixed": [640, 64, 320, 128, 64, 640, 128, 320]}
HBM_PEAK = 8e12   # bytes / s


class Buckets:
    def __init__(self, tiles, dev, seed):
        rng = np.random.default_rng(seed)
        self.n = [256 * k for k in tiles]
        self.stride = [t.preferred_rank_stride(n) for n in self.n]
        self.pristine, self.buf = [], []
        for n, stride in zip(self.n, self.stride):
            host = np.zeros((P, stride), dtype=np.uint16)
            host[:, :n] = rng.integers(0x0380, 0x0400, (P, n))   # bf16 in [2^-120, 2^-119)
            self.pristine.append(torch.from_numpy(host.view(np.int16)).to(dev))
            self.buf.append(self.pristine[-1].clone())
        self.args = [(b.data_ptr(), s, n) for b, s, n in zip(self.buf, self.stride, self.n)]

    def restore(self):
        for b, p in zip(self.buf, self.pristine):
            b.copy_(p)

    def snapshot(self):
        torch.cuda.synchronize()
        return [b.clone() for b in self.buf]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_buckets.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    group = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    plans = {}

    def plan_for(n):
        if n not in plans:
            plans[n] = t.Plan(t.SWING, t.BO, SIDE, n, P, t.EXEC_FUSED)
        return plans[n]

    arms, restores, verified, floors, launches = {}, {}, {}, {}, {}
    for li, (name, tiles) in enumerate(LISTS.items()):
        bk = Buckets(tiles, dev, seed=2 + li)
        per = [(plan_for(n), ptr, stride) for ptr, stride, n in bk.args]

        def grouped_ar(bk=bk):
            group.execute_group(bk.args, s)

        def loop_ar(per=per):
            for plan, ptr, stride in per:
                plan.execute(ptr, stride, None, s)

        def grouped_rs(bk=bk):
            group.reduce_scatter_group(bk.args, s)

        def loop_rs(per=per):
            for plan, ptr, stride in per:
                plan.reduce_scatter(ptr, stride, stream=s)

        for coll, a, b in (("allreduce", grouped_ar, loop_ar), ("reduce_scatter", grouped_rs, loop_rs)):
            key = f"{name}/{coll}"
            arms[f"{key}/a_grouped"], arms[f"{key}/b_loop"] = a, b
            restores[f"{key}/a_grouped"] = restores[f"{key}/b_loop"] = bk.restore
            # bit-exact against the loop arm, before anything is timed
            with torch.cuda.stream(s):
                bk.restore()
                b()
                want = bk.snapshot()
                bk.restore()
                a()
                got = bk.snapshot()
            verified[key] = all(bool(torch.equal(x, y)) for x, y in zip(got, want))
            moved = sum((2 * P if coll == "allreduce" else P + 1) * n * 2 for n in bk.n)
            floors[key] = {"algorithmic_bytes": moved, "floor_us": round(moved / HBM_PEAK * 1e6, 3)}
        launches[name] = {"a_grouped": group.group_launches(bk.args), "b_loop": sum(p.launches for p, _, _ in per)}

    # informative: the sixteen 64-tile buckets in one grouped launch against one plain pipe pass over 1024 tiles
    single = Buckets([64 * 16], dev, seed=9)
    single_plan = plan_for(single.n[0])

    def pipe_single():
        single_plan.execute(single.args[0][0], single.args[0][1], None, s)

    arms["sixteen_64/allreduce/c_one_pipe_pass_1024_tiles"] = pipe_single
    restores["sixteen_64/allreduce/c_one_pipe_pass_1024_tiles"] = single.restore
    tunes = {"sixteen_64/allreduce/c_one_pipe_pass_1024_tiles": {"fused_form": 3}}   # set around a whole window

    if not all(verified.values()):   # nothing is timed on wrong output
        print(json.dumps({"verified": False, "verified_per_arm": verified}))
        print("NOT verified: the grouped call differs from the per-bucket loop")
        return 1

    def window(key, calls, graph=None):
        with t.tuned(**tunes.get(key, {})), torch.cuda.stream(s):
            restores[key]()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            if graph is not None:
                graph.replay()
            else:
                for _ in range(calls):
                    arms[key]()
            e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    def capture(key):
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with t.tuned(**tunes.get(key, {})), torch.cuda.graph(g, stream=s):
            for _ in range(CALLS):
                arms[key]()
        torch.cuda.synchronize()
        return g

    results = {}
    for mode in ("eager", "graph"):
        graphs = {k: capture(k) if mode == "graph" else None for k in arms}
        for k in arms:
            window(k, WARMUP, graphs[k])
        us = {k: [] for k in arms}
        for _ in range(ROUNDS):
            for k in arms:
                us[k].append(sum(window(k, CALLS, graphs[k]) for _ in range(WINDOWS)) / (WINDOWS * CALLS))
        results[mode] = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3),
                             "max_us": round(max(v), 3), "rounds_us": [round(x, 3) for x in v]} for k, v in us.items()}
        del graphs

    for p in plans.values():
        p.close()
    group.close()

    bars = {}
    for mode, res in results.items():
        for key in floors:
            a, b = res[f"{key}/a_grouped"], res[f"{key}/b_loop"]
            bars[f"{mode}/{key}"] = {"a_median_us": a["median_us"], "b_min_us": b["min_us"],
                                     "a_median_below_b_min": a["median_us"] < b["min_us"],
                                     "b_over_a": round(b["median_us"] / a["median_us"], 3),
                                     "a_over_floor": round(a["median_us"] / floors[key]["floor_us"], 2)}
    walk = {mode: round(res["sixteen_64/allreduce/a_grouped"]["median_us"] /
                        res["sixteen_64/allreduce/c_one_pipe_pass_1024_tiles"]["median_us"], 4)
            for mode, res in results.items()}
    out = {
        "shape": {"algo": "swing", "side": SIDE, "ranks": P, "tile_elems": 256,
                  "lists_tiles_per_rank": LISTS, "rank_stride": "preferred_rank_stride(n) per bucket"},
        "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS, "warmup_calls": WARMUP,
        "hbm_peak_TBps": HBM_PEAK / 1e12, "floor": floors, "launches_per_call": launches,
        "arms": results, "bar": "a_grouped median < b_loop minimum, every list, both collectives",
        "bars": bars, "bar_met": {mode: all(v["a_median_below_b_min"] for k, v in bars.items() if k.startswith(mode))
                                  for mode in results},
        "grouped_16x64_over_one_pipe_pass_1024": walk,
        "verified": all(verified.values()), "verified_per_arm": verified,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    print("verified" if out["verified"] else "NOT verified: the grouped call differs from the per-bucket loop")
    return 0 if out["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
