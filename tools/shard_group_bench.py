"""Grouped all-gather and grouped reduce-scatter into shard buffers against per-bucket calls:
8x8 Swing, 64 ranks, lists of small buckets, one GPU.

Arms, for each bucket list and each of three collectives, alternated in one process:
  a  the grouped call (Plan.all_gather_shards / Plan.reduce_scatter_shards)      one launch
  b  the same buckets through per-bucket Plan.all_gather(in=...) /
     Plan.reduce_scatter(out=...) in a loop                                       one launch each
Collectives:
  all_gather                 in place: block b of rank b to every rank
  all_gather_flat            from ONE rank-major flat shard buffer (64 rows of F = sum of blk
                             elements; bucket i's shard at column off_i, shard_stride = F)
  reduce_scatter_flat        into that same buffer
Bucket lists (a tile is 256 elements of every rank; rows at preferred_rank_stride):
  sixteen_64     sixteen buckets of 64 tiles (32 kB per rank)
  mixed          eight buckets of 640, 64, 320, 128, 64, 640, 128, 320 tiles
Bar: a's median below b's minimum on every list, for every collective, in both modes.
Informative only:
  each list's floor, (P + 1) n 2 bytes / 8 TB/s;
  the grouped all-gather of the sixteen 64-tile buckets against ONE Plan.all_gather (k_ag) over a
    single bucket of the same 1024 tiles, one launch each: the cost of the table walk;
  one 960-tile bucket through the grouped call against Plan.all_gather of it: the one point next
    to the 1024-tile routing threshold the all-gather inherits from the tree passes;
  the grouped all-gather of both lists with the grid capped at 512 workgroups (pipe_grid), the
    tree passes' cap, next to its own cap of 2048.

Before anything is timed, arm a's output on the pristine data is compared bit for bit with arm
b's ("verified"), rank buffers and shard buffer alike.  A round times each arm over WINDOWS
windows of CALLS calls between device events; the pristine buffers are restored before every
window, outside the events.  Two modes: eager (plain calls from Python: what a caller pays, host
enqueue included) and graph (the window's calls captured once into a HIP graph and replayed: the
device side alone).  Writes one JSON (default profiles/group_shards.json, --out PATH) and prints
it."""
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
    """The rank buffers of a list and one rank-major flat shard buffer for all of them."""

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
        self.F = sum(n // P for n in self.n)
        flat = rng.integers(0x0380, 0x0400, (P, self.F)).astype(np.uint16)
        self.pristine.append(torch.from_numpy(flat.view(np.int16)).to(dev))
        self.buf.append(self.pristine[-1].clone())
        self.args = [(b.data_ptr(), s, n) for b, s, n in zip(self.buf, self.stride, self.n)]
        off, self.shard_args = 0, []
        for a, n in zip(self.args, self.n):
            self.shard_args.append(a + (self.buf[-1].data_ptr() + 2 * off, self.F))
            off += n // P

    def restore(self):
        for b, p in zip(self.buf, self.pristine):
            b.copy_(p)

    def snapshot(self):
        torch.cuda.synchronize()
        return [b.clone() for b in self.buf]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_shards.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    group = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    plans = {}

    def plan_for(n):
        if n not in plans:
            plans[n] = t.Plan(t.SWING, t.BO, SIDE, n, P, t.EXEC_FUSED)
        return plans[n]

    arms, restores, verified, floors, launches, tunes = {}, {}, {}, {}, {}, {}

    def collectives(bk):
        """name -> (grouped arm, loop arm, the op) of one set of buffers"""
        per = [(plan_for(n), ptr, stride, shard, ss) for ptr, stride, n, shard, ss in bk.shard_args]

        def grouped_ag():
            group.all_gather_shards(bk.args, s)

        def loop_ag():
            for plan, ptr, stride, _, _ in per:
                plan.all_gather(ptr, stride, stream=s)

        def grouped_ag_flat():
            group.all_gather_shards(bk.shard_args, s)

        def loop_ag_flat():
            for plan, ptr, stride, shard, ss in per:
                plan.all_gather(ptr, stride, shard, ss, stream=s)

        def grouped_rs_flat():
            group.reduce_scatter_shards(bk.shard_args, s)

        def loop_rs_flat():
            for plan, ptr, stride, shard, ss in per:
                plan.reduce_scatter(ptr, stride, shard, ss, stream=s)

        return {"all_gather": (grouped_ag, loop_ag, bk.args, t._lib.OP_ALL_GATHER),
                "all_gather_flat": (grouped_ag_flat, loop_ag_flat, bk.shard_args, t._lib.OP_ALL_GATHER),
                "reduce_scatter_flat": (grouped_rs_flat, loop_rs_flat, bk.shard_args, t._lib.OP_REDUCE_SCATTER)}

    def verify(bk, a, b, tune=None):
        """a's bits on the pristine data equal b's: every rank buffer and the shard buffer"""
        with torch.cuda.stream(s):
            bk.restore()
            b()
            want = bk.snapshot()
            bk.restore()
            with t.tuned(**(tune or {})):
                a()
            got = bk.snapshot()
        return all(bool(torch.equal(x, y)) for x, y in zip(got, want))

    for li, (name, tiles) in enumerate(LISTS.items()):
        bk = Buckets(tiles, dev, seed=2 + li)
        launches[name] = {}
        for coll, (a, b, lst, op) in collectives(bk).items():
            key = f"{name}/{coll}"
            arms[f"{key}/a_grouped"], arms[f"{key}/b_loop"] = a, b
            restores[f"{key}/a_grouped"] = restores[f"{key}/b_loop"] = bk.restore
            verified[key] = verify(bk, a, b)
            moved = sum((P + 1) * n * 2 for n in bk.n)
            floors[key] = {"algorithmic_bytes": moved, "floor_us": round(moved / HBM_PEAK * 1e6, 3)}
            launches[name][coll] = {"a_grouped": group.shards_launches(lst, op), "b_loop": len(lst)}
        # informative: the grouped all-gather under the tree passes' grid cap
        key = f"{name}/all_gather/a_grouped_grid512"
        arms[key], restores[key], tunes[key] = arms[f"{name}/all_gather/a_grouped"], bk.restore, {"pipe_grid": 512}
        verified[f"{name}/all_gather/grid512"] = verify(bk, arms[key], arms[f"{name}/all_gather/b_loop"], tunes[key])

    # informative: the sixteen 64-tile buckets in one grouped launch (the arm above) against ONE
    # Plan.all_gather over a single bucket of the same 1024 tiles
    single = Buckets([64 * 16], dev, seed=9)
    single_plan = plan_for(single.n[0])

    def ag_single():
        single_plan.all_gather(single.args[0][0], single.args[0][1], stream=s)

    arms["sixteen_64/all_gather/c_one_all_gather_1024_tiles"] = ag_single
    restores["sixteen_64/all_gather/c_one_all_gather_1024_tiles"] = single.restore

    # informative: one 960-tile bucket, next to the inherited 1024-tile threshold
    near = Buckets([960], dev, seed=10)
    near_plan = plan_for(near.n[0])

    def near_grouped():
        group.all_gather_shards(near.args, s)

    def near_single():
        near_plan.all_gather(near.args[0][0], near.args[0][1], stream=s)

    arms["one_960/all_gather/a_grouped"], arms["one_960/all_gather/b_plan_all_gather"] = near_grouped, near_single
    restores["one_960/all_gather/a_grouped"] = restores["one_960/all_gather/b_plan_all_gather"] = near.restore
    verified["one_960/all_gather"] = verify(near, near_grouped, near_single)
    launches["one_960"] = {"all_gather": {"a_grouped": group.shards_launches(near.args, t._lib.OP_ALL_GATHER), "b_loop": 1}}

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

    def ratio(res, x, y):
        return round(res[x]["median_us"] / res[y]["median_us"], 4)

    out = {
        "shape": {"algo": "swing", "side": SIDE, "ranks": P, "tile_elems": 256,
                  "lists_tiles_per_rank": LISTS, "rank_stride": "preferred_rank_stride(n) per bucket",
                  "flat_shard_buffer": "64 rows of F = sum of blk elements; bucket i at column off_i, shard_stride = F"},
        "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS, "warmup_calls": WARMUP,
        "hbm_peak_TBps": HBM_PEAK / 1e12, "floor": floors, "launches_per_call": launches,
        "arms": results,
        "bar": "a_grouped median < b_loop minimum, every list, every collective, both modes",
        "bars": bars, "bar_met": {mode: all(v["a_median_below_b_min"] for k, v in bars.items() if k.startswith(mode))
                                  for mode in results},
        "informative": {
            "grouped_16x64_all_gather_over_one_all_gather_1024_tiles": {
                mode: ratio(res, "sixteen_64/all_gather/a_grouped", "sixteen_64/all_gather/c_one_all_gather_1024_tiles")
                for mode, res in results.items()},
            "one_960_tile_bucket_grouped_over_plan_all_gather": {
                mode: ratio(res, "one_960/all_gather/a_grouped", "one_960/all_gather/b_plan_all_gather")
                for mode, res in results.items()},
            "all_gather_grid512_over_grid2048": {
                mode: {name: ratio(res, f"{name}/all_gather/a_grouped_grid512", f"{name}/all_gather/a_grouped")
                       for name in LISTS} for mode, res in results.items()},
        },
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
