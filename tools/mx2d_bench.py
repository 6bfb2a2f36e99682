"""Both MXFP8 orientations from one all-gather pass (Plan.all_gather_shards_mxfp8_2d) against the row-wise call,
with the method of tools/adamw_mx_bench.py: 8x8 Swing, 64 ranks, one rank-major flat fp32
buffer, one GPU, replayed from a HIP graph (the device side alone), the floor scale rule.  A bucket is a matrix
W[nrows][cols]; at 64 ranks the MX rules (R = nrows / 64 a multiple of 32) make nrows >= 2048.  Shapes:
  buckets16   sixteen buckets of 2048 x 128 (262,144 elements per rank each, R = 32): the smallest at cols = 128;
  one_large   one bucket of 2048 x 160 (327,680 elements per rank, R = 32);
  tall4       four buckets of 4096 x 128 (R = 64): the shape at which a patch may be taller than a square.
Arms, alternated in one process:
  (a) both        the new call with both outputs                                                     one launch
  (b) t_only      the new call column-wise only                                                      one launch
  (c) rows_alone  all_gather_shards_mxfp8 alone: half the bytes, a floor, not a competitor           one launch
  (d) rows_twice  all_gather_shards_mxfp8 twice, the second time on a fp32 buffer that already holds W^T; making
                  that transposed fp32 copy is NOT timed, and no user has one: the comparator flatters itself
The expectation is (a)'s median at or below (d)'s minimum over the rounds; what was measured is written down
either way.  Before anything is timed every arm's outputs are verified bit for bit: (a) against tests/mx2d_ref.py
(rank 0's rows on the host, every other rank's against rank 0's on the device), (b), (c) and (d) against (a).
A round times each arm over WINDOWS replays of a graph of CALLS calls between device events; the outputs are
zeroed before every window, outside the events.  Eager calls, the host cost of the checks and the grid cap
(inherited from kMaxGrid) are not measured.  --arms ab --tag NAME: the patch-shape A/B, one build per process
(ALLRED_LIB_PATH), printing one line.  Writes one JSON (default profiles/mx2d_all_gather.json) and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mx2d_ref  # noqa: E402  (tests/mx2d_ref.py: the expectation)
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
SHAPES = {"buckets16": (16, 128, 32), "one_large": (1, 160, 32), "tall4": (4, 128, 64)}   # buckets, cols, R
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
ARMS = {"a": "both", "b": "t_only", "c": "rows_alone", "d": "rows_twice"}


def run_shape(name, plan, s, dev, rng, which):
    count, cols, R = SHAPES[name]
    nrows = P * R
    n, blk = nrows * cols, R * cols
    F = count * blk
    W = [rng.standard_normal((nrows, cols)).astype(np.float32) * np.exp2(rng.integers(-8, 8, (nrows, 1))).astype(np.float32)
         for _ in range(count)]
    flat = np.concatenate([mx2d_ref.blocks(w, P) for w in W], axis=1)                                 # (P, F): bucket i at column blk i
    flat_t = np.concatenate([np.ascontiguousarray(w.T).reshape(P, blk) for w in W], axis=1)          # the same for W^T
    shard, shard_t = torch.from_numpy(flat).to(dev), torch.from_numpy(flat_t).to(dev)
    outs = {k: [torch.zeros((P, w), dtype=torch.uint8, device=dev) for _ in range(count)]
            for k, w in (("rows", n), ("scales", n // 32), ("t_rows", n), ("t_scales", n // 32))}
    ptr = lambda k, i: outs[k][i].data_ptr()   # noqa: E731
    at = lambda buf, i: buf.data_ptr() + 4 * blk * i   # noqa: E731
    both = [(ptr("rows", i), n, ptr("scales", i), n // 32, ptr("t_rows", i), n, ptr("t_scales", i), n // 32, n, cols, at(shard, i), F)
            for i in range(count)]
    t_only = [(None, 0, None, 0) + b[4:] for b in both]
    rows_mx = [(ptr("rows", i), n, ptr("scales", i), n // 32, n, at(shard, i), F) for i in range(count)]
    t_mx = [(ptr("t_rows", i), n, ptr("t_scales", i), n // 32, n, at(shard_t, i), F) for i in range(count)]

    def rows_twice():
        plan.all_gather_shards_mxfp8(rows_mx, rceil=False, stream=s)
        plan.all_gather_shards_mxfp8(t_mx, rceil=False, stream=s)

    arms = {"both": lambda: plan.all_gather_shards_mxfp8_2d(both, rceil=False, stream=s),
            "t_only": lambda: plan.all_gather_shards_mxfp8_2d(t_only, rceil=False, stream=s),
            "rows_alone": lambda: plan.all_gather_shards_mxfp8(rows_mx, rceil=False, stream=s),
            "rows_twice": rows_twice}
    arms = {k: v for k, v in arms.items() if k in [ARMS[c] for c in which] or k == "both"}

    def zero():
        for v in outs.values():
            for x in v:
                x.zero_()

    def run_once(arm):
        with torch.cuda.stream(s):
            zero()
            arm()
        torch.cuda.synchronize()
        return {k: [x.clone() for x in v] for k, v in outs.items()}

    got = {k: run_once(a) for k, a in arms.items()}
    same = lambda x, y, keys: all(bool(torch.equal(p, q)) for k in keys for p, q in zip(x[k], y[k]))   # noqa: E731
    verified = {"both_vs_numpy": True, "shard_only_read": True}
    for i, w in enumerate(W):
        want = dict(zip(("rows", "scales"), mx2d_ref.expected_rows(w, P)))
        want.update(zip(("t_rows", "t_scales"), mx2d_ref.expected_t(w)))
        for k, v in want.items():
            g = got["both"][k][i]
            verified["both_vs_numpy"] &= bool(np.array_equal(g[0].cpu().numpy(), v)) and bool((g == g[0]).all())
    verified["shard_only_read"] = bool(np.array_equal(shard.cpu().numpy().view(np.uint32), flat.view(np.uint32)))
    if "t_only" in arms:
        verified["t_only_vs_both"] = same(got["t_only"], got["both"], ("t_rows", "t_scales")) and \
            all(not bool(x.any()) for k in ("rows", "scales") for x in got["t_only"][k])
    if "rows_alone" in arms:
        verified["rows_alone_vs_both"] = same(got["rows_alone"], got["both"], ("rows", "scales"))
    if "rows_twice" in arms:
        verified["rows_twice_vs_both"] = same(got["rows_twice"], got["both"], ("rows", "scales", "t_rows", "t_scales"))
    del got
    if not all(verified.values()):   # nothing is timed on wrong output
        return {"verified": False, "verified_per_arm": verified}

    def capture(arm):
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(CALLS):
                arm()
        torch.cuda.synchronize()
        return g

    def window(g):
        with torch.cuda.stream(s):
            zero()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            g.replay()
            e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    launches, kernels, grids = {}, {}, {}
    for k, a in arms.items():
        with t.launch_trace() as tr:
            with torch.cuda.stream(s):
                a()
        launches[k], kernels[k], grids[k] = tr.count, tr.kernels, tr.grids
    torch.cuda.synchronize()
    graphs = {k: capture(a) for k, a in arms.items()}
    for g in graphs.values():
        for _ in range(WARMUP):
            window(g)
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            us[k].append(sum(window(g) for _ in range(WINDOWS)) / (WINDOWS * CALLS))
    del graphs
    res = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
               "rounds_us": [round(x, 3) for x in v]} for k, v in us.items()}
    elems = count * n
    out = {"shape": {"buckets": count, "cols": cols, "nrows": nrows, "R": R, "elems_per_rank_per_bucket": n,
                     "flat_shard": f"{P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
           "algorithmic_bytes": {"shard_read_once": 4 * elems, "written_both": 2 * (P * elems + P * elems // 32),
                                 "written_one_orientation": P * elems + P * elems // 32, "shard_read_by_rows_twice": 8 * elems},
           "library_launches_per_call": launches, "kernels": kernels, "grids": grids, "arms": res,
           "verified": True, "verified_per_arm": verified}
    if "rows_twice" in res:
        out["both_median_at_or_below_rows_twice_min"] = res["both"]["median_us"] <= res["rows_twice"]["min_us"]
        out["rows_twice_over_both"] = round(res["rows_twice"]["median_us"] / res["both"]["median_us"], 3)
    if "rows_alone" in res:
        out["both_over_rows_alone"] = round(res["both"]["median_us"] / res["rows_alone"]["median_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx2d_all_gather.json"))
    ap.add_argument("--arms", default="abcd")
    ap.add_argument("--tag", default=None, help="the patch-shape A/B: print one line for this build, write no file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    shapes = {name: run_shape(name, plan, s, dev, rng, args.arms) for name in SHAPES}
    plan.close()
    ok = all(v["verified"] for v in shapes.values())
    if args.tag is not None:
        line = {"patch": args.tag, "verified": ok}
        for name, v in shapes.items():
            if v["verified"]:
                line[name] = {k: [a["median_us"], a["min_us"], a["max_us"]] for k, a in v["arms"].items()}
        print("AB " + json.dumps(line))
        return 0 if ok else 1
    out = {"algo": "swing", "side": SIDE, "ranks": P, "mode": "graph", "scale_rule": "floor", "rounds": ROUNDS,
           "calls_per_arm_per_round": WINDOWS * CALLS, "arm_names": ARMS, "shapes": shapes, "verified": ok,
           "unmeasured": ["eager calls", "the host cost of the checks", "the grid cap (inherited from kMaxGrid)"],
           "session": "one session on one MI355X"}
    if ok:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))
    print("verified" if ok else "NOT verified")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
