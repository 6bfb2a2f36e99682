"""Both MXFP4 orientations from one all-gather pass (Plan.all_gather_shards_mxfp4_2d) against the row-wise MXFP4
call and against the MXFP8 2D call, with the method of tools/mx2d_bench.py: 8x8 Swing, 64 ranks,
one rank-major flat fp32 buffer, one GPU, graphs of CALLS calls replayed (the device side alone), the floor scale
rule, arms alternated in one process.  Shapes: §21's three —
  buckets16   sixteen buckets of 2048 x 128 (R = 32): every strip of the new kernel spans FOUR shard blocks;
  one_large   one bucket of 2048 x 160 (R = 32);
  tall4       four buckets of 4096 x 128 (R = 64): a strip spans two shard blocks.
Arms:
  (a) both         the new call with both outputs
  (b) t_only       the new call column-wise only
  (c) rows_alone   all_gather_shards_mxfp4 alone: half the bytes, a floor, not a competitor
  (d) rows_twice   all_gather_shards_mxfp4 twice, the second time on a fp32 buffer that already holds W^T; making
                   that copy is NOT timed, and no user has one: the comparator flatters itself
  (e) mx8_both     all_gather_shards_mxfp8_2d, both outputs: patches of ONE shard block, twice the element bytes
  (f) mx8_t_only   all_gather_shards_mxfp8_2d, column-wise only
The claim "strips across shard blocks lift the R = 32 case" stands only if (b)'s MAXIMUM over the rounds is below
(f)'s MINIMUM on both R = 32 shapes; what was measured is written down either way.  Before anything is timed every
arm's outputs are verified bit for bit: (a) against tests/mx4_2d_ref.py (rank 0's rows on the host, every other
rank's against rank 0's on the device), (b), (c), (d) against (a); (e) against tests/mx2d_ref.py, (f) against (e).
The outputs are zeroed before every window, outside the events.  Eager calls, the host cost of the checks and the
grid cap (inherited from kMaxGrid) are not measured.  --tag NAME: the strip A/B, one build per process
(ALLRED_LIB_PATH), printing one line.  Writes one JSON (default profiles/mx4_2d_all_gather.json) and prints it."""
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

import mx2d_ref  # noqa: E402  (tests/: the MXFP8 expectation)
import mx4_2d_ref  # noqa: E402  (tests/: the MXFP4 expectation)
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
SHAPES = {"buckets16": (16, 128, 32), "one_large": (1, 160, 32), "tall4": (4, 128, 64)}   # buckets, cols, R
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
KEYS = ("rows", "scales", "t_rows", "t_scales")


def run_shape(name, plan, s, dev, rng):
    count, cols, R = SHAPES[name]
    nrows = P * R
    n, blk = nrows * cols, R * cols
    F = count * blk
    W = [rng.standard_normal((nrows, cols)).astype(np.float32) * np.exp2(rng.integers(-8, 8, (nrows, 1))).astype(np.float32)
         for _ in range(count)]
    flat = np.concatenate([w.reshape(P, blk) for w in W], axis=1)                                   # (P, F): bucket i at column blk i
    flat_t = np.concatenate([np.ascontiguousarray(w.T).reshape(P, blk) for w in W], axis=1)        # the same for W^T
    shard, shard_t = torch.from_numpy(flat).to(dev), torch.from_numpy(flat_t).to(dev)
    at = lambda buf, i: buf.data_ptr() + 4 * blk * i   # noqa: E731

    def outputs(payload):
        o = {k: [torch.zeros((P, w), dtype=torch.uint8, device=dev) for _ in range(count)]
             for k, w in zip(KEYS, (payload, n // 32, payload, n // 32))}
        ptr = lambda k, i: o[k][i].data_ptr()   # noqa: E731
        both = [(ptr("rows", i), payload, ptr("scales", i), n // 32, ptr("t_rows", i), payload, ptr("t_scales", i), n // 32, n, cols,
                 at(shard, i), F) for i in range(count)]
        rows_mx = [(ptr("rows", i), payload, ptr("scales", i), n // 32, n, at(shard, i), F) for i in range(count)]
        t_mx = [(ptr("t_rows", i), payload, ptr("t_scales", i), n // 32, n, at(shard_t, i), F) for i in range(count)]
        return o, both, [(None, 0, None, 0) + b[4:] for b in both], rows_mx, t_mx

    o4, both4, t4, rows4, tmx4 = outputs(n // 2)
    o8, both8, t8, _, _ = outputs(n)

    def rows_twice():
        plan.all_gather_shards_mxfp4(rows4, rceil=False, stream=s)
        plan.all_gather_shards_mxfp4(tmx4, rceil=False, stream=s)

    arms = {"both": (o4, lambda: plan.all_gather_shards_mxfp4_2d(both4, rceil=False, stream=s)),
            "t_only": (o4, lambda: plan.all_gather_shards_mxfp4_2d(t4, rceil=False, stream=s)),
            "rows_alone": (o4, lambda: plan.all_gather_shards_mxfp4(rows4, rceil=False, stream=s)),
            "rows_twice": (o4, rows_twice),
            "mx8_both": (o8, lambda: plan.all_gather_shards_mxfp8_2d(both8, rceil=False, stream=s)),
            "mx8_t_only": (o8, lambda: plan.all_gather_shards_mxfp8_2d(t8, rceil=False, stream=s))}

    def zero():
        for o in (o4, o8):
            for v in o.values():
                for x in v:
                    x.zero_()

    def run_once(o, arm):
        with torch.cuda.stream(s):
            zero()
            arm()
        torch.cuda.synchronize()
        return {k: [x.clone() for x in v] for k, v in o.items()}

    got = {k: run_once(*a) for k, a in arms.items()}
    same = lambda x, y, keys: all(bool(torch.equal(p, q)) for k in keys for p, q in zip(x[k], y[k]))   # noqa: E731
    untouched = lambda x, keys: all(not bool(v.any()) for k in keys for v in x[k])   # noqa: E731
    verified = {"both_vs_numpy": True, "mx8_both_vs_numpy": True}
    for i, w in enumerate(W):
        for arm, want in (("both", mx4_2d_ref.expected(w, P)), ("mx8_both", mx2d_ref.expected_rows(w, P) + mx2d_ref.expected_t(w))):
            for k, v in zip(KEYS, want):
                g = got[arm][k][i]
                verified[arm + "_vs_numpy"] &= bool(np.array_equal(g[0].cpu().numpy(), v)) and bool((g == g[0]).all())
    verified["shard_only_read"] = bool(np.array_equal(shard.cpu().numpy().view(np.uint32), flat.view(np.uint32)))
    verified["t_only_vs_both"] = same(got["t_only"], got["both"], KEYS[2:]) and untouched(got["t_only"], KEYS[:2])
    verified["rows_alone_vs_both"] = same(got["rows_alone"], got["both"], KEYS[:2])
    verified["rows_twice_vs_both"] = same(got["rows_twice"], got["both"], KEYS)
    verified["mx8_t_only_vs_mx8_both"] = same(got["mx8_t_only"], got["mx8_both"], KEYS[2:]) and untouched(got["mx8_t_only"], KEYS[:2])
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

    kernels, grids = {}, {}
    for k, (_, a) in arms.items():
        with t.launch_trace() as tr:
            with torch.cuda.stream(s):
                a()
        kernels[k], grids[k] = tr.kernels, tr.grids
    torch.cuda.synchronize()
    graphs = {k: capture(a) for k, (_, a) in arms.items()}
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
    one4, one8 = P * elems // 2 + P * elems // 32, P * elems + P * elems // 32
    return {"shape": {"buckets": count, "cols": cols, "nrows": nrows, "R": R, "elems_per_rank_per_bucket": n,
                      "flat_shard": f"{P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
            "bytes_written": {"both": 2 * one4, "t_only": one4, "rows_alone": one4, "rows_twice": 2 * one4, "mx8_both": 2 * one8,
                              "mx8_t_only": one8},
            "shard_bytes_read": {k: (8 if k == "rows_twice" else 4) * elems for k in arms},
            "kernels": kernels, "grids": grids, "arms": res, "verified": True, "verified_per_arm": verified,
            "t_only_max_below_mx8_t_only_min": res["t_only"]["max_us"] < res["mx8_t_only"]["min_us"],
            "both_median_at_or_below_rows_twice_min": res["both"]["median_us"] <= res["rows_twice"]["min_us"],
            "mx8_t_only_over_t_only": round(res["mx8_t_only"]["median_us"] / res["t_only"]["median_us"], 3),
            "both_over_rows_alone": round(res["both"]["median_us"] / res["rows_alone"]["median_us"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx4_2d_all_gather.json"))
    ap.add_argument("--tag", default=None, help="the strip A/B: print one line for this build, write no file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    shapes = {name: run_shape(name, plan, s, dev, rng) for name in SHAPES}
    plan.close()
    ok = all(v["verified"] for v in shapes.values())
    if args.tag is not None:
        line = {"strip": args.tag, "verified": ok}
        for name, v in shapes.items():
            if v["verified"]:
                line[name] = {k: [a["median_us"], a["min_us"], a["max_us"]] for k, a in v["arms"].items()}
        print("AB " + json.dumps(line))
        return 0 if ok else 1
    out = {"algo": "swing", "side": SIDE, "ranks": P, "mode": "graph", "scale_rule": "floor", "rounds": ROUNDS,
           "calls_per_arm_per_round": WINDOWS * CALLS, "shapes": shapes, "verified": ok,
           "strips_lift_R32": ok and all(shapes[k]["t_only_max_below_mx8_t_only_min"] for k in ("buckets16", "one_large")),
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
