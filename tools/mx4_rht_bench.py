"""What the random Hadamard rotation costs inside the two 1D MXFP4 calls (Plan.all_gather_shards_mxfp4_rht,
Plan.adamw_all_gather_shards_mxfp4_rht) over their unrotated twins, with the method of tools/adamw_mx4_bench.py
 unchanged: 8x8 Swing, 64 ranks, rank-major flat fp32 planes, one GPU, replayed from a HIP graph of
CALLS calls (the device side alone), the arms alternated in one process, median [min - max] over the rounds.  The
README's two shapes:
  buckets16   sixteen buckets of 64 tiles (16,384 elements per rank), one tile per block;
  one_large   one bucket of 327,680 elements per rank (1280 tiles, 20 per block).
Arms (the floor scale rule, sign_mask 0x9E3779B9):
  mx4 / mx4_rht               all_gather_shards_mxfp4 / all_gather_shards_mxfp4_rht from the param plane
  adamw_mx4 / adamw_mx4_rht   adamw_all_gather_shards_mxfp4 / its rotated form, two parameter groups, clipping active
No ratio is a pass condition; whether a rotated arm's median lies above its twin's MAXIMUM is recorded.

Before anything is timed, from pristine buffers: mx4_rht's rows and scales are BIT-equal to tests/mxfp4_rht_ref.py's
expectation; adamw_mx4_rht's planes and info are bit-equal to adamw_mx4's, its rows and scales to mx4_rht's run on the
param plane it leaves.  Not measured: the pass the rotation replaces (a rotation kernel over the masters before the
call, or over every rank's rows after it), eager calls, the host cost of the checks.  Writes one JSON (default
profiles/mx4_rht_all_gather.json, --out PATH) and prints it."""
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

import mxfp4_rht_ref  # noqa: E402  (tests/mxfp4_rht_ref.py: the rotated rows)
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
SHAPES = {"buckets16": (16, 64), "one_large": (1, 1280)}   # buckets, tiles per rank row
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
STEP, MAX_NORM, MASK = 3, 1.0, 0x9E3779B9
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]
NAMES = ("param", "grad", "exp_avg", "exp_avg_sq")
PAIRS = (("mx4", "mx4_rht"), ("adamw_mx4", "adamw_mx4_rht"))


def run_shape(name, plan, s, dev, rng):
    count, tiles = SHAPES[name]
    n = 256 * tiles
    blk = n // P
    F = count * blk
    rows4 = [torch.zeros((P, n // 2), dtype=torch.uint8, device=dev) for _ in range(count)]
    scales = [torch.zeros((P, n // 32), dtype=torch.uint8, device=dev) for _ in range(count)]
    host = {"param": rng.standard_normal((P, F)).astype(np.float32), "grad": rng.standard_normal((P, F)).astype(np.float32),
            "exp_avg": (rng.standard_normal((P, F)) * 1e-2).astype(np.float32),
            "exp_avg_sq": (1e-4 * (0.25 + rng.random((P, F)))).astype(np.float32)}
    pristine = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    plane = {k: v.clone() for k, v in pristine.items()}
    at = lambda k, i: plane[k].data_ptr() + 4 * blk * i   # noqa: E731
    out = lambda i: (rows4[i].data_ptr(), n // 2, scales[i].data_ptr(), n // 32, n)   # noqa: E731
    adamw_list = [out(i) + tuple(at(k, i) for k in NAMES) + (F,) for i in range(count)]
    ag_list = [out(i) + (at("param", i), F) for i in range(count)]
    group_of = [i % 2 for i in range(count)]
    norm_sq = torch.from_numpy((host["grad"].astype(np.float64) ** 2).sum(axis=1).astype(np.float32)).to(dev)
    hyper = torch.from_numpy(t.adamw_hyper_groups(GROUPS, step=STEP, max_norm=MAX_NORM)).to(dev)
    info = torch.zeros(4, dtype=torch.float32, device=dev)
    small = (group_of, hyper.data_ptr(), 2)
    arms = {"mx4": lambda: plan.all_gather_shards_mxfp4(ag_list, stream=s),
            "mx4_rht": lambda: plan.all_gather_shards_mxfp4_rht(ag_list, MASK, stream=s),
            "adamw_mx4": lambda: plan.adamw_all_gather_shards_mxfp4(adamw_list, *small, norm_sq.data_ptr(), info.data_ptr(), stream=s),
            "adamw_mx4_rht": lambda: plan.adamw_all_gather_shards_mxfp4_rht(adamw_list, *small, MASK, norm_sq.data_ptr(), info.data_ptr(),
                                                                           stream=s)}

    def restore():
        for k in plane:
            plane[k].copy_(pristine[k])

    def run_once(*calls):
        with torch.cuda.stream(s):
            restore()
            info.zero_()
            for r in rows4 + scales:
                r.zero_()
            for call in calls:
                call()
        torch.cuda.synchronize()
        return {"planes": [plane[k].cpu().numpy().view(np.uint32).copy() for k in NAMES], "info": info.cpu().numpy().view(np.uint32).copy(),
                "rows4": np.stack([r.cpu().numpy() for r in rows4]), "scales": np.stack([r.cpu().numpy() for r in scales])}

    def same(a, b, keys):
        return {k: all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) if k == "planes" else bool(np.array_equal(a[k], b[k])) for k in keys}

    got = run_once(arms["mx4_rht"])
    want = [mxfp4_rht_ref.expected_rows(host["param"][:, i * blk:(i + 1) * blk], MASK) for i in range(count)]
    verified = {"mx4_rht_vs_numpy": {"rows4": all(np.array_equal(got["rows4"][i], np.broadcast_to(w[0], (P, n // 2))) for i, w in enumerate(want)),
                                     "scales": all(np.array_equal(got["scales"][i], np.broadcast_to(w[1], (P, n // 32))) for i, w in enumerate(want))}}
    rht, twin = run_once(arms["adamw_mx4_rht"]), run_once(arms["adamw_mx4"])
    verified["adamw_mx4_rht_vs_adamw_mx4"] = same(rht, twin, ("planes", "info"))
    verified["adamw_mx4_rht_vs_mx4_rht_on_its_param_plane"] = same(rht, run_once(arms["adamw_mx4"], arms["mx4_rht"]), ("rows4", "scales"))
    verified["rotated_rows_differ_from_the_twin's"] = {"rows4": not np.array_equal(rht["rows4"], twin["rows4"])}
    if not all(all(v.values()) for v in verified.values()):   # nothing is timed on wrong output
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
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            g.replay()
            e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    kernels = {}
    for k, a in arms.items():
        with t.launch_trace() as tr:
            with torch.cuda.stream(s):
                a()
        kernels[k] = tr.kernels
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
    cost = {b: {"minus_twin_us": round(res[b]["median_us"] - res[a]["median_us"], 3), "over_twin": round(res[b]["median_us"] / res[a]["median_us"], 3),
                "median_above_twin_max": res[b]["median_us"] > res[a]["max_us"]} for a, b in PAIRS}
    return {"shape": {"buckets": count, "tiles_per_rank": tiles, "elems_per_rank_per_bucket": n}, "kernels": kernels, "arms": res,
            "rotation_cost": cost, "verified": True, "verified_per_arm": verified}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx4_rht_all_gather.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    shapes = {name: run_shape(name, plan, s, dev, rng) for name in SHAPES}
    plan.close()
    ok = all(v["verified"] for v in shapes.values())
    out = {"algo": "swing", "side": SIDE, "ranks": P, "mode": "graph", "groups": GROUPS, "step": STEP, "max_norm": MAX_NORM,
           "scale_rule": "floor", "sign_mask": hex(MASK), "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS, "shapes": shapes,
           "verified": ok,
           "unmeasured": ["the pass the rotation replaces: a rotation kernel over the fp32 masters before the call, or over every rank's rows after it",
                          "eager calls and the host cost of the checks", "the grid cap (inherited from the grouped all-gather's)"],
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
