"""The 2D MXFP4 all-gather with stochastically rounded (and rotated) column-wise rows
(Plan.all_gather_shards_mxfp4_2d_sr) against its RNE twin and against the route it replaces, with the method of
tools/mx4_2d_bench.py: 8x8 Swing, 64 ranks, one rank-major flat fp32 buffer, one GPU, graphs of CALLS calls replayed
(the device side alone), the RCEIL scale rule, arms alternated in one process.  Shapes: that tool's three —
  buckets16   sixteen buckets of 2048 x 128 (R = 32);
  one_large   one bucket of 2048 x 160 (R = 32);
  tall4       four buckets of 4096 x 128 (R = 64).
Arms, each `_both` (all four outputs) and `_t` (column-wise only):
  sr       the new call, no rotation
  srrot    the new call with the rotation
  rne      all_gather_shards_mxfp4_2d: the RNE twin — what SR, and SR with the rotation, cost on top of it
  route_sr / route_srrot   what a user had to do before: all_gather_shards_mxfp4_sr on a fp32 buffer that already
           holds W^T (`_both`: plus all_gather_shards_mxfp4 for the rows).  Making that transposed copy is NOT timed
           and is NOT in the comparison, and no user has one: the comparator flatters itself.
No threshold is set: per arm median [min - max] over the rounds, and for every pair whether the two ranges overlap.
Before anything is timed every arm is verified bit for bit: sr / srrot t rows against t.mxfp4_sr_quantize on W^T
(rank 0 on the host, every other rank against rank 0 on the device), their rows and rne against tests/mx4_2d_ref.py,
`_t` arms against `_both` with untouched rows, and the route's outputs against the new call's — the contract, GPU
against GPU.  The outputs are zeroed before every window, outside the events.  Eager calls, the host cost of the
checks, the floor rule and the grid cap (inherited from kMaxGrid) are not measured.  Writes one JSON (default
profiles/mx4_2d_sr_all_gather.json) and prints it."""
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

import mx4_2d_ref  # noqa: E402  (tests/: the RNE expectation)
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
SHAPES = {"buckets16": (16, 128, 32), "one_large": (1, 160, 32), "tall4": (4, 128, 64)}   # buckets, cols, R
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
KEYS = ("rows", "scales", "t_rows", "t_scales")
MASK, SEED, STEP = 0x9E3779B9, 0xC0FFEE0123456789, 7
PAIRS = [(new + out, old + out) for out in ("_both", "_t") for new in ("sr", "srrot") for old in ("rne", "route_" + new)]


def run_shape(name, plan, s, dev, rng, sr):
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
    o = {k: [torch.zeros((P, w), dtype=torch.uint8, device=dev) for _ in range(count)] for k, w in zip(KEYS, (n // 2, n // 32, n // 2, n // 32))}
    ptr = lambda k, i: o[k][i].data_ptr()   # noqa: E731
    both = [(ptr("rows", i), n // 2, ptr("scales", i), n // 32, ptr("t_rows", i), n // 2, ptr("t_scales", i), n // 32, n, cols, at(shard, i), F)
            for i in range(count)]
    t_only = [(None, 0, None, 0) + b[4:] for b in both]
    rows_mx = [(ptr("rows", i), n // 2, ptr("scales", i), n // 32, n, at(shard, i), F) for i in range(count)]
    t_mx = [(ptr("t_rows", i), n // 2, ptr("t_scales", i), n // 32, n, at(shard_t, i), F) for i in range(count)]

    def new(lst, mask):
        return lambda: plan.all_gather_shards_mxfp4_2d_sr(lst, sr.data_ptr(), sign_mask=mask, rceil=True, stream=s)

    def route(mask, rows):
        def run():
            if rows:
                plan.all_gather_shards_mxfp4(rows_mx, rceil=True, stream=s)
            plan.all_gather_shards_mxfp4_sr(t_mx, sr.data_ptr(), sign_mask=mask, rceil=True, stream=s)
        return run

    arms = {"sr_both": new(both, None), "sr_t": new(t_only, None), "srrot_both": new(both, MASK), "srrot_t": new(t_only, MASK),
            "rne_both": lambda: plan.all_gather_shards_mxfp4_2d(both, rceil=True, stream=s),
            "rne_t": lambda: plan.all_gather_shards_mxfp4_2d(t_only, rceil=True, stream=s),
            "route_sr_both": route(None, True), "route_sr_t": route(None, False),
            "route_srrot_both": route(MASK, True), "route_srrot_t": route(MASK, False)}

    def zero():
        for v in o.values():
            for x in v:
                x.zero_()

    def run_once(arm):
        with torch.cuda.stream(s):
            zero()
            arm()
        torch.cuda.synchronize()
        return {k: [x.clone() for x in v] for k, v in o.items()}

    got = {k: run_once(a) for k, a in arms.items()}
    same = lambda x, y, keys: all(bool(torch.equal(p, q)) for k in keys for p, q in zip(x[k], y[k]))   # noqa: E731
    untouched = lambda x, keys: all(not bool(v.any()) for k in keys for v in x[k])   # noqa: E731
    verified = {"sr_both_vs_numpy": True, "srrot_both_vs_numpy": True, "rne_both_vs_numpy": True}
    for i, w in enumerate(W):
        rne = mx4_2d_ref.expected(w, P, True)
        for arm, mask in (("sr_both", None), ("srrot_both", MASK), ("rne_both", 0)):
            want = rne if arm == "rne_both" else rne[:2] + t.mxfp4_sr_quantize(np.ascontiguousarray(w.T).reshape(-1), SEED, STEP, i, rceil=True,
                                                                               sign_mask=mask)
            for k, v in zip(KEYS, want):
                g = got[arm][k][i]
                verified[arm + "_vs_numpy"] &= bool(np.array_equal(g[0].cpu().numpy(), v)) and bool((g == g[0]).all())
    verified["shard_only_read"] = bool(np.array_equal(shard.cpu().numpy().view(np.uint32), flat.view(np.uint32)))
    for a in ("sr", "srrot", "rne"):
        verified[f"{a}_t_vs_{a}_both"] = same(got[a + "_t"], got[a + "_both"], KEYS[2:]) and untouched(got[a + "_t"], KEYS[:2])
    for a in ("sr", "srrot"):
        verified[f"route_{a}_both_vs_{a}_both"] = same(got[f"route_{a}_both"], got[a + "_both"], KEYS)
        verified[f"route_{a}_t_vs_{a}_both"] = same(got[f"route_{a}_t"], got[a + "_both"], KEYS[2:]) and untouched(got[f"route_{a}_t"], KEYS[:2])
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
    for k, a in arms.items():
        with t.launch_trace() as tr:
            with torch.cuda.stream(s):
                a()
        kernels[k], grids[k] = tr.kernels, tr.grids
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
    pairs = {}
    for a, b in PAIRS:
        x, y = res[a], res[b]
        pairs[f"{a}_vs_{b}"] = {"ratio_of_medians": round(x["median_us"] / y["median_us"], 3),
                                "ranges_overlap": not (x["max_us"] < y["min_us"] or y["max_us"] < x["min_us"])}
    elems = count * n
    one = P * elems // 2 + P * elems // 32
    return {"shape": {"buckets": count, "cols": cols, "nrows": nrows, "R": R, "elems_per_rank_per_bucket": n,
                      "flat_shard": f"{P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
            "bytes_written": {k: (2 if k.endswith("_both") else 1) * one for k in arms},
            "shard_bytes_read": {k: (8 if k.startswith("route_") and k.endswith("_both") else 4) * elems for k in arms},
            "kernels": kernels, "grids": grids, "arms": res, "pairs": pairs, "verified": True, "verified_per_arm": verified}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx4_2d_sr_all_gather.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    sr = torch.from_numpy(np.array([SEED & 0xFFFFFFFF, SEED >> 32, STEP, 0], dtype=np.uint32).view(np.int32)).to(dev)
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    shapes = {name: run_shape(name, plan, s, dev, rng, sr) for name in SHAPES}
    plan.close()
    ok = all(v["verified"] for v in shapes.values())
    out = {"algo": "swing", "side": SIDE, "ranks": P, "mode": "graph", "scale_rule": "rceil", "rounds": ROUNDS,
           "calls_per_arm_per_round": WINDOWS * CALLS, "shapes": shapes, "verified": ok,
           "not_in_the_comparison": "the route's fp32 W^T is prepared outside the timing",
           "unmeasured": ["eager calls", "the host cost of the checks", "the floor scale rule", "the grid cap (inherited from kMaxGrid)",
                          "the transposed fp32 copy the route needs"],
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
