"""What stochastic rounding costs inside the two 1D MXFP4 calls (Plan.all_gather_shards_mxfp4_sr,
Plan.adamw_all_gather_shards_mxfp4_sr) over their round-to-nearest twins, unrotated and rotated, with the method of
tools/mx4_rht_bench.py unchanged: 8x8 Swing, 64 ranks, rank-major flat fp32 planes, one GPU, replayed
from a HIP graph of CALLS calls (the device side alone), the arms alternated in one process, median [min - max] over the
rounds.  The README's two shapes:
  buckets16   sixteen buckets of 64 tiles (16,384 elements per rank), one tile per block;
  one_large   one bucket of 327,680 elements per rank (1280 tiles, 20 per block).
Arms (the RCEIL scale rule — the one under which SR is unbiased —, sign_mask 0x9E3779B9), each SR arm next to its twin:
  mx4 / mx4_sr                      all_gather_shards_mxfp4 / all_gather_shards_mxfp4_sr from the param plane
  mx4_rht / mx4_sr_rht              the same, rotated
  adamw_mx4 / adamw_mx4_sr          adamw_all_gather_shards_mxfp4 / its SR form, two parameter groups, clipping active
  adamw_mx4_rht / adamw_mx4_sr_rht  the same, rotated
No ratio is a pass condition; whether an SR arm's median lies above its twin's MAXIMUM is recorded.

Before anything is timed, from pristine buffers: both mx4_sr arms' rows and scales are BIT-equal to t.mxfp4_sr_quantize;
both adamw SR arms' planes and info are bit-equal to adamw_mx4's, their rows and scales to the plain SR arm's run on the
param plane they leave.  Not an arm, and not measured: the pass SR replaces (an SR quantisation kernel over every rank's
gathered copy, with its RNG kept in step across ranks), eager calls, the host cost of the checks.  Writes one JSON
(default profiles/mx4_sr_all_gather.json, --out PATH) and prints it."""
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
SHAPES = {"buckets16": (16, 64), "one_large": (1, 1280)}   # buckets, tiles per rank row
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
STEP, MAX_NORM, MASK = 3, 1.0, 0x9E3779B9
SEED, SR_STEP = 0x5EED0123456789AB, 17
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]
NAMES = ("param", "grad", "exp_avg", "exp_avg_sq")
PAIRS = (("mx4", "mx4_sr"), ("mx4_rht", "mx4_sr_rht"), ("adamw_mx4", "adamw_mx4_sr"), ("adamw_mx4_rht", "adamw_mx4_sr_rht"))


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
    sr = torch.from_numpy(np.array([SEED & 0xFFFFFFFF, SEED >> 32, SR_STEP, 0], dtype=np.uint32).view(np.int32)).to(dev)
    small = (group_of, hyper.data_ptr(), 2)
    tail = dict(norm_sq_ptr=norm_sq.data_ptr(), info_ptr=info.data_ptr(), rceil=True, stream=s)
    arms = {"mx4": lambda: plan.all_gather_shards_mxfp4(ag_list, rceil=True, stream=s),
            "mx4_sr": lambda: plan.all_gather_shards_mxfp4_sr(ag_list, sr.data_ptr(), rceil=True, stream=s),
            "mx4_rht": lambda: plan.all_gather_shards_mxfp4_rht(ag_list, MASK, rceil=True, stream=s),
            "mx4_sr_rht": lambda: plan.all_gather_shards_mxfp4_sr(ag_list, sr.data_ptr(), sign_mask=MASK, rceil=True, stream=s),
            "adamw_mx4": lambda: plan.adamw_all_gather_shards_mxfp4(adamw_list, *small, **tail),
            "adamw_mx4_sr": lambda: plan.adamw_all_gather_shards_mxfp4_sr(adamw_list, *small, sr.data_ptr(), **tail),
            "adamw_mx4_rht": lambda: plan.adamw_all_gather_shards_mxfp4_rht(adamw_list, *small, MASK, **tail),
            "adamw_mx4_sr_rht": lambda: plan.adamw_all_gather_shards_mxfp4_sr(adamw_list, *small, sr.data_ptr(), MASK, **tail)}

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

    verified = {}
    for arm, mask in (("mx4_sr", None), ("mx4_sr_rht", MASK)):
        got = run_once(arms[arm])
        want = [t.mxfp4_sr_quantize(host["param"][:, i * blk:(i + 1) * blk].reshape(-1), SEED, SR_STEP, i, rceil=True, sign_mask=mask)
                for i in range(count)]
        verified[arm + "_vs_numpy"] = {"rows4": all(np.array_equal(got["rows4"][i], np.broadcast_to(w[0], (P, n // 2))) for i, w in enumerate(want)),
                                       "scales": all(np.array_equal(got["scales"][i], np.broadcast_to(w[1], (P, n // 32))) for i, w in enumerate(want))}
    twin = run_once(arms["adamw_mx4"])
    for arm, plain in (("adamw_mx4_sr", "mx4_sr"), ("adamw_mx4_sr_rht", "mx4_sr_rht")):
        got = run_once(arms[arm])
        verified[arm + "_vs_adamw_mx4"] = same(got, twin, ("planes", "info"))
        verified[arm + "_vs_" + plain + "_on_its_param_plane"] = same(got, run_once(arms["adamw_mx4"], arms[plain]), ("rows4", "scales"))
        verified[arm + "_rows_differ_from_the_rne_call's"] = {"rows4": not np.array_equal(got["rows4"], twin["rows4"])}
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
    cost = {b: {"twin": a, "minus_twin_us": round(res[b]["median_us"] - res[a]["median_us"], 3),
                "over_twin": round(res[b]["median_us"] / res[a]["median_us"], 3),
                "median_above_twin_max": res[b]["median_us"] > res[a]["max_us"]} for a, b in PAIRS}
    return {"shape": {"buckets": count, "tiles_per_rank": tiles, "elems_per_rank_per_bucket": n}, "kernels": kernels, "arms": res,
            "sr_cost": cost, "verified": True, "verified_per_arm": verified}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx4_sr_all_gather.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    shapes = {name: run_shape(name, plan, s, dev, rng) for name in SHAPES}
    plan.close()
    ok = all(v["verified"] for v in shapes.values())
    out = {"algo": "swing", "side": SIDE, "ranks": P, "mode": "graph", "groups": GROUPS, "step": STEP, "max_norm": MAX_NORM,
           "scale_rule": "rceil", "sign_mask": hex(MASK), "sr_state": {"seed": hex(SEED), "step": SR_STEP}, "rounds": ROUNDS,
           "calls_per_arm_per_round": WINDOWS * CALLS, "shapes": shapes, "verified": ok,
           "unmeasured": ["the pass SR replaces (not an arm): an SR quantisation kernel over every rank's gathered copy, its RNG kept in step across ranks",
                          "eager calls and the host cost of the checks", "the grid cap (inherited from the grouped all-gather's)",
                          "v_cvt_scalef32_sr_pk_fp4_f32 in place of the integer rule"],
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
