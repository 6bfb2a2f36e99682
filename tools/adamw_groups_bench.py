"""AdamW parameter groups in one launch (Plan.adamw_all_gather_shards_f32_groups) against one call of
the existing entry point per group, with the method of tools/adamw_shard_bench.py
unchanged: 8x8 Swing, 64 ranks, sixteen buckets of 32 kB per rank (64 tiles, one tile per block), FOUR
rank-major flat fp32 planes (64 rows of F = 16 x 256 floats; bucket i at column 256 i,
shard_stride = F), one GPU, replayed from a HIP graph (the device side alone).

Arms, alternated in one process:
  (a) groups_2     the new call, two parameter groups alternating bucket by bucket          one launch
  (b) two_calls    the parent's way: adamw_all_gather_shards_f32 twice, the eight buckets of
                   each group with that group's set, in one graph                          two launches
  (c) one_call     adamw_all_gather_shards_f32 on all sixteen buckets, one set              one launch
  (d) groups_1     the new call with ngroups = 1 (group_of = NULL)                          one launch
(d) against (c) is what the per-tile lookup costs.  The expectation, not a bar: (a) near (c) and well
under (b); what the feature has to show is (a)'s median below (b)'s minimum.  What was measured is
written down either way.

Before anything is timed, from pristine buffers: (a)'s four planes and every rank row are BIT-equal
to tests/adamw_ref.py's numpy step with each bucket's group (max_norm: group 0's; the gradient norm
here is about 512, so max_norm = 1 clips); (b)'s buffers are bit-equal to (a)'s and (d)'s to (c)'s.  A
round times each arm over WINDOWS replays of a graph of CALLS calls between device events; the
pristine buffers are restored before every window, outside the events.  Eager calls and the host
cost of the checks are not measured.  Writes one JSON (default profiles/adamw_param_groups.json,
--out PATH) and prints it."""
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

import adamw_ref  # noqa: E402  (tests/adamw_ref.py: the expectation)
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
BUCKETS, TILES = 16, 64
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
STEP, MAX_NORM = 3, 1.0
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),     # the weights
          dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]      # biases and norm weights: no decay, an lr of their own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_param_groups.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    n = 256 * TILES
    blk = n // P
    stride = t.preferred_rank_stride(n)
    F = BUCKETS * blk
    param_rows = [torch.zeros((P, stride), dtype=torch.int16, device=dev) for _ in range(BUCKETS)]
    host = {"param": rng.standard_normal((P, F)).astype(np.float32), "grad": rng.standard_normal((P, F)).astype(np.float32),
            "exp_avg": (rng.standard_normal((P, F)) * 1e-2).astype(np.float32),
            "exp_avg_sq": (1e-4 * (0.25 + rng.random((P, F)))).astype(np.float32)}   # away from 0: no huge m / sqrt(v)
    NAMES = ("param", "grad", "exp_avg", "exp_avg_sq")
    pristine = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    plane = {k: v.clone() for k, v in pristine.items()}
    at = lambda k, i: plane[k].data_ptr() + 4 * blk * i   # noqa: E731
    buckets = [(param_rows[i].data_ptr(), stride, n) + tuple(at(k, i) for k in NAMES) + (F,) for i in range(BUCKETS)]
    group_of = [i % 2 for i in range(BUCKETS)]
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    norm_sq_host = (host["grad"].astype(np.float64) ** 2).sum(axis=1).astype(np.float32)   # per rank, of the pristine gradient
    norm_sq = torch.from_numpy(norm_sq_host).to(dev)
    hyper_host = t.adamw_hyper_groups(GROUPS, step=STEP, max_norm=MAX_NORM)   # (2, 8): max_norm in every row, so row g is eff(g)
    hyper = torch.from_numpy(hyper_host).to(dev)                                # the array of (a), its row 0 the set of (c) and (d)
    hyper_1 = torch.from_numpy(hyper_host[1].copy()).to(dev)                    # group 1's set for (b)'s second call
    info = torch.zeros(4, dtype=torch.float32, device=dev)
    subs = [[b for b, g in zip(buckets, group_of) if g == k] for k in range(2)]

    def restore():
        for k in plane:
            plane[k].copy_(pristine[k])

    def groups_2():
        plan.adamw_all_gather_shards_f32_groups(buckets, group_of, hyper.data_ptr(), 2, norm_sq.data_ptr(), info.data_ptr(), stream=s)

    def two_calls():
        plan.adamw_all_gather_shards_f32(subs[0], hyper.data_ptr(), norm_sq.data_ptr(), info.data_ptr(), stream=s)
        plan.adamw_all_gather_shards_f32(subs[1], hyper_1.data_ptr(), norm_sq.data_ptr(), info.data_ptr(), stream=s)

    def one_call():
        plan.adamw_all_gather_shards_f32(buckets, hyper.data_ptr(), norm_sq.data_ptr(), info.data_ptr(), stream=s)

    def groups_1():
        plan.adamw_all_gather_shards_f32_groups(buckets, None, hyper.data_ptr(), 1, norm_sq.data_ptr(), info.data_ptr(), stream=s)

    arms = {"groups_2": groups_2, "two_calls": two_calls, "one_call": one_call, "groups_1": groups_1}

    def run_once(arm):
        with torch.cuda.stream(s):
            restore()
            info.zero_()
            for r in param_rows:
                r.zero_()
            arm()
        torch.cuda.synchronize()
        return ({k: plane[k].cpu().numpy().view(np.uint32).copy() for k in NAMES},
                torch.stack([r[:, :n] for r in param_rows]).cpu().numpy().view(np.uint16).copy(), info.cpu().numpy().view(np.uint32).copy())

    def expected(groups_of_buckets):
        """tests/adamw_ref.py's step, bucket by bucket, each with its group's row of hyper_host"""
        want = {k: host[k].view(np.uint32).copy() for k in NAMES}
        rows = np.zeros((BUCKETS, P, n), dtype=np.uint16)
        inf = None
        for i, g in enumerate(groups_of_buckets):
            col = slice(i * blk, (i + 1) * blk)
            new, r16, inf_g = adamw_ref.step(*(host[k][:, col] for k in NAMES), hyper_host[g], norm_sq_host, P, False)
            for k, v in zip(NAMES, new):
                want[k][:, col] = np.ascontiguousarray(v).view(np.uint32)
            rows[i] = np.ascontiguousarray(r16).reshape(-1)[None, :]   # block b of EVERY rank row
            inf = inf_g if g == 0 or inf is None else inf
        return want, rows, inf.view(np.uint32)

    def bit_equal(got, want):
        return {"planes": {k: bool(np.array_equal(got[0][k], want[0][k])) for k in NAMES}, "rows": bool(np.array_equal(got[1], want[1])),
                "info": bool(np.array_equal(got[2], want[2]))}

    got = {k: run_once(a) for k, a in arms.items()}
    verified = {"groups_2_vs_adamw_ref": bit_equal(got["groups_2"], expected(group_of)),
                "groups_1_vs_adamw_ref": bit_equal(got["groups_1"], expected([0] * BUCKETS)),
                "two_calls_vs_groups_2": bit_equal(got["two_calls"], got["groups_2"]),
                "groups_1_vs_one_call": bit_equal(got["groups_1"], got["one_call"])}
    clip = float(got["groups_2"][2].view(np.float32)[1])
    verified["clip_coefficient"] = clip
    ok = all(all(v["planes"].values()) and v["rows"] and v["info"] for v in verified.values() if isinstance(v, dict)) and 0.0 < clip < 1.0 \
        and not np.array_equal(got["groups_2"][0]["param"], got["groups_1"][0]["param"])   # the second group matters
    if not ok:   # nothing is timed on wrong output
        print(json.dumps({"verified": False, "verified_per_arm": verified}))
        print("NOT verified")
        return 1

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

    launches, kernels = {}, {}
    for k, a in arms.items():
        with t.launch_trace() as tr:
            with torch.cuda.stream(s):
                a()
        launches[k], kernels[k] = tr.count, tr.kernels
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
    plan.close()
    res = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
               "rounds_us": [round(x, 3) for x in v]} for k, v in us.items()}
    a, b, c, d = (res[k] for k in ("groups_2", "two_calls", "one_call", "groups_1"))
    lookup = round(d["median_us"] - c["median_us"], 3)
    spread = round(max(c["max_us"] - c["min_us"], d["max_us"] - d["min_us"]), 3)
    out = {
        "shape": {"algo": "swing", "side": SIDE, "ranks": P, "buckets": BUCKETS, "tiles_per_rank": TILES,
                  "bytes_per_rank_per_bucket": 2 * n, "rank_stride": stride,
                  "flat_planes": f"four of {P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
        "mode": "graph", "groups": GROUPS, "group_of": group_of, "step": STEP, "max_norm": MAX_NORM,
        "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS,
        "arm_names": {"a": "groups_2", "b": "two_calls", "c": "one_call", "d": "groups_1"},
        "library_launches_per_call": launches, "kernels": kernels,
        "arms": res,
        "groups_2_median_below_two_calls_min": a["median_us"] < b["min_us"],
        "two_calls_over_groups_2": round(b["median_us"] / a["median_us"], 3),
        "groups_2_minus_one_call_us": round(a["median_us"] - c["median_us"], 3),
        "lookup_cost_us_groups_1_minus_one_call": lookup,
        "largest_round_to_round_spread_of_those_two_arms_us": spread,
        "lookup_cost_exceeds_that_spread": abs(lookup) > spread,
        "session": "one session on one MI355X; eager calls and the host cost of the checks are not measured",
        "verified": True, "verified_per_arm": verified,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    print("verified")
    return 0


if __name__ == "__main__":
    sys.exit(main())
