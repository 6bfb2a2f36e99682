"""The MXFP8 all-gather from fp32 shards (Plan.all_gather_shards_mxfp8, both flag values) against the bf16
all-gather from the same shards (Plan.all_gather_shards_f32), in one build, with the method of
tools/adamw_groups_bench.py: 8x8 Swing, 64 ranks, one GPU, replayed from a HIP graph (the device side
alone).  Two shapes:
  buckets16   sixteen buckets of 64 tiles (16,384 elements, 32 kB of bf16 per rank), one rank-major flat
              fp32 shard buffer (64 rows of F = 16 x 256 floats; bucket i at column 256 i) — latency-bound:
              no gain is expected and none is required;
  one_large   one bucket of 327,680 elements per rank (config 2's size: 1280 tiles, 20 per block), where
              the written bytes are 64 n 1.03125 against 64 n 2.
Arms, alternated in one process: mxfp8_floor, mxfp8_rceil, bf16.  Nothing is fixed in advance: what was
measured is written down either way.

Before anything is timed: the element rows and scale rows of both MXFP8 arms are BIT-equal to
tests/mxfp8_ref.py's numpy expectation, and the bf16 rows to tests/f32_tree.py's bf16_rne.  A round
times each arm over WINDOWS replays of a graph of CALLS calls between device events.  Eager calls and
the host cost of the checks are not measured.  Writes one JSON (default profiles/mx_all_gather.json,
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

import f32_tree  # noqa: E402  (tests/f32_tree.py: bf16_rne)
import mxfp8_ref  # noqa: E402  (tests/mxfp8_ref.py: the expectation)
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
SHAPES = {"buckets16": (16, 64), "one_large": (1, 1280)}   # buckets, tiles per rank row
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3


def run_shape(name, plan, s, dev, rng):
    count, tiles = SHAPES[name]
    n = 256 * tiles
    blk = n // P
    F = count * blk
    host = (rng.standard_normal((P, F)) * np.exp2(rng.integers(-12, 6, (P, F // 32)).repeat(32, axis=1))).astype(np.float32)
    shard = torch.from_numpy(host).to(dev)
    stride16 = t.preferred_rank_stride(n)
    rows16 = [torch.zeros((P, stride16), dtype=torch.int16, device=dev) for _ in range(count)]
    rows8 = [torch.zeros((P, n), dtype=torch.uint8, device=dev) for _ in range(count)]
    scales = [torch.zeros((P, n // 32), dtype=torch.uint8, device=dev) for _ in range(count)]
    at = lambda i: shard.data_ptr() + 4 * blk * i   # noqa: E731
    mx = [(rows8[i].data_ptr(), n, scales[i].data_ptr(), n // 32, n, at(i), F) for i in range(count)]
    bf = [(rows16[i].data_ptr(), stride16, n, at(i), F) for i in range(count)]
    arms = {"mxfp8_floor": lambda: plan.all_gather_shards_mxfp8(mx, rceil=False, stream=s),
            "mxfp8_rceil": lambda: plan.all_gather_shards_mxfp8(mx, rceil=True, stream=s),
            "bf16": lambda: plan.all_gather_shards_f32(bf, s)}

    def run_once(arm):
        with torch.cuda.stream(s):
            for r in rows16 + rows8 + scales:
                r.zero_()
            arms[arm]()
        torch.cuda.synchronize()

    verified = {}
    for arm, rceil in (("mxfp8_floor", False), ("mxfp8_rceil", True)):
        run_once(arm)
        ok = True
        for i in range(count):
            we, ws = mxfp8_ref.expected_rows(host[:, i * blk:(i + 1) * blk], rceil)
            ok = ok and np.array_equal(rows8[i].cpu().numpy(), np.broadcast_to(we, (P, n))) \
                and np.array_equal(scales[i].cpu().numpy(), np.broadcast_to(ws, (P, n // 32)))
        verified[arm] = bool(ok)
    run_once("bf16")
    verified["bf16"] = bool(all(
        np.array_equal(rows16[i][:, :n].cpu().numpy().view(np.uint16),
                       np.broadcast_to(f32_tree.bf16_rne(host[:, i * blk:(i + 1) * blk]).reshape(-1), (P, n))) for i in range(count)))
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
    res = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
               "rounds_us": [round(x, 3) for x in v]} for k, v in us.items()}
    elems = count * n
    return {
        "shape": {"buckets": count, "tiles_per_rank": tiles, "elems_per_rank_per_bucket": n,
                  "flat_shard": f"{P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
        "algorithmic_bytes": {"read_fp32_shard": 4 * elems, "written_mxfp8": P * elems + P * elems // 32, "written_bf16": 2 * P * elems},
        "library_launches_per_call": launches, "kernels": kernels, "arms": res,
        "bf16_over_mxfp8_floor": round(res["bf16"]["median_us"] / res["mxfp8_floor"]["median_us"], 3),
        "bf16_over_mxfp8_rceil": round(res["bf16"]["median_us"] / res["mxfp8_rceil"]["median_us"], 3),
        "mxfp8_floor_median_below_bf16_min": res["mxfp8_floor"]["median_us"] < res["bf16"]["min_us"],
        "mxfp8_rceil_median_below_bf16_min": res["mxfp8_rceil"]["median_us"] < res["bf16"]["min_us"],
        "verified": True, "verified_per_arm": verified,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_all_gather.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(17)
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    shapes = {name: run_shape(name, plan, s, dev, rng) for name in SHAPES}
    plan.close()
    ok = all(v["verified"] for v in shapes.values())
    out = {"algo": "swing", "side": SIDE, "ranks": P, "mode": "graph", "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS,
           "shapes": shapes, "verified": ok,
           "session": "one session on one MI355X; eager calls and the host cost of the checks are not measured"}
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
