"""AdamW inside the MXFP4 all-gather's launch (Plan.adamw_all_gather_shards_mxfp4) against what it replaces, with
the method of tools/adamw_mx_bench.py unchanged: 8x8 Swing, 64 ranks, FOUR rank-major flat fp32
planes, two parameter groups alternating bucket by bucket, clipping active, one GPU, replayed from a HIP graph (the
device side alone), the arms alternated in one process.  §20's two shapes:
  buckets16   sixteen buckets of 64 tiles (16,384 elements per rank), one tile per block;
  one_large   one bucket of 327,680 elements per rank (1280 tiles, 20 per block).
Arms (the floor scale rule throughout):
  (a) adamw_mx4         the new call                                                                        one launch
  (b) groups_then_mx4   what it replaces: adamw_all_gather_shards_f32_groups (whose bf16 rows nobody reads),
                        then all_gather_shards_mxfp4 from the param plane                                    two launches
  (c) adamw_mx8         adamw_all_gather_shards_mxfp8: the same update with rows of twice the bytes         one launch
  (d) step_adamw_mx4    the whole step: reduce_scatter_shards_f32_norm, then (a)                             two launches
      step_groups_mx4   the whole step: reduce_scatter_shards_f32_norm, then (b)                             three launches
The expectation to test is (a)'s median below (b)'s MINIMUM over the rounds on both shapes; no ratio is a pass
condition and (a) against (c) is recorded without a requirement.  What was measured is written down either way.

Before anything is timed, from pristine buffers: (a)'s four planes, nibble rows, scale rows and info are BIT-equal to
the numpy expectation (tests/adamw_ref.py's step, then tests/mxfp4_ref.py's rows of the new param plane); (b)'s and
(c)'s planes and info are bit-equal to (a)'s, (b)'s rows and scales too; both whole steps are bit-equal to the
expectation on what the reduce-scatter left, and to each other.  A round times each arm over WINDOWS replays of a
graph of CALLS calls between device events; the pristine buffers are restored before every window, outside the
events.  Not measured: eager calls, the host cost of the checks, the inherited grid cap, and the other LDS write
form (lane pairs combined into dword writes).  Writes one JSON (default profiles/adamw_mx4_all_gather.json,
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

import adamw_ref  # noqa: E402  (tests/adamw_ref.py: the update)
import mxfp4_ref  # noqa: E402  (tests/mxfp4_ref.py: the rows)
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
SHAPES = {"buckets16": (16, 64), "one_large": (1, 1280)}   # buckets, tiles per rank row
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
STEP, MAX_NORM = 3, 1.0
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),     # the weights
          dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]      # biases and norm weights
NAMES = ("param", "grad", "exp_avg", "exp_avg_sq")
ARMS = {"a": "adamw_mx4", "b": "groups_then_mx4", "c": "adamw_mx8", "d": "step_adamw_mx4", "d'": "step_groups_mx4"}
ALL = ("planes", "rows4", "scales", "info")


def run_shape(name, plan, s, dev, rng):
    count, tiles = SHAPES[name]
    n = 256 * tiles
    blk = n // P
    F = count * blk
    stride16 = t.preferred_rank_stride(n)

    def rows16():
        host = np.zeros((P, stride16), dtype=np.uint16)
        host[:, :n] = rng.integers(0x3C00, 0x3F80, (P, n)) | (rng.integers(0, 2, (P, n)) << 15)   # +-[2^-7, 1)
        return torch.from_numpy(host.view(np.int16)).to(dev)

    grad_rows = [rows16() for _ in range(count)]                # the reduce-scatter's input: only read
    param_rows16 = [torch.zeros((P, stride16), dtype=torch.int16, device=dev) for _ in range(count)]   # (b): written, never read
    rows4 = [torch.zeros((P, n // 2), dtype=torch.uint8, device=dev) for _ in range(count)]
    rows8 = [torch.zeros((P, n), dtype=torch.uint8, device=dev) for _ in range(count)]             # (c)
    scales = [torch.zeros((P, n // 32), dtype=torch.uint8, device=dev) for _ in range(count)]
    host = {"param": rng.standard_normal((P, F)).astype(np.float32), "grad": rng.standard_normal((P, F)).astype(np.float32),
            "exp_avg": (rng.standard_normal((P, F)) * 1e-2).astype(np.float32),
            "exp_avg_sq": (1e-4 * (0.25 + rng.random((P, F)))).astype(np.float32)}   # away from 0: no huge m / sqrt(v)
    pristine = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    plane = {k: v.clone() for k, v in pristine.items()}
    at = lambda k, i: plane[k].data_ptr() + 4 * blk * i   # noqa: E731
    four = lambda i: tuple(at(k, i) for k in NAMES)   # noqa: E731
    mx4_adamw = [(rows4[i].data_ptr(), n // 2, scales[i].data_ptr(), n // 32, n) + four(i) + (F,) for i in range(count)]
    mx8_adamw = [(rows8[i].data_ptr(), n, scales[i].data_ptr(), n // 32, n) + four(i) + (F,) for i in range(count)]
    bf_adamw = [(param_rows16[i].data_ptr(), stride16, n) + four(i) + (F,) for i in range(count)]
    mx4_ag = [(rows4[i].data_ptr(), n // 2, scales[i].data_ptr(), n // 32, n, at("param", i), F) for i in range(count)]
    rs_args = [(grad_rows[i].data_ptr(), stride16, n, at("grad", i), F) for i in range(count)]
    group_of = [i % 2 for i in range(count)]
    ws = torch.zeros(plan.shards_f32_norm_workspace_bytes(rs_args) // 4, dtype=torch.int32, device=dev)
    norm_sq_host = (host["grad"].astype(np.float64) ** 2).sum(axis=1).astype(np.float32)   # per rank, of the pristine gradient
    norm_sq_0 = torch.from_numpy(norm_sq_host).to(dev)
    norm_sq = norm_sq_0.clone()
    hyper_host = t.adamw_hyper_groups(GROUPS, step=STEP, max_norm=MAX_NORM)   # (2, 8): max_norm in every row
    hyper = torch.from_numpy(hyper_host).to(dev)
    info = torch.zeros(4, dtype=torch.float32, device=dev)
    small = (group_of, hyper.data_ptr(), 2, norm_sq.data_ptr(), info.data_ptr())

    def restore():
        for k in plane:
            plane[k].copy_(pristine[k])
        norm_sq.copy_(norm_sq_0)

    def adamw_mx4():
        plan.adamw_all_gather_shards_mxfp4(mx4_adamw, *small, stream=s)

    def groups_then_mx4():
        plan.adamw_all_gather_shards_f32_groups(bf_adamw, *small, stream=s)
        plan.all_gather_shards_mxfp4(mx4_ag, rceil=False, stream=s)

    def adamw_mx8():
        plan.adamw_all_gather_shards_mxfp8(mx8_adamw, *small, stream=s)

    def rs_norm():
        plan.reduce_scatter_shards_f32_norm(rs_args, norm_sq.data_ptr(), ws.data_ptr(), 1.0 / P, stream=s)

    def step_adamw_mx4():
        rs_norm()
        adamw_mx4()

    def step_groups_mx4():
        rs_norm()
        groups_then_mx4()

    arms = {"adamw_mx4": adamw_mx4, "groups_then_mx4": groups_then_mx4, "adamw_mx8": adamw_mx8,
            "step_adamw_mx4": step_adamw_mx4, "step_groups_mx4": step_groups_mx4}

    def run_once(arm):
        with torch.cuda.stream(s):
            restore()
            info.zero_()
            for r in param_rows16 + rows4 + rows8 + scales:
                r.zero_()
            arm()
        torch.cuda.synchronize()
        return {"planes": {k: plane[k].cpu().numpy().view(np.uint32).copy() for k in NAMES},
                "rows4": np.stack([r.cpu().numpy() for r in rows4]), "scales": np.stack([r.cpu().numpy() for r in scales]),
                "info": info.cpu().numpy().view(np.uint32).copy()}

    def expected(src, nsq):
        """tests/adamw_ref.py's step, bucket by bucket with its group's row of hyper_host, then tests/mxfp4_ref.py's rows
        of the new param plane; src: the four planes as (P, F) float32"""
        want = {k: src[k].view(np.uint32).copy() for k in NAMES}
        e4, s4 = np.zeros((count, P, n // 2), dtype=np.uint8), np.zeros((count, P, n // 32), dtype=np.uint8)
        inf = None
        for i, g in enumerate(group_of):
            col = slice(i * blk, (i + 1) * blk)
            new, _, inf_g = adamw_ref.step(*(src[k][:, col] for k in NAMES), hyper_host[g], nsq, P, False)
            for k, v in zip(NAMES, new):
                want[k][:, col] = np.ascontiguousarray(v).view(np.uint32)
            e, sc = mxfp4_ref.expected_rows(new[0], False)
            e4[i], s4[i] = e[None, :], sc[None, :]   # block b of EVERY rank's rows
            inf = inf_g if g == 0 or inf is None else inf
        return {"planes": want, "rows4": e4, "scales": s4, "info": inf.view(np.uint32)}

    def same(got, want, keys):
        return {k: all(bool(np.array_equal(got["planes"][p], want["planes"][p])) for p in NAMES) if k == "planes"
                else bool(np.array_equal(got[k], want[k])) for k in keys}

    got = {k: run_once(a) for k, a in arms.items()}
    verified = {"adamw_mx4_vs_numpy": same(got["adamw_mx4"], expected(host, norm_sq_host), ALL),
                "groups_then_mx4_vs_adamw_mx4": same(got["groups_then_mx4"], got["adamw_mx4"], ALL),
                "adamw_mx8_vs_adamw_mx4": same(got["adamw_mx8"], got["adamw_mx4"], ("planes", "info"))}
    # the whole step: the expectation on what the reduce-scatter left (its own bits are tests/test_gpu_shards_f32_norm.py's business)
    with torch.cuda.stream(s):
        restore()
        rs_norm()
    torch.cuda.synchronize()
    after_rs = {k: plane[k].cpu().numpy().copy() for k in NAMES}
    verified["step_adamw_mx4_vs_numpy"] = same(got["step_adamw_mx4"], expected(after_rs, norm_sq.cpu().numpy().copy()), ALL)
    verified["step_groups_mx4_vs_step_adamw_mx4"] = same(got["step_groups_mx4"], got["step_adamw_mx4"], ALL)
    clip = float(got["adamw_mx4"]["info"].view(np.float32)[1])
    ok = all(all(v.values()) for v in verified.values()) and 0.0 < clip < 1.0 \
        and not np.array_equal(got["adamw_mx4"]["planes"]["param"], host["param"].view(np.uint32))
    verified["clip_coefficient"] = clip
    if not ok:   # nothing is timed on wrong output
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
    a, b, c, d, d2 = (res[ARMS[k]] for k in ("a", "b", "c", "d", "d'"))
    elems = count * n
    return {
        "shape": {"buckets": count, "tiles_per_rank": tiles, "elems_per_rank_per_bucket": n,
                  "flat_planes": f"four of {P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
        "bytes_written_per_call": {"adamw_mx4": 12 * elems + P * elems // 2 + P * elems // 32,
                                   "groups_then_mx4": 12 * elems + 2 * P * elems + P * elems // 2 + P * elems // 32,
                                   "adamw_mx8": 12 * elems + P * elems + P * elems // 32},
        "bytes_read_per_call": {"adamw_mx4": 16 * elems, "groups_then_mx4": 16 * elems + 4 * elems, "adamw_mx8": 16 * elems},
        "library_launches_per_call": launches, "kernels": kernels, "arms": res,
        "adamw_mx4_median_below_groups_then_mx4_min": a["median_us"] < b["min_us"],
        "groups_then_mx4_over_adamw_mx4": round(b["median_us"] / a["median_us"], 3),
        "adamw_mx4_minus_adamw_mx8_us": round(a["median_us"] - c["median_us"], 3),
        "step_adamw_mx4_median_below_step_groups_mx4_min": d["median_us"] < d2["min_us"],
        "step_groups_mx4_over_step_adamw_mx4": round(d2["median_us"] / d["median_us"], 3),
        "verified": True, "verified_per_arm": verified,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_mx4_all_gather.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    shapes = {name: run_shape(name, plan, s, dev, rng) for name in SHAPES}
    plan.close()
    ok = all(v["verified"] for v in shapes.values())
    out = {"algo": "swing", "side": SIDE, "ranks": P, "mode": "graph", "groups": GROUPS, "step": STEP, "max_norm": MAX_NORM,
           "scale_rule": "floor", "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS, "arm_names": ARMS,
           "shapes": shapes, "verified": ok,
           "unmeasured": ["eager calls and the host cost of the checks", "the grid cap (inherited from the grouped all-gather's)",
                          "the other LDS write form: lane pairs combined over a DPP step into dword writes"],
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
