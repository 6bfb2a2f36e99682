"""AdamW inside the 2D MXFP8 all-gather's launch (Plan.adamw_all_gather_shards_mxfp8_2d) against what a user has
without it, with the method of tools/adamw_mx_bench.py on the shapes of tools/mx2d_bench.py
(DESIGN.md §21): 8x8 Swing, 64 ranks, FOUR rank-major flat fp32 planes, one GPU, replayed from a HIP graph (the
device side alone), the floor scale rule, two parameter groups alternating bucket by bucket, clipping active.
Shapes: buckets16 (sixteen matrices of 2048 x 128, R = 32), one_large (one of 2048 x 160, R = 32), tall4 (four of
4096 x 128, R = 64: patches of 64 x 64).
Arms, alternated in one process:
  (a) adamw_2d          the new call, both outputs                                                         one launch
  (b) adamw_mx_then_t   what a user has today: adamw_all_gather_shards_mxfp8, then all_gather_shards_mxfp8_2d
                        column-wise only from the param plane                                              two launches
  (c) adamw_2d_t_only   the new call, column-wise only                                                     one launch
  (d) step_adamw_2d     reduce_scatter_shards_f32_norm, then (a)                                           two launches
  (e) step_then_t       reduce_scatter_shards_f32_norm, then (b)                                           three launches
The claim to check is (a)'s median below (b)'s MINIMUM over the rounds on tall4; the R = 32 shapes are recorded
without a requirement (their 32-byte t runs dominate both arms, §21).  What was measured is written down either way.

Before anything is timed, from pristine buffers: (a)'s four planes and info are BIT-equal to tests/adamw_ref.py's
numpy step and its four outputs to tests/mx2d_ref.py's quantisation of that p' (rank 0's rows on the host, every other
rank's against rank 0's on the device); (b)'s planes and outputs and (c)'s planes and t outputs are bit-equal to (a)'s;
(d) equals the numpy expectation on the gradient planes and norm_sq the reduce-scatter left, and (e) equals (d).  A
round times each arm over WINDOWS replays of a graph of CALLS calls between device events; the pristine buffers are
restored before every window, outside the events.  Eager calls, the host cost of the checks and the grid cap
(inherited) are not measured.  Writes one JSON (default profiles/adamw_mx2d_all_gather.json, --out PATH) and prints it."""
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

import adamw_ref  # noqa: E402  (tests/adamw_ref.py: the step)
import mx2d_ref  # noqa: E402  (tests/mx2d_ref.py: both quantisations)
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
SHAPES = {"buckets16": (16, 128, 32), "one_large": (1, 160, 32), "tall4": (4, 128, 64)}   # buckets, cols, R
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
STEP, MAX_NORM = 3, 1.0
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),     # the weights
          dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]      # biases and norm weights
NAMES = ("param", "grad", "exp_avg", "exp_avg_sq")
OUTS = ("rows", "scales", "t_rows", "t_scales")
ARMS = {"a": "adamw_2d", "b": "adamw_mx_then_t", "c": "adamw_2d_t_only", "d": "step_adamw_2d", "e": "step_then_t"}


def run_shape(name, plan, s, dev, rng):
    count, cols, R = SHAPES[name]
    nrows = P * R
    n, blk = nrows * cols, R * cols
    F = count * blk
    stride16 = t.preferred_rank_stride(n)
    grad_rows = []                                              # the reduce-scatter's input: only read
    for _ in range(count):
        h = np.zeros((P, stride16), dtype=np.uint16)
        h[:, :n] = rng.integers(0x3C00, 0x3F80, (P, n)) | (rng.integers(0, 2, (P, n)) << 15)   # +-[2^-7, 1)
        grad_rows.append(torch.from_numpy(h.view(np.int16)).to(dev))
    out = {k: [torch.zeros((P, w), dtype=torch.uint8, device=dev) for _ in range(count)] for k, w in zip(OUTS, (n, n // 32, n, n // 32))}
    host = {"param": rng.standard_normal((P, F)).astype(np.float32), "grad": rng.standard_normal((P, F)).astype(np.float32),
            "exp_avg": (rng.standard_normal((P, F)) * 1e-2).astype(np.float32),
            "exp_avg_sq": (1e-4 * (0.25 + rng.random((P, F)))).astype(np.float32)}   # away from 0: no huge m / sqrt(v)
    pristine = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    plane = {k: v.clone() for k, v in pristine.items()}
    at = lambda k, i: plane[k].data_ptr() + 4 * blk * i   # noqa: E731
    four = lambda i: tuple(at(k, i) for k in NAMES)   # noqa: E731
    ptr = lambda k, i: out[k][i].data_ptr()   # noqa: E731
    outs4 = lambda i: (ptr("rows", i), n, ptr("scales", i), n // 32, ptr("t_rows", i), n, ptr("t_scales", i), n // 32)   # noqa: E731
    both = [outs4(i) + (n, cols) + four(i) + (F,) for i in range(count)]
    t_only = [(None, 0, None, 0) + b[4:] for b in both]
    mx_adamw = [outs4(i)[:4] + (n,) + four(i) + (F,) for i in range(count)]
    t_ag = [(None, 0, None, 0) + outs4(i)[4:] + (n, cols, at("param", i), F) for i in range(count)]
    rs_args = [(grad_rows[i].data_ptr(), stride16, n, at("grad", i), F) for i in range(count)]
    group_of = [i % 2 for i in range(count)]
    ws = torch.zeros(plan.shards_f32_norm_workspace_bytes(rs_args) // 4, dtype=torch.int32, device=dev)
    norm_sq_host = (host["grad"].astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    norm_sq_0 = torch.from_numpy(norm_sq_host).to(dev)
    norm_sq = norm_sq_0.clone()
    hyper_host = t.adamw_hyper_groups(GROUPS, step=STEP, max_norm=MAX_NORM)   # (2, 8): max_norm in every row
    hyper = torch.from_numpy(hyper_host).to(dev)
    info = torch.zeros(4, dtype=torch.float32, device=dev)
    small = (hyper.data_ptr(), 2, norm_sq.data_ptr(), info.data_ptr())

    def restore():
        for k in plane:
            plane[k].copy_(pristine[k])
        norm_sq.copy_(norm_sq_0)

    def adamw_2d():
        plan.adamw_all_gather_shards_mxfp8_2d(both, group_of, *small, stream=s)

    def adamw_2d_t_only():
        plan.adamw_all_gather_shards_mxfp8_2d(t_only, group_of, *small, stream=s)

    def adamw_mx_then_t():
        plan.adamw_all_gather_shards_mxfp8(mx_adamw, group_of, *small, stream=s)
        plan.all_gather_shards_mxfp8_2d(t_ag, rceil=False, stream=s)

    def rs_norm():
        plan.reduce_scatter_shards_f32_norm(rs_args, norm_sq.data_ptr(), ws.data_ptr(), 1.0 / P, stream=s)

    def step_adamw_2d():
        rs_norm()
        adamw_2d()

    def step_then_t():
        rs_norm()
        adamw_mx_then_t()

    arms = {"adamw_2d": adamw_2d, "adamw_mx_then_t": adamw_mx_then_t, "adamw_2d_t_only": adamw_2d_t_only,
            "step_adamw_2d": step_adamw_2d, "step_then_t": step_then_t}

    def run_once(arm):
        """the planes and info on the host; of the outputs rank 0's rows on the host and whether every rank's equal them"""
        with torch.cuda.stream(s):
            restore()
            info.zero_()
            for v in out.values():
                for x in v:
                    x.zero_()
            arm()
        torch.cuda.synchronize()
        got = {"planes": {k: plane[k].cpu().numpy().view(np.uint32).copy() for k in NAMES}, "info": info.cpu().numpy().view(np.uint32).copy()}
        for k in OUTS:
            got[k] = np.stack([x[0].cpu().numpy() for x in out[k]])
            got[k + "_all_ranks_alike"] = all(bool((x == x[0:1]).all().item()) for x in out[k])
        return got

    def expected(src, nsq):
        want = {"planes": {k: src[k].view(np.uint32).copy() for k in NAMES}}
        q = {k: [] for k in OUTS}
        inf = None
        for i, g in enumerate(group_of):
            col = slice(i * blk, (i + 1) * blk)
            new, _, inf_g = adamw_ref.step(*(src[k][:, col] for k in NAMES), hyper_host[g], nsq, P, False)
            for k, v in zip(NAMES, new):
                want["planes"][k][:, col] = np.ascontiguousarray(v).view(np.uint32)
            W = np.ascontiguousarray(new[0]).reshape(nrows, cols)
            for k, v in zip(OUTS, mx2d_ref.expected_rows(W, P, False) + mx2d_ref.expected_t(W, False)):
                q[k].append(v)
            inf = inf_g if g == 0 or inf is None else inf
        want.update({k: np.stack(v) for k, v in q.items()})
        want["info"] = inf.view(np.uint32)
        return want

    def same(got, want, keys):
        res = {k: (all(bool(np.array_equal(got["planes"][p], want["planes"][p])) for p in NAMES) if k == "planes"
                   else bool(np.array_equal(got[k], want[k]))) for k in keys}
        res.update({k + "_all_ranks_alike": got[k + "_all_ranks_alike"] for k in keys if k in OUTS})
        return res

    got = {k: run_once(a) for k, a in arms.items()}
    everything = ("planes", "info") + OUTS
    verified = {"adamw_2d_vs_numpy": same(got["adamw_2d"], expected(host, norm_sq_host), everything),
                "adamw_mx_then_t_vs_adamw_2d": same(got["adamw_mx_then_t"], got["adamw_2d"], everything),
                "adamw_2d_t_only_vs_adamw_2d": same(got["adamw_2d_t_only"], got["adamw_2d"], ("planes", "info", "t_rows", "t_scales"))}
    with torch.cuda.stream(s):   # the whole step: the expectation on what the reduce-scatter left
        restore()
        rs_norm()
    torch.cuda.synchronize()
    after_rs = {k: plane[k].cpu().numpy().copy() for k in NAMES}
    verified["step_adamw_2d_vs_numpy"] = same(got["step_adamw_2d"], expected(after_rs, norm_sq.cpu().numpy().copy()), everything)
    verified["step_then_t_vs_step_adamw_2d"] = same(got["step_then_t"], got["step_adamw_2d"], everything)
    clip = float(got["adamw_2d"]["info"].view(np.float32)[1])
    ok = all(all(v.values()) for v in verified.values()) and 0.0 < clip < 1.0 \
        and not np.array_equal(got["adamw_2d"]["planes"]["param"], host["param"].view(np.uint32))
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
    a, b, c, d, e = (res[ARMS[k]] for k in "abcde")
    elems = count * n
    return {
        "shape": {"buckets": count, "cols": cols, "nrows": nrows, "rows_per_block": R, "elems_per_rank_per_bucket": n,
                  "flat_planes": f"four of {P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
        "algorithmic_bytes": {"planes_read": 16 * elems, "planes_written": 12 * elems,
                              "outputs_written": 2 * (P * elems + P * elems // 32),
                              "param_plane_read_again_by_adamw_mx_then_t": 4 * elems},
        "library_launches_per_call": launches, "kernels": kernels, "arms": res,
        "adamw_2d_median_below_adamw_mx_then_t_min": a["median_us"] < b["min_us"],
        "adamw_mx_then_t_over_adamw_2d": round(b["median_us"] / a["median_us"], 3),
        "adamw_2d_minus_t_only_us": round(a["median_us"] - c["median_us"], 3),
        "step_adamw_2d_median_below_step_then_t_min": d["median_us"] < e["min_us"],
        "step_then_t_over_step_adamw_2d": round(e["median_us"] / d["median_us"], 3),
        "verified": True, "verified_per_arm": verified,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_mx2d_all_gather.json"))
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
           "unmeasured": ["the grid cap (inherited from the grouped all-gather's)", "eager calls and the host cost of the checks",
                          "patches across neighbouring shard blocks (out of scope)"],
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
