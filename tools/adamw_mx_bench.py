"""AdamW inside the MXFP8 all-gather's launch (Plan.adamw_all_gather_shards_mxfp8) against what it replaces,
with the method of tools/adamw_shard_bench.py and tools/adamw_groups_bench.py unchanged:
8x8 Swing, 64 ranks, FOUR rank-major flat fp32 planes, one GPU, replayed from a HIP graph (the device side
alone).  Two shapes:
  buckets16   sixteen buckets of 64 tiles (16,384 elements per rank: 32 kB of bf16), one tile per block;
  one_large   one bucket of 327,680 elements per rank (1280 tiles, 20 per block).
Arms, alternated in one process (the floor scale rule throughout):
  (a) adamw_mx          the new call, two parameter groups alternating bucket by bucket, clipping active    one launch
  (b) groups_then_mx    what it replaces: adamw_all_gather_shards_f32_groups (whose bf16 rows nobody reads),
                        then all_gather_shards_mxfp8 from the param plane                                    two launches
  (c) groups_alone      adamw_all_gather_shards_f32_groups
  (d) mx_alone          all_gather_shards_mxfp8
  (e) step_adamw_mx     the whole step: reduce_scatter_shards_f32_norm, then (a)                             two launches
  (f) step_groups_mx    the whole step: reduce_scatter_shards_f32_norm, then (b)                             three launches
The claim to check is (a) against (b) on both shapes, by the project's convention: (a)'s median below (b)'s
MINIMUM over the rounds.  No ratio is fixed in advance; (a) against (c) and (d) is recorded without a
requirement.  What was measured is written down either way.

Before anything is timed, from pristine buffers: (a)'s four planes, element rows, scale rows and info are
BIT-equal to tests/adamw_mx_ref.py's numpy expectation (the gradient norm here is about 512, so max_norm = 1
clips); (b)'s planes, element rows and scale rows are bit-equal to (a)'s; (c)'s planes to (a)'s and its rows to
bf16_rne of them; (d)'s rows to tests/mxfp8_ref.py's quantisation of the pristine param plane; (e) and (f) to
the numpy expectation on the gradient planes and norm_sq the reduce-scatter left, and to each other.  A round
times each arm over WINDOWS replays of a graph of CALLS calls between device events; the pristine buffers are
restored before every window, outside the events.  Eager calls and the host cost of the checks are not
measured; the grid cap is the inherited one.  Writes one JSON (default profiles/adamw_mx_all_gather.json,
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

import adamw_mx_ref  # noqa: E402  (tests/adamw_mx_ref.py: the expectation)
import f32_tree  # noqa: E402  (tests/f32_tree.py: bf16_rne)
import mxfp8_ref  # noqa: E402
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
SHAPES = {"buckets16": (16, 64), "one_large": (1, 1280)}   # buckets, tiles per rank row
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
STEP, MAX_NORM = 3, 1.0
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),     # the weights
          dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]      # biases and norm weights
NAMES = ("param", "grad", "exp_avg", "exp_avg_sq")
ARMS = {"a": "adamw_mx", "b": "groups_then_mx", "c": "groups_alone", "d": "mx_alone", "e": "step_adamw_mx", "f": "step_groups_mx"}


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
    param_rows16 = [torch.zeros((P, stride16), dtype=torch.int16, device=dev) for _ in range(count)]   # (b) and (c): written, never read
    rows8 = [torch.zeros((P, n), dtype=torch.uint8, device=dev) for _ in range(count)]
    scales = [torch.zeros((P, n // 32), dtype=torch.uint8, device=dev) for _ in range(count)]
    host = {"param": rng.standard_normal((P, F)).astype(np.float32), "grad": rng.standard_normal((P, F)).astype(np.float32),
            "exp_avg": (rng.standard_normal((P, F)) * 1e-2).astype(np.float32),
            "exp_avg_sq": (1e-4 * (0.25 + rng.random((P, F)))).astype(np.float32)}   # away from 0: no huge m / sqrt(v)
    pristine = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    plane = {k: v.clone() for k, v in pristine.items()}
    at = lambda k, i: plane[k].data_ptr() + 4 * blk * i   # noqa: E731
    four = lambda i: tuple(at(k, i) for k in NAMES)   # noqa: E731
    mx_adamw = [(rows8[i].data_ptr(), n, scales[i].data_ptr(), n // 32, n) + four(i) + (F,) for i in range(count)]
    bf_adamw = [(param_rows16[i].data_ptr(), stride16, n) + four(i) + (F,) for i in range(count)]
    mx_ag = [(rows8[i].data_ptr(), n, scales[i].data_ptr(), n // 32, n, at("param", i), F) for i in range(count)]
    rs_args = [(grad_rows[i].data_ptr(), stride16, n, at("grad", i), F) for i in range(count)]
    group_of = [i % 2 for i in range(count)]
    ws = torch.zeros(plan.shards_f32_norm_workspace_bytes(rs_args) // 4, dtype=torch.int32, device=dev)
    norm_sq_host = (host["grad"].astype(np.float64) ** 2).sum(axis=1).astype(np.float32)   # per rank, of the pristine gradient
    norm_sq_0 = torch.from_numpy(norm_sq_host).to(dev)
    norm_sq = norm_sq_0.clone()
    hyper_host = t.adamw_hyper_groups(GROUPS, step=STEP, max_norm=MAX_NORM)   # (2, 8): max_norm in every row, so row g is eff(g)
    hyper = torch.from_numpy(hyper_host).to(dev)
    info = torch.zeros(4, dtype=torch.float32, device=dev)

    def restore():
        for k in plane:
            plane[k].copy_(pristine[k])
        norm_sq.copy_(norm_sq_0)

    def adamw_mx():
        plan.adamw_all_gather_shards_mxfp8(mx_adamw, group_of, hyper.data_ptr(), 2, norm_sq.data_ptr(), info.data_ptr(), stream=s)

    def groups_alone():
        plan.adamw_all_gather_shards_f32_groups(bf_adamw, group_of, hyper.data_ptr(), 2, norm_sq.data_ptr(), info.data_ptr(), stream=s)

    def mx_alone():
        plan.all_gather_shards_mxfp8(mx_ag, rceil=False, stream=s)

    def groups_then_mx():
        groups_alone()
        mx_alone()

    def rs_norm():
        plan.reduce_scatter_shards_f32_norm(rs_args, norm_sq.data_ptr(), ws.data_ptr(), 1.0 / P, stream=s)

    def step_adamw_mx():
        rs_norm()
        adamw_mx()

    def step_groups_mx():
        rs_norm()
        groups_then_mx()

    arms = {"adamw_mx": adamw_mx, "groups_then_mx": groups_then_mx, "groups_alone": groups_alone, "mx_alone": mx_alone,
            "step_adamw_mx": step_adamw_mx, "step_groups_mx": step_groups_mx}

    def run_once(arm):
        with torch.cuda.stream(s):
            restore()
            info.zero_()
            for r in param_rows16 + rows8 + scales:
                r.zero_()
            arm()
        torch.cuda.synchronize()
        return {"planes": {k: plane[k].cpu().numpy().view(np.uint32).copy() for k in NAMES},
                "rows8": np.stack([r.cpu().numpy() for r in rows8]), "scales": np.stack([r.cpu().numpy() for r in scales]),
                "rows16": np.stack([r[:, :n].cpu().numpy().view(np.uint16) for r in param_rows16]),
                "info": info.cpu().numpy().view(np.uint32).copy(), "norm_sq": norm_sq.cpu().numpy().copy()}

    def expected(src, nsq):
        """tests/adamw_mx_ref.py's step, bucket by bucket, each with its group's row of hyper_host; src: the four
        planes as (P, F) float32"""
        want = {k: src[k].view(np.uint32).copy() for k in NAMES}
        e8, s8 = np.zeros((count, P, n), dtype=np.uint8), np.zeros((count, P, n // 32), dtype=np.uint8)
        inf = None
        for i, g in enumerate(group_of):
            col = slice(i * blk, (i + 1) * blk)
            new, (e, sc), inf_g = adamw_mx_ref.step(*(src[k][:, col] for k in NAMES), hyper_host[g], nsq, P, False, False)
            for k, v in zip(NAMES, new):
                want[k][:, col] = np.ascontiguousarray(v).view(np.uint32)
            e8[i], s8[i] = e[None, :], sc[None, :]   # block b of EVERY rank's rows
            inf = inf_g if g == 0 or inf is None else inf
        return {"planes": want, "rows8": e8, "scales": s8, "info": inf.view(np.uint32)}

    def same(got, want, keys):
        out = {}
        for k in keys:
            out[k] = all(bool(np.array_equal(got["planes"][p], want["planes"][p])) for p in NAMES) if k == "planes" \
                else bool(np.array_equal(got[k], want[k]))
        return out

    got = {k: run_once(a) for k, a in arms.items()}
    want = expected(host, norm_sq_host)
    verified = {"adamw_mx_vs_numpy": same(got["adamw_mx"], want, ("planes", "rows8", "scales", "info")),
                "groups_then_mx_vs_adamw_mx": same(got["groups_then_mx"], got["adamw_mx"], ("planes", "rows8", "scales", "info")),
                "groups_alone_vs_adamw_mx": same(got["groups_alone"], got["adamw_mx"], ("planes", "info"))}
    new_param = got["groups_alone"]["planes"]["param"].view(np.float32)
    rne = np.stack([np.broadcast_to(f32_tree.bf16_rne(new_param[:, i * blk:(i + 1) * blk]).reshape(-1), (P, n)) for i in range(count)])
    verified["groups_alone_vs_adamw_mx"]["rows16_are_bf16_rne_of_its_param_plane"] = bool(np.array_equal(got["groups_alone"]["rows16"], rne))
    d8 = [mxfp8_ref.expected_rows(host["param"][:, i * blk:(i + 1) * blk], False) for i in range(count)]
    verified["mx_alone_vs_numpy"] = {
        "rows8": bool(all(np.array_equal(got["mx_alone"]["rows8"][i], np.broadcast_to(d8[i][0], (P, n))) for i in range(count))),
        "scales": bool(all(np.array_equal(got["mx_alone"]["scales"][i], np.broadcast_to(d8[i][1], (P, n // 32))) for i in range(count))),
        "planes": all(bool(np.array_equal(got["mx_alone"]["planes"][p], host[p].view(np.uint32))) for p in NAMES)}
    # the whole step: the expectation on what the reduce-scatter left (its own bits are tests/test_gpu_shards_f32_norm.py's business)
    with torch.cuda.stream(s):
        restore()
        rs_norm()
    torch.cuda.synchronize()
    after_rs = {k: plane[k].cpu().numpy().copy() for k in NAMES}
    want_step = expected(after_rs, norm_sq.cpu().numpy().copy())
    verified["step_adamw_mx_vs_numpy"] = same(got["step_adamw_mx"], want_step, ("planes", "rows8", "scales", "info"))
    verified["step_groups_mx_vs_step_adamw_mx"] = same(got["step_groups_mx"], got["step_adamw_mx"], ("planes", "rows8", "scales", "info"))
    clip = float(got["adamw_mx"]["info"].view(np.float32)[1])
    ok = all(all(v.values()) for v in verified.values()) and 0.0 < clip < 1.0 \
        and not np.array_equal(got["adamw_mx"]["planes"]["param"], host["param"].view(np.uint32))
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
    a, b, c, d, e, f = (res[ARMS[k]] for k in "abcdef")
    elems = count * n
    return {
        "shape": {"buckets": count, "tiles_per_rank": tiles, "elems_per_rank_per_bucket": n,
                  "flat_planes": f"four of {P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
        "algorithmic_bytes": {"planes_read": 16 * elems, "planes_written": 12 * elems,
                              "rows_written_adamw_mx": P * elems + P * elems // 32,
                              "rows_written_groups_then_mx": 2 * P * elems + P * elems + P * elems // 32,
                              "param_plane_read_again_by_groups_then_mx": 4 * elems},
        "library_launches_per_call": launches, "kernels": kernels, "arms": res,
        "adamw_mx_median_below_groups_then_mx_min": a["median_us"] < b["min_us"],
        "groups_then_mx_over_adamw_mx": round(b["median_us"] / a["median_us"], 3),
        "adamw_mx_minus_groups_alone_us": round(a["median_us"] - c["median_us"], 3),
        "adamw_mx_minus_mx_alone_us": round(a["median_us"] - d["median_us"], 3),
        "step_adamw_mx_median_below_step_groups_mx_min": e["median_us"] < f["min_us"],
        "step_groups_mx_over_step_adamw_mx": round(f["median_us"] / e["median_us"], 3),
        "verified": True, "verified_per_arm": verified,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_mx_all_gather.json"))
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
           "unmeasured": ["the grid cap (inherited from the grouped all-gather's)", "eager calls and the host cost of the checks"],
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
