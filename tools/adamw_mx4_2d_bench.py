"""AdamW inside the 2D MXFP4 all-gather's launch (Plan.adamw_all_gather_shards_mxfp4_2d) against what it replaces, with
the method of tools/adamw_mx4_bench.py and tools/mx4_2d_bench.py unchanged: 8x8 Swing, 64 ranks, FOUR rank-major flat
fp32 planes, two parameter groups alternating bucket by bucket, clipping active, the floor scale rule, one GPU, graphs of
CALLS calls replayed (the device side alone), the arms alternated in one process.  Shapes: the parent profiles' three —
  buckets16   sixteen buckets of 2048 x 128 (R = 32): every strip spans FOUR shard blocks;
  one_large   one bucket of 2048 x 160 (R = 32);
  tall4       four buckets of 4096 x 128 (R = 64): a strip spans two shard blocks.
Arms:
  (a) new_both      the new call with both outputs                                                           one launch
  (b) mx4_then_t    what it replaces: adamw_all_gather_shards_mxfp4 (the row-wise rows), then
                    all_gather_shards_mxfp4_2d column-wise only, which reads p' back                         two launches
  (c) new_t         the new call column-wise only                                                            one launch
  (d) groups_then_t adamw_all_gather_shards_f32_groups (whose bf16 rows nobody reads), then the same
                    column-wise call                                                                         two launches
  (e) mx8_both      adamw_all_gather_shards_mxfp8_2d on the same shapes: twice the element bytes             one launch
  (f) step_new      the whole step: reduce_scatter_shards_f32_norm, then (a)                                 two launches
      step_pair     the whole step: reduce_scatter_shards_f32_norm, then (b)                                 three launches
No threshold is set.  "Faster than the pair" is claimed only where the new call's MAXIMUM over the rounds lies below the
pair's MINIMUM ((a) against (b), (c) against (d), step_new against step_pair); what was measured is written down either way.

Before anything is timed, from pristine buffers: (a)'s four planes, info and four outputs are BIT-equal to the numpy
expectation (tests/adamw_ref.py's step, then tests/mx4_2d_ref.py of the new param plane; rank 0's rows on the host, every
other rank's against rank 0's); (b)'s planes, info and outputs are bit-equal to (a)'s, (c)'s and (d)'s planes and t outputs,
(e)'s planes and info; step_new is bit-equal to the expectation on what the reduce-scatter left, step_pair to step_new.  The
planes are restored before every window, outside the events.  Not measured: eager calls, the host cost of the checks, the
inherited grid cap.  Writes one JSON (default profiles/adamw_mx4_2d_all_gather.json, --out PATH) and prints it."""
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
import mx4_2d_ref  # noqa: E402  (tests/mx4_2d_ref.py: both orientations)
import tenstorrentallreduce_amd as t  # noqa: E402

SIDE, P = 8, 64
SHAPES = {"buckets16": (16, 128, 32), "one_large": (1, 160, 32), "tall4": (4, 128, 64)}   # buckets, cols, R
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
STEP, MAX_NORM = 3, 1.0
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),     # the weights
          dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]      # biases and norm weights
NAMES = ("param", "grad", "exp_avg", "exp_avg_sq")
KEYS = ("rows", "scales", "t_rows", "t_scales")
PAIRS = (("new_both", "mx4_then_t"), ("new_t", "groups_then_t"), ("step_new", "step_pair"))


def run_shape(name, plan, s, dev, rng):
    count, cols, R = SHAPES[name]
    nrows = P * R
    n, blk = nrows * cols, R * cols
    F = count * blk
    stride16 = t.preferred_rank_stride(n)

    def rows16(fill):
        host = np.zeros((P, stride16), dtype=np.uint16)
        if fill:
            host[:, :n] = rng.integers(0x3C00, 0x3F80, (P, n)) | (rng.integers(0, 2, (P, n)) << 15)   # +-[2^-7, 1)
        return torch.from_numpy(host.view(np.int16)).to(dev)

    grad_rows = [rows16(True) for _ in range(count)]       # the reduce-scatter's input: only read
    param_rows16 = [rows16(False) for _ in range(count)]   # (d): written, never read
    out4 = {k: [torch.zeros((P, w), dtype=torch.uint8, device=dev) for _ in range(count)] for k, w in zip(KEYS, (n // 2, n // 32) * 2)}
    out8 = {k: [torch.zeros((P, w), dtype=torch.uint8, device=dev) for _ in range(count)] for k, w in zip(KEYS, (n, n // 32) * 2)}
    host = {"param": rng.standard_normal((P, F)).astype(np.float32), "grad": rng.standard_normal((P, F)).astype(np.float32),
            "exp_avg": (rng.standard_normal((P, F)) * 1e-2).astype(np.float32),
            "exp_avg_sq": (1e-4 * (0.25 + rng.random((P, F)))).astype(np.float32)}   # away from 0: no huge m / sqrt(v)
    pristine = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    plane = {k: v.clone() for k, v in pristine.items()}
    at = lambda k, i: plane[k].data_ptr() + 4 * blk * i   # noqa: E731
    four = lambda i: tuple(at(k, i) for k in NAMES)   # noqa: E731

    def outs(o, i, payload):
        return (o["rows"][i].data_ptr(), payload, o["scales"][i].data_ptr(), n // 32, o["t_rows"][i].data_ptr(), payload,
                o["t_scales"][i].data_ptr(), n // 32)

    both4 = [outs(out4, i, n // 2) + (n, cols) + four(i) + (F,) for i in range(count)]
    t4 = [(None, 0, None, 0) + b[4:] for b in both4]
    both8 = [outs(out8, i, n) + (n, cols) + four(i) + (F,) for i in range(count)]
    rows4 = [b[:4] + (n,) + four(i) + (F,) for i, b in enumerate(both4)]                        # adamw_all_gather_shards_mxfp4
    t_ag = [(None, 0, None, 0) + b[4:10] + (at("param", i), F) for i, b in enumerate(both4)]    # all_gather_shards_mxfp4_2d, t only
    bf_adamw = [(param_rows16[i].data_ptr(), stride16, n) + four(i) + (F,) for i in range(count)]
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

    def t_only():
        plan.all_gather_shards_mxfp4_2d(t_ag, rceil=False, stream=s)

    def rs_norm():
        plan.reduce_scatter_shards_f32_norm(rs_args, norm_sq.data_ptr(), ws.data_ptr(), 1.0 / P, stream=s)

    def new_both():
        plan.adamw_all_gather_shards_mxfp4_2d(both4, *small, stream=s)

    def mx4_then_t():
        plan.adamw_all_gather_shards_mxfp4(rows4, *small, stream=s)
        t_only()

    def groups_then_t():
        plan.adamw_all_gather_shards_f32_groups(bf_adamw, *small, stream=s)
        t_only()

    arms = {"new_both": new_both, "mx4_then_t": mx4_then_t,
            "new_t": lambda: plan.adamw_all_gather_shards_mxfp4_2d(t4, *small, stream=s), "groups_then_t": groups_then_t,
            "mx8_both": lambda: plan.adamw_all_gather_shards_mxfp8_2d(both8, *small, stream=s),
            "step_new": lambda: (rs_norm(), new_both()), "step_pair": lambda: (rs_norm(), mx4_then_t())}

    def run_once(arm):
        with torch.cuda.stream(s):
            restore()
            info.zero_()
            for v in list(out4.values()) + list(out8.values()):
                for x in v:
                    x.zero_()
            arm()
        torch.cuda.synchronize()
        got = {k: plane[k].cpu().numpy().view(np.uint32).copy() for k in NAMES}
        got.update({k: [x.clone() for x in v] for k, v in out4.items()})
        got["info"] = info.cpu().numpy().view(np.uint32).copy()
        return got

    def against_numpy(got, src, nsq):
        """tests/adamw_ref.py's step, bucket by bucket with its group's row of hyper_host, then tests/mx4_2d_ref.py of the new
        param plane: rank 0's rows on the host, every other rank's against rank 0's; src: the four planes as (P, F) float32"""
        ok, inf = True, None
        for i, g in enumerate(group_of):
            col = slice(i * blk, (i + 1) * blk)
            new, _, inf_g = adamw_ref.step(*(src[k][:, col] for k in NAMES), hyper_host[g], nsq, P, False)
            ok &= all(bool(np.array_equal(got[k][:, col], np.ascontiguousarray(v).view(np.uint32))) for k, v in zip(NAMES, new))
            for k, v in zip(KEYS, mx4_2d_ref.expected(np.ascontiguousarray(new[0]).reshape(nrows, cols), P)):
                x = got[k][i]
                ok &= bool(np.array_equal(x[0].cpu().numpy(), v)) and bool((x == x[0]).all())
            inf = inf_g if g == 0 or inf is None else inf
        return ok and bool(np.array_equal(got["info"], inf.view(np.uint32)))

    def same(x, y, keys):
        return all(bool(np.array_equal(x[k], y[k])) if isinstance(x[k], np.ndarray) else all(bool(torch.equal(p, q)) for p, q in zip(x[k], y[k]))
                   for k in keys)

    got = {k: run_once(a) for k, a in arms.items()}
    a = got["new_both"]
    verified = {"new_both_vs_numpy": against_numpy(a, host, norm_sq_host),
                "mx4_then_t_vs_new_both": same(got["mx4_then_t"], a, NAMES + KEYS + ("info",)),
                "new_t_vs_new_both": same(got["new_t"], a, NAMES + KEYS[2:] + ("info",)) and not any(bool(x.any()) for k in KEYS[:2] for x in got["new_t"][k]),
                "groups_then_t_vs_new_both": same(got["groups_then_t"], a, NAMES + KEYS[2:] + ("info",)),
                "mx8_both_vs_new_both": same(got["mx8_both"], a, NAMES + ("info",))}
    with torch.cuda.stream(s):   # the whole step: the expectation on what the reduce-scatter left
        restore()
        rs_norm()
    torch.cuda.synchronize()
    after_rs = {k: plane[k].cpu().numpy().copy() for k in NAMES}
    verified["step_new_vs_numpy"] = against_numpy(got["step_new"], after_rs, norm_sq.cpu().numpy().copy())
    verified["step_pair_vs_step_new"] = same(got["step_pair"], got["step_new"], NAMES + KEYS + ("info",))
    clip = float(a["info"].view(np.float32)[1])
    ok = all(verified.values()) and 0.0 < clip < 1.0 and not np.array_equal(a["param"], host["param"].view(np.uint32))
    verified["clip_coefficient"] = clip
    del got, a
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

    kernels, grids = {}, {}
    for k, arm in arms.items():
        with t.launch_trace() as tr:
            with torch.cuda.stream(s):
                arm()
        kernels[k], grids[k] = tr.kernels, tr.grids
    torch.cuda.synchronize()
    graphs = {k: capture(arm) for k, arm in arms.items()}
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
    one4 = P * elems // 2 + P * elems // 32
    out = {"shape": {"buckets": count, "cols": cols, "nrows": nrows, "R": R, "elems_per_rank_per_bucket": n,
                     "flat_planes": f"four of {P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
           "bytes_written_per_call": {"new_both": 12 * elems + 2 * one4, "mx4_then_t": 12 * elems + 2 * one4, "new_t": 12 * elems + one4,
                                      "groups_then_t": 12 * elems + 2 * P * elems + one4,
                                      "mx8_both": 12 * elems + 2 * (P * elems + P * elems // 32)},
           "plane_bytes_read_per_call": {"new_both": 16 * elems, "mx4_then_t": 20 * elems, "new_t": 16 * elems, "groups_then_t": 20 * elems,
                                         "mx8_both": 16 * elems},
           "kernels": kernels, "grids": grids, "arms": res, "verified": True, "verified_per_arm": verified}
    for new, old in PAIRS:
        out[f"{new}_max_below_{old}_min"] = res[new]["max_us"] < res[old]["min_us"]
        out[f"{old}_over_{new}"] = round(res[old]["median_us"] / res[new]["median_us"], 3)
    out["new_both_over_mx8_both"] = round(res["new_both"]["median_us"] / res["mx8_both"]["median_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_mx4_2d_all_gather.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    shapes = {name: run_shape(name, plan, s, dev, rng) for name in SHAPES}
    plan.close()
    ok = all(v["verified"] for v in shapes.values())
    out = {"algo": "swing", "side": SIDE, "ranks": P, "mode": "graph", "groups": GROUPS, "step": STEP, "max_norm": MAX_NORM,
           "scale_rule": "floor", "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS, "shapes": shapes, "verified": ok,
           "unmeasured": ["eager calls and the host cost of the checks", "the grid cap (inherited from the grouped all-gather's)"],
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
