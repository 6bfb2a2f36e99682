"""The fp32 grouped reduce-scatter with the gradient norm in the same launch against what a caller
needs without it, with the method of tools/shard_f32_bench.py: 8x8 Swing, 64 ranks, sixteen buckets
of 32 kB per rank (64 tiles, one tile per block) into ONE rank-major flat fp32 buffer (64 rows of
F = 16 x 256 floats; bucket i's shard at column 256 i, shard_stride = F), scale 1 / 64 and
accumulate, one GPU, replayed from a HIP graph (the device side alone).

Arms, alternated in one process:
  rs_norm         Plan.reduce_scatter_shards_f32_norm                                  one launch
  rs_then_sqsum   Plan.reduce_scatter_shards_f32, then torch's flat32.square().sum(1)
                  into a preallocated buffer                                           three launches
  rs_then_vnorm   Plan.reduce_scatter_shards_f32, then torch.linalg.vector_norm(flat32, dim=1)
                  into a preallocated buffer (the norm, not its square)                two launches
  rs_alone        Plan.reduce_scatter_shards_f32: what the norm costs on top

"composite" is the faster of the two torch arms by its median.  The expectation is rs_norm below
it with rs_norm's median outside the composite's min-max range; what was measured is written down
either way.

Before anything is timed: rs_norm's shards equal rs_alone's bit for bit; rs_norm's norm_sq is
within (16 + 1) 2^-24 x 1.01 (relative) of the float64 sum of squares of the stored floats (one
squaring and at most 2 + 6 + 1 + 6 adds of non-negative terms; 16 partials per rank); torch's
two results agree with float64 to 1e-5; the workspace's counter is zero again.  A round times each arm over WINDOWS
replays of a graph of CALLS calls between device events; the pristine buffers are restored before
every window, outside the events.  Writes one JSON (default profiles/group_shards_f32_norm.json,
--out PATH; --form NAME is recorded as the finalizer form of the build) and prints it."""
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
BUCKETS, TILES = 16, 64
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 3
SCALE = 1.0 / 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_shards_f32_norm.json"))
    ap.add_argument("--form", default="acquire fence + plain loads")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(3)
    n = 256 * TILES
    blk = n // P
    stride = t.preferred_rank_stride(n)
    F = BUCKETS * blk
    pristine, buf = [], []
    for _ in range(BUCKETS):
        host = np.zeros((P, stride), dtype=np.uint16)
        host[:, :n] = rng.integers(0x3F80, 0x42C8, (P, n)) | (rng.integers(0, 2, (P, n)) << 15)   # +-[1, 100)
        pristine.append(torch.from_numpy(host.view(np.int16)).to(dev))
        buf.append(pristine[-1].clone())
    flat32_0 = torch.from_numpy(rng.standard_normal((P, F)).astype(np.float32)).to(dev)
    flat32 = flat32_0.clone()
    a32 = [(b.data_ptr(), stride, n, flat32.data_ptr() + 4 * blk * i, F) for i, b in enumerate(buf)]
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    ws_bytes = plan.shards_f32_norm_workspace_bytes(a32)
    ws = torch.zeros(ws_bytes // 4, dtype=torch.int32, device=dev)   # the counter zeroed once, here
    norm_sq = torch.full((P,), float("nan"), dtype=torch.float32, device=dev)
    sqsum = torch.zeros(P, dtype=torch.float32, device=dev)
    vnorm = torch.zeros(P, dtype=torch.float32, device=dev)

    def restore():
        for b, p in zip(buf, pristine):
            b.copy_(p)
        flat32.copy_(flat32_0)

    def rs_norm():
        plan.reduce_scatter_shards_f32_norm(a32, norm_sq.data_ptr(), ws.data_ptr(), SCALE, accumulate=True, stream=s)

    def rs_alone():
        plan.reduce_scatter_shards_f32(a32, SCALE, accumulate=True, stream=s)

    def rs_then_sqsum():
        rs_alone()
        torch.sum(flat32.square(), 1, out=sqsum)

    def rs_then_vnorm():
        rs_alone()
        torch.linalg.vector_norm(flat32, dim=1, out=vnorm)

    arms = {"rs_norm": rs_norm, "rs_then_sqsum": rs_then_sqsum, "rs_then_vnorm": rs_then_vnorm, "rs_alone": rs_alone}
    rs_launches = plan.shards_f32_launches(a32, t._lib.OP_REDUCE_SCATTER)
    launches = {"rs_norm": rs_launches, "rs_then_sqsum": rs_launches + 2, "rs_then_vnorm": rs_launches + 1,
                "rs_alone": rs_launches}

    def run_once(arm):
        with torch.cuda.stream(s):
            restore()
            arm()
        torch.cuda.synchronize()
        return flat32.clone()

    sh_alone = run_once(rs_alone)
    sh_norm = run_once(rs_norm)
    run_once(rs_then_sqsum)
    run_once(rs_then_vnorm)
    exact = (sh_alone.double() ** 2).sum(dim=1)
    rel = lambda x: float(((x.double() - exact).abs() / exact).max())   # noqa: E731
    bound = (16 + 1) * 2.0 ** -24 * 1.01
    verified = {"rs_norm_shards_equal_rs_alone_bits": bool(torch.equal(sh_norm.view(torch.int32), sh_alone.view(torch.int32))),
                "rs_norm_relative_error_vs_float64": rel(norm_sq), "bound": bound,
                "sqsum_relative_error_vs_float64": rel(sqsum), "vnorm_squared_relative_error_vs_float64": rel(vnorm.double() ** 2),
                "counter_zero_after_the_call": bool((ws[:16] == 0).all())}
    ok = (verified["rs_norm_shards_equal_rs_alone_bits"] and verified["rs_norm_relative_error_vs_float64"] <= bound
          and verified["sqsum_relative_error_vs_float64"] <= 1e-5 and verified["vnorm_squared_relative_error_vs_float64"] <= 1e-5
          and verified["counter_zero_after_the_call"])
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

    graphs = {k: capture(a) for k, a in arms.items()}
    for g in graphs.values():
        for _ in range(WARMUP):
            window(g)
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            us[k].append(sum(window(g) for _ in range(WINDOWS)) / (WINDOWS * CALLS))
    del graphs
    counter_zero = bool((ws[:16] == 0).all())
    plan.close()
    res = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
               "rounds_us": [round(x, 3) for x in v]} for k, v in us.items()}
    composite = min(("rs_then_sqsum", "rs_then_vnorm"), key=lambda k: res[k]["median_us"])
    a, b, c = res["rs_norm"], res[composite], res["rs_alone"]
    out = {
        "shape": {"algo": "swing", "side": SIDE, "ranks": P, "buckets": BUCKETS, "tiles_per_rank": TILES,
                  "bytes_per_rank_per_bucket": 2 * n, "rank_stride": stride,
                  "flat_shard_buffer": f"{P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F",
                  "workspace_bytes": ws_bytes},
        "mode": "graph", "scale": SCALE, "accumulate": True, "finalizer_form": args.form,
        "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS, "launches_per_call": launches,
        "arms": res,
        "composite": composite,
        "composite_over_rs_norm": round(b["median_us"] / a["median_us"], 3),
        "norm_costs_us": round(a["median_us"] - c["median_us"], 3),
        "rs_norm_below_composite": a["median_us"] < b["median_us"],
        "rs_norm_median_outside_composite_range": not (b["min_us"] <= a["median_us"] <= b["max_us"]),
        "counter_zero_after_the_replays": counter_zero,
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
