"""The grouped calls on fp32 shards against what the bf16 calls need for the same result:
8x8 Swing, 64 ranks, sixteen buckets of 32 kB per rank (64 tiles, one tile per block) into ONE
rank-major flat fp32 buffer (64 rows of F = 16 x 256 floats; bucket i's shard at column 256 i,
shard_stride = F), one GPU, replayed from a HIP graph (the device side alone).

Arms, alternated in one process:
  rs_f32        Plan.reduce_scatter_shards_f32(scale = 1 / 64, accumulate)            one launch
  rs_composite  Plan.reduce_scatter_shards into a bf16 flat buffer, then torch's
                flat32.add_(flat16.float(), alpha = 1 / 64)                            three launches
  ag_f32        Plan.all_gather_shards_f32                                            one launch
  ag_composite  torch's cast of the fp32 flat buffer to bf16 (the kernel of
                .to(torch.bfloat16), into a preallocated buffer), then
                Plan.all_gather_shards                                                 two launches
Informative: rs_composite_one_add, the same with flat32.add_(flat16, alpha = 1 / 64) — torch's
type promotion inside ONE elementwise kernel, the cheapest composite there is.

No ratio is fixed in advance: the numeric gain of the fp32 calls (no rounding of the tree to
bf16) does not depend on speed; they should not LOSE to the composite they replace.

Before anything is timed: ag_f32's rank rows equal ag_composite's bit for bit (both round the same
finite floats to nearest even), and rs_f32's shard agrees with rs_composite's within the bf16
tree's rounding (2^-6 of the sum of magnitudes: six levels, every add rounded to 8 bits, 6 x 2^-9).  A round
times each arm over WINDOWS replays of a graph of CALLS calls between device events; the pristine
buffers are restored before every window, outside the events.  Writes one JSON (default
profiles/group_shards_f32.json, --out PATH) and prints it."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_shards_f32.json"))
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
    flat16 = torch.zeros((P, F), dtype=torch.bfloat16, device=dev)
    a32 = [(b.data_ptr(), stride, n, flat32.data_ptr() + 4 * blk * i, F) for i, b in enumerate(buf)]
    a16 = [(b.data_ptr(), stride, n, flat16.data_ptr() + 2 * blk * i, F) for i, b in enumerate(buf)]
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only

    def restore():
        for b, p in zip(buf, pristine):
            b.copy_(p)
        flat32.copy_(flat32_0)
        flat16.zero_()

    def rs_f32():
        plan.reduce_scatter_shards_f32(a32, SCALE, accumulate=True, stream=s)

    def rs_composite():
        plan.reduce_scatter_shards(a16, s)
        flat32.add_(flat16.float(), alpha=SCALE)

    def rs_composite_one_add():
        plan.reduce_scatter_shards(a16, s)
        flat32.add_(flat16, alpha=SCALE)

    def ag_f32():
        plan.all_gather_shards_f32(a32, s)

    def ag_composite():
        flat16.copy_(flat32)
        plan.all_gather_shards(a16, s)

    arms = {"rs_f32": rs_f32, "rs_composite": rs_composite, "rs_composite_one_add": rs_composite_one_add,
            "ag_f32": ag_f32, "ag_composite": ag_composite}
    launches = {"rs_f32": plan.shards_f32_launches(a32, t._lib.OP_REDUCE_SCATTER),
                "rs_composite": plan.shards_launches(a16, t._lib.OP_REDUCE_SCATTER) + 2,
                "rs_composite_one_add": plan.shards_launches(a16, t._lib.OP_REDUCE_SCATTER) + 1,
                "ag_f32": plan.shards_f32_launches(a32, t._lib.OP_ALL_GATHER),
                "ag_composite": plan.shards_launches(a16, t._lib.OP_ALL_GATHER) + 1}

    def run_once(arm):
        with torch.cuda.stream(s):
            restore()
            arm()
        torch.cuda.synchronize()
        return [b.clone() for b in buf], flat32.clone()

    rows_a, _ = run_once(ag_f32)
    rows_b, _ = run_once(ag_composite)
    ag_same = all(bool(torch.equal(x, y)) for x, y in zip(rows_a, rows_b))
    _, sh_a = run_once(rs_f32)
    _, sh_b = run_once(rs_composite)
    mags = torch.zeros((P, F), dtype=torch.float32, device=dev)
    for i, p in enumerate(pristine):
        rows = p[:, :n].view(torch.bfloat16).float().abs().sum(dim=0)       # (n,): sum of magnitudes per column
        mags[:, blk * i:blk * (i + 1)] = rows.view(P, blk)
    rs_close = bool(((sh_a - sh_b).abs() <= mags * SCALE * 2.0 ** -6 + 1e-30).all())
    verified = {"ag_f32_equals_ag_composite_bits": ag_same, "rs_f32_within_bf16_tree_rounding_of_rs_composite": rs_close,
                "rs_max_abs_difference": float((sh_a - sh_b).abs().max())}
    if not (ag_same and rs_close):   # nothing is timed on wrong output
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
    plan.close()
    res = {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
               "rounds_us": [round(x, 3) for x in v]} for k, v in us.items()}
    out = {
        "shape": {"algo": "swing", "side": SIDE, "ranks": P, "buckets": BUCKETS, "tiles_per_rank": TILES,
                  "bytes_per_rank_per_bucket": 2 * n, "rank_stride": stride,
                  "flat_shard_buffer": f"{P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
        "mode": "graph", "scale": SCALE, "accumulate": True,
        "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS, "launches_per_call": launches,
        "arms": res,
        "composite_over_f32": {"reduce_scatter": round(res["rs_composite"]["median_us"] / res["rs_f32"]["median_us"], 3),
                               "reduce_scatter_one_add": round(res["rs_composite_one_add"]["median_us"] / res["rs_f32"]["median_us"], 3),
                               "all_gather": round(res["ag_composite"]["median_us"] / res["ag_f32"]["median_us"], 3)},
        "f32_not_slower_than_composite": {"reduce_scatter": res["rs_f32"]["median_us"] <= res["rs_composite"]["median_us"],
                                          "all_gather": res["ag_f32"]["median_us"] <= res["ag_composite"]["median_us"]},
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
