"""AdamW inside the grouped all-gather's launch (Plan.adamw_all_gather_shards_f32) against what a
caller needs without it, with the method of tools/shard_f32_norm_bench.py: 8x8
Swing, 64 ranks, sixteen buckets of 32 kB per rank (64 tiles, one tile per block), FOUR rank-major
flat fp32 planes (64 rows of F = 16 x 256 floats each: param, grad, exp_avg, exp_avg_sq; bucket i at
column 256 i, shard_stride = F), one GPU, replayed from a HIP graph (the device side alone).

Arms, alternated in one process:
  adamw_ag            the new call with norm_sq, clipping active                        one launch
  torch_clip_ag       torch forming the clip coefficient from norm_sq (sum, sqrt, add, reciprocal-multiply,
                      clamp), grad.mul_ by it, torch._fused_adamw_ on the flat planes, then
                      Plan.all_gather_shards_f32 — what the same result takes without the call
  adamw_ag_noclip     the new call with norm_sq = NULL
  torch_noclip_ag     torch._fused_adamw_, then Plan.all_gather_shards_f32
  ag_alone            Plan.all_gather_shards_f32: what the update costs on top
  step_adamw          Plan.reduce_scatter_shards_f32_norm, then adamw_ag: the two-launch step
  step_torch          Plan.reduce_scatter_shards_f32_norm, then torch_clip_ag

Before anything is timed, from pristine buffers: adamw_ag's param, exp_avg and exp_avg_sq planes are
within 2e-6 (absolute) of torch_clip_ag's — the bound tests/test_adamw_ref.py pins between the
numpy expectation and torch.optim.AdamW; the gradient norm here is about 512, so max_norm = 1 clips;
the rows adamw_ag wrote are bit-equal to torch's bf16 rounding (RNE) of adamw_ag's own param plane,
and within one bf16 ulp of torch_clip_ag's rows; the same for the two no-clip arms.  A round times
each arm over WINDOWS replays of a graph of CALLS calls between device events; the pristine buffers
are restored before every window, outside the events.  The expectation is adamw_ag below
torch_clip_ag with its median outside that arm's min-max range; what was measured is written down
either way.  Eager calls are not measured.  Writes one JSON (default profiles/adamw_shards.json,
--out PATH) and prints it."""
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
LR, BETAS, EPS, WD, STEP, MAX_NORM = 1e-3, (0.9, 0.999), 1e-8, 0.01, 3, 1.0
TOL = 2e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_shards.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    n = 256 * TILES
    blk = n // P
    stride = t.preferred_rank_stride(n)
    F = BUCKETS * blk

    def rows():
        host = np.zeros((P, stride), dtype=np.uint16)
        host[:, :n] = rng.integers(0x3C00, 0x3F80, (P, n)) | (rng.integers(0, 2, (P, n)) << 15)   # +-[2^-7, 1)
        return torch.from_numpy(host.view(np.int16)).to(dev)

    grad_rows = [rows() for _ in range(BUCKETS)]                # the reduce-scatter's input: only read
    param_rows = [torch.zeros((P, stride), dtype=torch.int16, device=dev) for _ in range(BUCKETS)]
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)   # noqa: E731
    pristine = {"param": f32(rng.standard_normal((P, F))), "grad": f32(rng.standard_normal((P, F))),
                "exp_avg": f32(rng.standard_normal((P, F)) * 1e-2), "exp_avg_sq": f32(1e-4 * (0.25 + rng.random((P, F))))}   # away from 0: no huge m / sqrt(v)
    plane = {k: v.clone() for k, v in pristine.items()}
    at = lambda k, i: plane[k].data_ptr() + 4 * blk * i   # noqa: E731
    adamw_args = [(param_rows[i].data_ptr(), stride, n, at("param", i), at("grad", i), at("exp_avg", i), at("exp_avg_sq", i), F)
                  for i in range(BUCKETS)]
    ag_args = [(param_rows[i].data_ptr(), stride, n, at("param", i), F) for i in range(BUCKETS)]
    rs_args = [(grad_rows[i].data_ptr(), stride, n, at("grad", i), F) for i in range(BUCKETS)]
    plan = t.Plan(t.SWING, t.BO, SIDE, 256 * P, P, t.EXEC_FUSED)   # the schedule only
    ws = torch.zeros(plan.shards_f32_norm_workspace_bytes(rs_args) // 4, dtype=torch.int32, device=dev)
    norm_sq_0 = (pristine["grad"].double() ** 2).sum(dim=1).float()   # per rank, of the pristine gradient
    norm_sq = norm_sq_0.clone()
    hyper = torch.from_numpy(t.adamw_hyper(LR, BETAS, EPS, WD, STEP, MAX_NORM)).to(dev)
    hyper_noclip = torch.from_numpy(t.adamw_hyper(LR, BETAS, EPS, WD, STEP)).to(dev)
    info = torch.zeros(4, dtype=torch.float32, device=dev)
    step_t = torch.tensor(float(STEP), device=dev)
    coef = torch.zeros((), dtype=torch.float32, device=dev)

    def restore():
        for k in plane:
            plane[k].copy_(pristine[k])
        norm_sq.copy_(norm_sq_0)

    def adamw_ag():
        plan.adamw_all_gather_shards_f32(adamw_args, hyper.data_ptr(), norm_sq.data_ptr(), info.data_ptr(), stream=s)

    def adamw_ag_noclip():
        plan.adamw_all_gather_shards_f32(adamw_args, hyper_noclip.data_ptr(), None, None, stream=s)

    def ag_alone():
        plan.all_gather_shards_f32(ag_args, s)

    def fused():
        torch._fused_adamw_([plane["param"]], [plane["grad"]], [plane["exp_avg"]], [plane["exp_avg_sq"]], [], [step_t], lr=LR,
                            beta1=BETAS[0], beta2=BETAS[1], weight_decay=WD, eps=EPS, amsgrad=False, maximize=False)

    def torch_noclip_ag():
        fused()
        ag_alone()

    def torch_clip_ag():
        # torch.nn.utils.clip_grad_norm_'s arithmetic from the per-rank squared norms
        torch.clamp(MAX_NORM / (norm_sq.sum().sqrt() + 1e-6), max=1.0, out=coef)
        plane["grad"].mul_(coef)
        fused()
        ag_alone()

    def rs_norm():
        plan.reduce_scatter_shards_f32_norm(rs_args, norm_sq.data_ptr(), ws.data_ptr(), 1.0 / P, stream=s)

    def step_adamw():
        rs_norm()
        adamw_ag()

    def step_torch():
        rs_norm()
        torch_clip_ag()

    arms = {"adamw_ag": adamw_ag, "torch_clip_ag": torch_clip_ag, "adamw_ag_noclip": adamw_ag_noclip,
            "torch_noclip_ag": torch_noclip_ag, "ag_alone": ag_alone, "step_adamw": step_adamw, "step_torch": step_torch}

    def run_once(arm):
        with torch.cuda.stream(s):
            restore()
            arm()
        torch.cuda.synchronize()
        return {k: plane[k].clone() for k in ("param", "exp_avg", "exp_avg_sq")}, torch.stack([r[:, :n].clone() for r in param_rows])

    def as_f32(rows16):   # bf16 bit patterns (int16) -> float32
        return (rows16.to(torch.int32) << 16).view(torch.float32)

    def compare(new, ref):
        (pn, rn), (pr, rr) = new, ref
        plane_diff = {k: float((pn[k] - pr[k]).abs().max()) for k in pn}
        # the new call's rows: block b of every rank row = RNE of its own new param plane, block b
        own = pn["param"].to(torch.bfloat16).view(torch.int16).view(P, BUCKETS, blk).permute(1, 0, 2).reshape(BUCKETS, 1, n)
        a, b = as_f32(rn), as_f32(rr)
        ulp = torch.maximum(a.abs(), b.abs()) * 2.0 ** -7
        return {"max_abs_plane_difference": plane_diff, "rows_are_rne_of_own_param_plane": bool((rn == own).all()),
                "rows_within_one_bf16_ulp": bool(((a - b).abs() <= ulp).all())}

    verified = {"clip": compare(run_once(adamw_ag), run_once(torch_clip_ag)),
                "noclip": compare(run_once(adamw_ag_noclip), run_once(torch_noclip_ag)),
                "tolerance": TOL}
    run_once(adamw_ag)
    verified["info"] = [float(x) for x in info.cpu()]
    ok = all(max(verified[k]["max_abs_plane_difference"].values()) <= TOL and verified[k]["rows_are_rne_of_own_param_plane"]
             and verified[k]["rows_within_one_bf16_ulp"] for k in ("clip", "noclip")) and 0.0 < verified["info"][1] < 1.0
    for arm in (step_adamw, step_torch, ag_alone):
        run_once(arm)
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

    launches = {}
    for k, a in arms.items():   # the LIBRARY's launches of each arm, by its trace (torch's own kernels are not in it)
        with t.launch_trace() as tr:
            with torch.cuda.stream(s):
                a()
        launches[k] = tr.count
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

    def versus(new, ref):
        a, b = res[new], res[ref]
        return {"new": new, "reference": ref, "reference_over_new": round(b["median_us"] / a["median_us"], 3),
                "new_below_reference": a["median_us"] < b["median_us"],
                "new_median_outside_reference_range": not (b["min_us"] <= a["median_us"] <= b["max_us"])}

    out = {
        "shape": {"algo": "swing", "side": SIDE, "ranks": P, "buckets": BUCKETS, "tiles_per_rank": TILES,
                  "bytes_per_rank_per_bucket": 2 * n, "rank_stride": stride,
                  "flat_planes": f"four of {P} rows of F = {F} floats; bucket i at column {blk} i, shard_stride = F"},
        "mode": "graph", "hyper": {"lr": LR, "betas": BETAS, "eps": EPS, "weight_decay": WD, "step": STEP, "max_norm": MAX_NORM},
        "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS,
        "library_launches_per_call": launches,
        "arms": res,
        "comparisons": [versus("adamw_ag", "torch_clip_ag"), versus("adamw_ag_noclip", "torch_noclip_ag"),
                        versus("step_adamw", "step_torch")],
        "update_costs_us_over_ag_alone": round(res["adamw_ag"]["median_us"] - res["ag_alone"]["median_us"], 3),
        "session": "one session on one MI355X; eager calls are not measured",
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
