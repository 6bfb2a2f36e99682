"""Reduce-scatter / all-gather microbench at BASELINE config 2's shape: 8x8 Swing,
64 ranks x 327,680 bf16, rows at preferred_rank_stride, one GPU.

Arms, alternated in one process, ROUNDS rounds, median and spread per arm:
  a  Plan.execute (fused BO allreduce)        reads P rows, writes P rows
  b  Plan.reduce_scatter in place             reads P rows, writes one row's worth
  c  Plan.all_gather in place                 reads one row's worth, writes P rows
  d  tree_reduce (one tree, one row out)      the traffic of b
  e  broadcast (one row to P rows)            the traffic of c
Bars, each against the comparator of the same run: b <= 1.05 d, c <= 1.05 e.
b + c against a is reported for information.

A round times each arm over WINDOWS windows of CALLS calls between device events;
the pristine bucket (values near 2^-120, so 32 in-place allreduces of 64 ranks stay
finite) is restored before every window, outside the events.  After timing, b then c
on the pristine data is compared with a's bits ("verified").  Writes one JSON
(default profiles/rs_ag_config2.json, --out PATH) and prints it.
--ag-grids G ...: extra arms, c with the all-gather's grid capped at G workgroups
(tune pipe_grid), for information."""
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

SIDE, P, N = 8, 64, 327680
ROUNDS, WINDOWS, CALLS, WARMUP = 5, 7, 32, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rs_ag_config2.json"))
    ap.add_argument("--ag-grids", type=int, nargs="*", default=[])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream()
    stride = t.preferred_rank_stride(N)
    rng = np.random.default_rng(2)
    host = np.zeros((P, stride), dtype=np.uint16)
    host[:, :N] = rng.integers(0x0380, 0x0400, (P, N))   # bf16 in [2^-120, 2^-119)
    pristine = torch.from_numpy(host.view(np.int16)).to(dev)
    buf = pristine.clone()
    row = torch.zeros(N, dtype=torch.int16, device=dev)           # d's output / e's source
    row.copy_(pristine[0, :N])
    plan = t.Plan(t.SWING, t.BO, SIDE, N, P, t.EXEC_FUSED)
    arms = {
        "a_allreduce": lambda: plan.execute(buf.data_ptr(), stride, None, s),
        "b_reduce_scatter": lambda: plan.reduce_scatter(buf.data_ptr(), stride, stream=s),
        "c_all_gather": lambda: plan.all_gather(buf.data_ptr(), stride, stream=s),
        "d_tree_reduce": lambda: t.tree_reduce(buf.data_ptr(), stride, N, t.SWING, SIDE, P, row.data_ptr(), s),
        "e_broadcast": lambda: t.broadcast(buf.data_ptr(), stride, N, P, row.data_ptr(), s),
    }

    # --ag-grids G ...: c again with the all-gather's grid capped at G workgroups (tune pipe_grid)
    for g in args.ag_grids:
        arms[f"c_all_gather_grid{g}"] = arms["c_all_gather"]

    def window(call, calls, grid=0):
        with t.tuned(pipe_grid=grid):
            return window_us(call, calls)

    def window_us(call, calls):
        buf.copy_(pristine)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(calls):
            call()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    grid_of = {k: int(k.split("grid")[1]) if "grid" in k else 0 for k in arms}
    for k, call in arms.items():
        window(call, WARMUP, grid_of[k])
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, call in arms.items():
            us[k].append(sum(window(call, CALLS, grid_of[k]) for _ in range(WINDOWS)) / (WINDOWS * CALLS))

    # b then c against a's bits, on the pristine data
    want = pristine.clone()
    plan.execute(want.data_ptr(), stride, None, s)
    buf.copy_(pristine)
    plan.reduce_scatter(buf.data_ptr(), stride, stream=s)
    plan.all_gather(buf.data_ptr(), stride, stream=s)
    torch.cuda.synchronize()
    verified = bool(torch.equal(buf, want))
    plan.close()

    med = {k: statistics.median(v) for k, v in us.items()}
    bytes_moved = {k: (2 * P if k == "a_allreduce" else P + 1) * N * 2 for k in arms}
    out = {
        "shape": {"algo": "swing", "side": SIDE, "ranks": P, "elems_per_rank": N, "rank_stride": stride},
        "rounds": ROUNDS, "calls_per_arm_per_round": WINDOWS * CALLS, "warmup_calls": WARMUP,
        "arms": {k: {"median_us": round(med[k], 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
                     "rounds_us": [round(x, 3) for x in v],
                     "TBps": round(bytes_moved[k] / (med[k] * 1e-6) / 1e12, 3)} for k, v in us.items()},
        "b_over_d": round(med["b_reduce_scatter"] / med["d_tree_reduce"], 4),
        "c_over_e": round(med["c_all_gather"] / med["e_broadcast"], 4),
        "bar": 1.05,
        "b_plus_c_over_a": round((med["b_reduce_scatter"] + med["c_all_gather"]) / med["a_allreduce"], 4),
        "verified": verified,
    }
    out["b_within_bar"] = out["b_over_d"] <= 1.05
    out["c_within_bar"] = out["c_over_e"] <= 1.05
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    print("verified" if verified else "NOT verified: reduce_scatter + all_gather differ from execute")
    return 0 if verified else 1


if __name__ == "__main__":
    sys.exit(main())
