"""The one-GPU engine's routes, one entry per kernel route (data only; no GPU, no library needed).

Every entry names an operation, a shape, the tune keys that steer it, and the EXPECTED LAUNCH
TRACE: the ordered kernel names t.launch_trace() must report.  tests/test_gpu_routes.py runs each
entry on hard inputs with every buffer compared whole; tests/test_route_table.py checks, on the
CPU, that every __global__ kernel of csrc/kernels.hip and every rank count a template is
instantiated for has an entry here.

Shapes are the smallest that reach the route and still exercise its indexing: several tiles or
slices per block, odd counts, and — for persistent grids — pipe_grid of 3 to 7 so that a
workgroup loops over at least 3 tiles with a ragged tail.

Fields: id, op, algo, variant, side, total, n (elements per rank), exec, acc (mem_accum), host
(rank rows in pinned host memory), keys (tune keys, set before the plan is created), trace, and
for the grouped operations `buckets`: a list of (n, has_shard).
"""
SWING, RECDUB, RECDUB_1D, SWING_1D = 1, 0, 2, 3     # ALLRED_SWING ...
BO, LO, MEM = 0, 1, 2                               # ALLRED_BO ...
STEPS, FUSED = 0, 1                                 # ALLRED_EXEC_*
FP32, BF16 = 0, 1                                   # ALLRED_ACC_*

OPS = ("allreduce", "rs_inplace", "rs_compact", "ag_inplace", "ag_from_in", "group_exec", "group_rs", "shard_rs",
       "shard_ag", "tree_bcast")

SIDE = {1: 1, 2: 2, 4: 2, 8: 4, 16: 4, 32: 8, 64: 8}   # the valid 2D grid (side, total) of every rank count
ALL_RANKS = [1, 2, 4, 8, 16, 32, 64]
R8_64 = [8, 16, 32, 64]
R4_64 = [4, 8, 16, 32, 64]
R2_64 = [2, 4, 8, 16, 32, 64]

CASES = []


def case(id, op, total, n, trace, algo=SWING, variant=BO, side=None, exec=FUSED, acc=FP32, host=False, keys=None,
         buckets=None):
    assert op in OPS and all(c["id"] != id for c in CASES), id
    CASES.append({"id": id, "op": op, "algo": algo, "variant": variant, "side": SIDE[total] if side is None else side,
                  "total": total, "n": n, "exec": exec, "acc": acc, "host": host, "keys": dict(keys or {}),
                  "trace": list(trace), "buckets": buckets})


def tf(b):
    return "true" if b else "false"


# The rank counts every rank-templated kernel is instantiated for, by launch site.  A pattern's P
# is the rank count; tests/test_route_table.py holds the table's coverage against these ranges.
RANGES = {
    "k_tree<P, true>": ALL_RANKS,                       # tree_dispatch<true>: for_ranks<1, 64>
    "k_tree<P, false>": ALL_RANKS,                      # tree_dispatch<false>: for_ranks<1, 64>
    "k_tree_lds<P, true>": R8_64,                       # tree_dispatch<true>: for_ranks<8, 64>
    "k_tree_lds<P, false>": R8_64,                      # tree_dispatch<false>: for_ranks<8, 64>
    "k_tree_lds_pipe<P, true>": R8_64,                  # launch_tree_fused: for_ranks<8, 64>
    "k_tree_lds_pipe<P, false>": R8_64,                 # tree_dispatch<false>: for_ranks<8, 64>
    "k_tree_lds_lag<P>": [64],                          # launch_tree_fused: the one instance
    "k_tree_group<P, true>": R8_64,                     # launch_tree_group flush: for_ranks<8, 64>
    "k_tree_group<P, false>": R8_64,                    # launch_tree_group / launch_shard_group flush
    "k_tree_group<P, false, GroupShards>": R8_64,       # launch_shard_group flush: for_ranks<8, 64>
    "k_ag_group<P>": R8_64,                             # launch_shard_group flush: for_ranks<8, 64>
    "k_butterfly<P, 1>": R2_64,                         # launch_butterfly: for_ranks<2, 64>
    "k_mem_lds<P, false>": R4_64,                       # mem_fused_impl / mem_reduce_impl: for_ranks<4, 64>
    "k_mem_lds<P, true>": R4_64,
    "k_steps_reg<P, true, 3>": R8_64,                   # launch_steps_reg: for_ranks<8, 64> x BO x MINW
    "k_steps_reg<P, true, 4>": R8_64,
    "k_steps_reg<P, true, 5>": R8_64,
    "k_steps_reg<P, false, 3>": R8_64,
    "k_steps_reg<P, false, 4>": R8_64,
    "k_steps_reg<P, false, 5>": R8_64,
}
# Names without a rank range that must each head at least one trace entry.  k_butterfly<P, 8> is
# instantiated for P 2..64 beside k_butterfly<P, 1> (launch_butterfly); it shares the kernel body
# and differs in the unroll only, and its smallest shape grows as 64 / P, so ONE rank count below
# 64 stands for it.
FIXED = [
    "k_butterfly<8, 8>", "k_butterfly_lds64", "k_butterfly_lds64_pipe<0>", "k_butterfly_lds64_pipe<4>",
    "k_lo_dag_reg<LoDag0>", "k_lo_dag_reg<LoDag1>", "k_lo_dag_reg<LoDag2>",   # TSA_LO_DAGS (build/lo_dag_gen.inc)
    "k_tree_bcast_x<0, false>", "k_tree_bcast_x<0, true>", "k_tree_bcast_x<1, false>", "k_tree_bcast_x<1, true>",
    "k_mem<true, 8, false>", "k_mem<true, 8, true>", "k_mem<false, 16, false>", "k_mem<false, 16, true>",
    "k_mem_lds_lag<false>", "k_mem_lds_lag<true>", "k_broadcast", "k_ag", "k_bo_steps", "k_lo_steps",
    "k_step_w<true, 8>", "k_step_w<false, 8>", "k_lo_step", "k_copy_ranks",
]
# kernels of kernels.hip that no plan route launches: where each is tested
EXEMPT = {
    "k_add": "tests/test_gpu_parity.py (allred_bf16_add against the oracle's add, special values included)",
    "k_add_scalar": "tests/test_gpu_parity.py (allred_bf16_add: unaligned pointers and tails)",
    "k_add_segs": "tests/test_gpu_parity.py (allred_bf16_add_masked)",
    "k_validate": "tests/test_gpu_validate_device.py",
}

# vectors (8 elements) per block that make the register tree k_tree run several workgroups at every
# rank count (a wave covers 64 / max(1, P / 8) vectors) without being whole 32-vector tiles
REG_BV = {1: 517, 2: 259, 4: 131, 8: 67, 16: 37, 32: 5, 64: 5}
WHOLE = 3          # 256-element tiles per block of the whole-tile shapes: 3 P tiles
LOOP = {"pipe_grid": 5}   # a persistent grid of 5: 24 .. 192 tiles, every workgroup loops, the tail is ragged
T1088 = 1088 * 256        # 64 ranks, 17 tiles per block: the smallest odd shape of the >= 1024-tile routes

# ------------------------------------------------------------------ BO fused
for P in ALL_RANKS:
    case(f"bo-fused-reg-{P}", "allreduce", P, 8 * P * REG_BV[P], [f"k_tree<{P}, true>"])
for P in R8_64:
    case(f"bo-fused-lds-{P}", "allreduce", P, 256 * P * WHOLE, [f"k_tree_lds<{P}, true>"])
    case(f"bo-fused-pipe-{P}", "allreduce", P, 256 * P * WHOLE, [f"k_tree_lds_pipe<{P}, true>"],
         keys={"fused_form": 3, **LOOP})
case("bo-fused-pipe-host-16", "allreduce", 16, 256 * 16 * WHOLE, ["k_tree_lds_pipe<16, true>"], host=True, keys=LOOP)
case("bo-fused-lag-1088", "allreduce", 64, T1088, ["k_tree_lds_lag<64>"])
case("bo-fused-lag-2176-chunked", "allreduce", 64, 2176 * 256, ["k_tree_lds_lag<64>"] * 3,
     keys={"fused_chunk_tiles": 725})
case("bo-fused-recdub-lds-64", "allreduce", 64, 256 * 64 * WHOLE, ["k_tree_lds<64, true>"], algo=RECDUB)

# ------------------------------------------------------------------ reduce-scatter and the partial
case("rs-inplace-one-rank", "rs_inplace", 1, 8 * REG_BV[1], [])        # rank 0 owns its block: nothing enqueued
for P in ALL_RANKS:
    if P > 1:
        case(f"rs-inplace-reg-{P}", "rs_inplace", P, 8 * P * REG_BV[P], [f"k_tree<{P}, false>"])
    case(f"rs-compact-reg-{P}", "rs_compact", P, 8 * P * REG_BV[P], [f"k_tree<{P}, false>"])
for P in R8_64:
    for op in ("rs_inplace", "rs_compact"):
        case(f"{op}-lds-{P}", op, P, 256 * P * WHOLE, [f"k_tree_lds<{P}, false>"])
        case(f"{op}-pipe-{P}", op, P, 256 * P * WHOLE, [f"k_tree_lds_pipe<{P}, false>"],
             keys={"fused_form": 3, **LOOP})
case("rs-inplace-pipe-1088", "rs_inplace", 64, T1088, ["k_tree_lds_pipe<64, false>"])
# block_vec == 0 (tree 0 over the whole vector) through tree_broadcast_pipelined
for lag in (0, 1):
    for bal in (0, 1):
        case(f"tree-bcast-x-lag{lag}-bal{bal}", "tree_bcast", 64, 256 * 7, [f"k_tree_bcast_x<{lag}, {tf(bal)}>"],
             keys={"tree_bcast_lag": lag, "tree_bcast_bal": bal, "pipe_grid": 3})
case("tree-bcast-two-launches-64", "tree_bcast", 64, 8 * 261, ["k_broadcast", "k_tree<64, false>"])
case("tree-bcast-two-launches-8", "tree_bcast", 8, 256 * 6, ["k_broadcast", "k_tree_lds<8, false>"], algo=RECDUB)

# ------------------------------------------------------------------ all-gather
# blocks of 9 vectors: 7 or 8 blocks inside one 64-vector run, n_vec no multiple of 64 below 64 ranks
case("ag-inplace-one-rank", "ag_inplace", 1, 8 * 9, [])
for P in (2, 8, 16, 64):
    case(f"ag-inplace-{P}", "ag_inplace", P, 8 * P * 9, ["k_ag"])
for P in (1, 2, 8, 16, 64):
    case(f"ag-from-in-{P}", "ag_from_in", P, 8 * P * 9, ["k_ag"])
case("ag-inplace-loop-16", "ag_inplace", 16, 8 * 16 * 67, ["k_ag"], keys={"pipe_grid": 3})

# ------------------------------------------------------------------ groups
GROUP3 = [1, 3, 2]   # tiles per block of the three buckets
for P in R8_64:
    ns = [256 * P * k for k in GROUP3]
    case(f"group-exec-{P}", "group_exec", P, 8 * P, [f"k_tree_group<{P}, true>"], keys=LOOP,
         buckets=[(n, False) for n in ns])
    case(f"group-rs-{P}", "group_rs", P, 8 * P, [f"k_tree_group<{P}, false>"], keys=LOOP,
         buckets=[(n, False) for n in ns])
    case(f"shard-rs-{P}", "shard_rs", P, 8 * P, [f"k_tree_group<{P}, false, GroupShards>"], keys=LOOP,
         buckets=[(ns[0], False), (ns[1], True), (ns[2], False)])
    case(f"shard-rs-no-shard-{P}", "shard_rs", P, 8 * P, [f"k_tree_group<{P}, false>"], keys=LOOP,
         buckets=[(n, False) for n in ns])
    case(f"shard-ag-{P}", "shard_ag", P, 8 * P, [f"k_ag_group<{P}>"], keys=LOOP,
         buckets=[(ns[0], True), (ns[1], False), (ns[2], True)])
# a grouped bucket, one that is not whole tiles, a 1024-tile 64-rank bucket, a grouped bucket: the two
# own-route buckets launch at their place in the list, the group when its last member is reached
MIXED = [(256 * 64 * 2, False), (8 * 64 * 5, False), (1024 * 256, False), (256 * 64, False)]
case("group-exec-mixed-64", "group_exec", 64, 8 * 64, ["k_tree<64, true>", "k_tree_lds_lag<64>", "k_tree_group<64, true>"],
     buckets=MIXED)
case("group-rs-mixed-64", "group_rs", 64, 8 * 64,
     ["k_tree<64, false>", "k_tree_lds_pipe<64, false>", "k_tree_group<64, false>"], buckets=MIXED)
case("shard-ag-mixed-64", "shard_ag", 64, 8 * 64, ["k_ag", "k_ag", "k_ag_group<64>"],
     buckets=[(256 * 64 * 2, False), (8 * 64 * 5, True), (1024 * 256, False), (256 * 64, True)])

# ------------------------------------------------------------------ LO fused
DAG_KEYS = {"lo_dag_reg_min_tiles": 1, "pipe_grid": 3}
case("lo-dag-reg-swing-32", "allreduce", 32, 256 * 7, ["k_lo_dag_reg<LoDag0>"], variant=LO, keys=DAG_KEYS)
case("lo-dag-reg-swing-64", "allreduce", 64, 256 * 7, ["k_lo_dag_reg<LoDag1>"], variant=LO, keys=DAG_KEYS)
case("lo-dag-reg-swing1d-32", "allreduce", 32, 256 * 7, ["k_lo_dag_reg<LoDag2>"], variant=LO, algo=SWING_1D, side=1,
     keys=DAG_KEYS)
case("lo-one-rank-butterfly", "allreduce", 1, 8 * 333, [], variant=LO, keys={"lo_tree": 0})   # nothing to reduce
case("lo-one-rank-tree", "allreduce", 1, 8 * 333, ["k_tree<1, true>"], variant=LO)
for P in R2_64:
    case(f"lo-butterfly-{P}", "allreduce", P, 8 * 333, [f"k_butterfly<{P}, 1>"], variant=LO, keys={"lo_tree": 0})
case("lo-butterfly-recdub-64", "allreduce", 64, 8 * 333, ["k_butterfly<64, 1>"], variant=LO, algo=RECDUB)   # below lo_tree_min_tiles
case("lo-butterfly-u8-8", "allreduce", 8, 8 * (65536 + 3), ["k_butterfly<8, 8>"], variant=LO, keys={"lo_tree": 0})
NO_DAG = {"lo_dag": 0, "lo_dag_reg": 0}
case("lo-butterfly-lds64", "allreduce", 64, 256 * 259, ["k_butterfly_lds64"], variant=LO, keys=NO_DAG)
case("lo-butterfly-lds64-pipe0", "allreduce", 64, 256 * 259, ["k_butterfly_lds64_pipe<0>"], variant=LO,
     keys={**NO_DAG, "fused_form": 3, "pipe_grid": 7})
case("lo-butterfly-lds64-pipe4", "allreduce", 64, 256 * 7, ["k_butterfly_lds64_pipe<4>"], variant=LO,
     keys={"lo_dag_reg": 0, "lo_dag_min_tiles": 1, "pipe_grid": 3})
case("lo-tree-recdub-64", "allreduce", 64, 256 * 64, ["k_tree_lds<64, true>"], variant=LO, algo=RECDUB)
case("lo-tree-swing-16", "allreduce", 16, 8 * 16 * REG_BV[16], ["k_tree<16, true>"], variant=LO)

# ------------------------------------------------------------------ MEM
for acc in (FP32, BF16):
    a, A = ("fp32", "false") if acc == FP32 else ("bf16", "true")
    case(f"mem-fused-reg-2-{a}", "allreduce", 2, 8 * 2 * 259, [f"k_mem<true, 8, {A}>"], variant=MEM, acc=acc)
    case(f"mem-fused-reg-8-{a}", "allreduce", 8, 8 * 8 * 67, [f"k_mem<true, 8, {A}>"], variant=MEM, acc=acc)
    for P in R4_64:
        case(f"mem-fused-lds-{P}-{a}", "allreduce", P, 256 * P * WHOLE, [f"k_mem_lds<{P}, {A}>"], variant=MEM, acc=acc)
    case(f"mem-fused-lag-1088-{a}", "allreduce", 64, T1088, [f"k_mem_lds_lag<{A}>"], variant=MEM, acc=acc)
    for P in (8, 64):
        case(f"mem-steps-lds-{P}-{a}", "allreduce", P, 256 * P * WHOLE, [f"k_mem_lds<{P}, {A}>", "k_broadcast"],
             variant=MEM, exec=STEPS, acc=acc)
    case(f"mem-steps-reg-8-{a}", "allreduce", 8, 256 * 8 * WHOLE, [f"k_mem<false, 16, {A}>", "k_broadcast"],
         variant=MEM, exec=STEPS, acc=acc, keys={"mem_reduce_lds": 0})
    case(f"mem-steps-reg-2-{a}", "allreduce", 2, 8 * 2 * 259, [f"k_mem<false, 16, {A}>", "k_broadcast"],
         variant=MEM, exec=STEPS, acc=acc)

# ------------------------------------------------------------------ schedule form
for P in R8_64:
    for minw, bo_keys, lo_keys in ((3, {}, {"steps_groups": 3}), (4, {"steps_groups": 4}, {}),
                                   (5, {"steps_groups": 5}, {"steps_groups": 5})):
        case(f"steps-reg-bo-{P}-w{minw}", "allreduce", P, 256 * P * WHOLE, [f"k_steps_reg<{P}, true, {minw}>"],
             exec=STEPS, keys={**bo_keys, **LOOP})
        case(f"steps-reg-lo-{P}-w{minw}", "allreduce", P, 256 * P * WHOLE, [f"k_steps_reg<{P}, false, {minw}>"],
             variant=LO, exec=STEPS, keys={**lo_keys, **LOOP})
case("steps-bo-4", "allreduce", 4, 256 * 4 * WHOLE, ["k_bo_steps"], exec=STEPS)                  # fewer than 8 ranks
case("steps-bo-narrow-8", "allreduce", 8, 8 * 8 * 67, ["k_bo_steps"], exec=STEPS)                # slices narrower than a unit
case("steps-bo-resident-16", "allreduce", 16, 256 * 16 * WHOLE, ["k_bo_steps"], exec=STEPS, keys={"steps_form": 2})
case("steps-lo-4", "allreduce", 4, 256 * 4 * WHOLE, ["k_lo_steps"], variant=LO, exec=STEPS)
case("steps-lo-narrow-16", "allreduce", 16, 8 * 333, ["k_lo_steps"], variant=LO, exec=STEPS)
for P, steps in ((8, 3), (16, 4)):   # an odd and an even step count
    case(f"steps-per-step-bo-{P}", "allreduce", P, 8 * P * REG_BV[P],
         ["k_step_w<true, 8>"] * steps + ["k_step_w<false, 8>"] * steps, exec=STEPS, keys={"steps_form": 1})
    case(f"steps-per-step-lo-{P}", "allreduce", P, 8 * 333, ["k_lo_step"] * steps + ["k_copy_ranks"] * (steps % 2),
         variant=LO, exec=STEPS, keys={"steps_form": 1})
