"""The peer-window (N-GPU) routes, one entry per kernel route (data only; no GPU, no library needed).

The twin of tests/route_cases.py for csrc/peer_kernels.hip: every entry names a program, the knobs
and tune keys that steer it, a shape as a function of the world size W, and the EXPECTED LAUNCH
TRACE of one rank's call or calls, written down from csrc/peer.cpp.  tests/test_gpu_peer_hard.py
runs each entry on tests/hard_inputs.py with every buffer compared whole around sentinel guards;
tests/test_peer_table.py checks, on the CPU, that every __global__ kernel of peer_kernels.hip and
every compiled k_hier_* instance has an entry here.

Why the trace: allred_peer_allreduce and allred_peer_dist_allreduce pick a form from the knobs AND
from conditions nobody sets (uncached flags and windows, the LL area holding the bucket), and fall
back to the window forms without a word.  A case that names k_peer_mem_ll and ran k_peer_oneshot
fails on its trace.

Fields:
  id
  program     mem | hier | hier_x2 | dist_bo | dist_lo
              mem      allred_peer_allreduce, one bucket per GPU
              hier     the same with 64 local ranks (8x8 Swing tree per GPU)
              hier_x2  allred_peer_allreduce_pipelined2: `calls` buckets, then the flush
              dist_*   allred_peer_dist_allreduce (BO / LO program over the GPU grid of test_dist_host.GRIDS)
  knobs       oneshot_max, mem_ll_max, hier_ll, lo_ll_max, sched_push (allred_peer_set_*) and
              max_groups: FULL (one grid per GPU; 256 // W where the ranks share a GPU) or a number
  keys        tune keys set around the calls (hier_ws_cols, hier_ws_ahead)
  peer_fence  world -> the values of the tune key peer_fence the case runs under (the same bits)
  algo, channels, local   the dist programs' schedule, link-spreading channels and local ranks per GPU
  unit        the shape: unit * W elements per rank row
  worlds      the world sizes the case runs at
  calls       back-to-back calls inside one trace (no host sync between them)
  before      the call that precedes the traced ones, itself traced first: None or "mem_oneshot"
              (it reads every rank's window, so the next scheduled call needs the full barrier)
  trace       the kernel names t.launch_trace() must report for one rank, `before` included
"""
SWING, RECDUB, RECDUB_1D, SWING_1D = 1, 0, 2, 3     # ALLRED_SWING ...
PROGRAMS = ("mem", "hier", "hier_x2", "dist_bo", "dist_lo")
FULL = "full"
NEVER, ALWAYS = 0, 1 << 40                          # a byte limit no bucket / every bucket is under
LO_LL_DEFAULT = 256 << 10                           # allred_peer's own lo_ll_max

ALL_WORLDS = (1, 2, 4, 8)
MULTI = (2, 4, 8)
# the fenced forms give the same bits and the same launches: once, at a world where the order shows
PEER_FENCE = {1: (0,), 2: (0,), 4: (0, 1), 8: (0,)}

# k_peer_oneshot gets three workgroups with a ragged last chunk out of a block of 131 vectors, and
# k_peer_ag's 4-way unroll a tail
MEM_UNIT = 8 * 131
# 64 local ranks: 3 tiles per owner; 20 per owner for the cases that give ONE workgroup every tile, so
# owned partials past the 16 LDS slots of k_hier_ws go through the own inbox and k_hier_x2 stages
# results in chunks of 8
HIER_UNIT, HIER_RING_UNIT = 256 * 3, 256 * 20
DIST_UNIT = 8 * 16 * 3                              # tests/test_gpu_peer.py's dist shape
LOCAL_HIER = 64

MEM_LAUNCHES = ["k_copy_ranks", "k_peer_barrier", "k_peer_rs", "k_peer_barrier", "k_peer_ag"]
MEM_FORMS = {   # name -> (knobs, trace of one call)
    "launches": ({"oneshot_max": NEVER, "mem_ll_max": NEVER}, MEM_LAUNCHES),
    "oneshot": ({"oneshot_max": ALWAYS, "mem_ll_max": NEVER}, ["k_peer_oneshot"]),
    "ll": ({"oneshot_max": NEVER, "mem_ll_max": ALWAYS}, ["k_peer_mem_ll"]),
}

HIER_WS = [(a, cw) for a in (1, 2) for cw in (8, 16, 32)]          # every compiled k_hier_ws<A, CW>
HIER_X2 = ["k_hier_x2", "k_hier_x2<chunked>"]

CASES = []


def case(id, program, unit, trace, calls=2, worlds=ALL_WORLDS, knobs=None, keys=None, algo=SWING, channels=1,
         local=1, before=None):
    assert program in PROGRAMS and all(c["id"] != id for c in CASES), id
    k = {"oneshot_max": NEVER, "mem_ll_max": NEVER, "hier_ll": 0, "lo_ll_max": NEVER, "sched_push": 0,
         "max_groups": FULL}
    k.update(knobs or {})
    CASES.append({"id": id, "program": program, "unit": unit, "trace": list(trace), "calls": calls,
                  "worlds": tuple(worlds), "knobs": k, "keys": dict(keys or {}), "peer_fence": PEER_FENCE,
                  "algo": algo, "channels": channels, "local": local, "before": before})


def elems(c, world):
    return c["unit"] * world


# ------------------------------------------------------------------ mem_2D, one bucket per GPU
for form, (knobs, one) in MEM_FORMS.items():
    case(f"mem-{form}", "mem", MEM_UNIT, one * 2, knobs=knobs)

# ------------------------------------------------------------------ 64 local ranks, one launch (k_hier_ws)
# W = 2 cannot show an add order (two addends commute) and is there for the transport: every instance
# with a full grid, the one-workgroup forms for the default CW = 16 only (all of them at W = 1, 4, 8)
for a, cw in HIER_WS:
    name, keys = f"k_hier_ws<{a}, {cw}>", {"hier_ws_ahead": a, "hier_ws_cols": cw}
    capped = ALL_WORLDS if cw == 16 else (1, 4, 8)
    case(f"hier-ws-a{a}-c{cw}", "hier", HIER_UNIT, [name] * 2, knobs={"hier_ll": 1}, keys=keys, local=LOCAL_HIER)
    case(f"hier-ws-a{a}-c{cw}-one-group", "hier", HIER_UNIT, [name] * 2, knobs={"hier_ll": 1, "max_groups": 1},
         keys=keys, local=LOCAL_HIER, worlds=capped)
    case(f"hier-ws-a{a}-c{cw}-ring", "hier", HIER_RING_UNIT, [name] * 2, knobs={"hier_ll": 1, "max_groups": 1},
         keys=keys, local=LOCAL_HIER, worlds=capped)
# the launch form: the tree of local rank 0 (3 W whole tiles: one tile per workgroup), the mem_2D
# exchange of the partials in each of its forms, the result to the 64 rows
for form, (knobs, one) in MEM_FORMS.items():
    case(f"hier-launch-{form}", "hier", HIER_UNIT, (["k_tree_lds<64, false>"] + one + ["k_broadcast"]) * 2,
         knobs={**knobs, "hier_ll": 0}, local=LOCAL_HIER)
# two buckets deep: three buckets and the flush are four launches; one tile per workgroup, and 20 W
# tiles in one workgroup (more than a chunk of 8: the chunked instance)
case("hier-x2", "hier_x2", HIER_UNIT, ["k_hier_x2"] * 4, calls=3, local=LOCAL_HIER)
case("hier-x2-chunked", "hier_x2", HIER_RING_UNIT, ["k_hier_x2<chunked>"] * 4, calls=3, knobs={"max_groups": 1},
     local=LOCAL_HIER)


# ------------------------------------------------------------------ the scheduled programs
def dist_cases(world):
    """tests/test_dist_host.py::cases(world), restated (tests/test_peer_table.py holds the two equal)"""
    out, cmax = [], world - 1
    for variant in ("bo", "lo"):
        out.append((variant, SWING_1D, 1, 1))
        out.append((variant, RECDUB_1D, 1, cmax))
        for algo in (RECDUB, SWING):
            out.append((variant, algo, 1, 1))
            out.append((variant, algo, 4, 1))
            if cmax > 1:
                out.append((variant, algo, 1, cmax))
                out.append((variant, algo, 4, 2))
    return out


def dist_trace(kernel, local, barrier):
    """the mem_2D call in front, then two scheduled calls: only the first follows a call that read every
    window (last_all_peer), so only it is preceded by the full barrier; k_peer_lo_ll touches no window
    and never needs it.  4 local ranks: the register tree in front, the broadcast behind."""
    pre, post = (["k_tree<4, false>"], ["k_broadcast"]) if local > 1 else ([], [])
    return (["k_peer_oneshot"] + pre + (["k_peer_barrier"] if barrier else []) + [kernel] + post +
            pre + [kernel] + post)


ALGO_NAME = {SWING: "swing", RECDUB: "recdub", RECDUB_1D: "recdub1d", SWING_1D: "swing1d"}
for world in MULTI:
    for variant, algo, local, chans in dist_cases(world):
        tag = f"{ALGO_NAME[algo]}-l{local}-c{chans}-w{world}"
        common = dict(worlds=(world,), algo=algo, channels=chans, local=local, before="mem_oneshot")
        front = {"oneshot_max": ALWAYS}   # the form of the mem_2D call in front
        # every program pulled by the receiver
        case(f"dist-{variant}-sched-{tag}", f"dist_{variant}", DIST_UNIT, dist_trace("k_peer_sched", local, True),
             knobs=front, **common)
        if variant == "bo":   # pushed by the sender
            case(f"dist-bo-push-{tag}", "dist_bo", DIST_UNIT, dist_trace("k_peer_sched_push", local, True),
                 knobs={**front, "sched_push": 1}, **common)
        elif chans == 1:      # one-channel LO buckets this small: LL pushes (every schedule here with
            #                   more than one channel requested is an XOR schedule and gets them)
            case(f"dist-lo-ll-{tag}", "dist_lo", DIST_UNIT, dist_trace("k_peer_lo_ll", local, False),
                 knobs={**front, "lo_ll_max": LO_LL_DEFAULT}, **common)

# every name a trace may hold, beside the k_hier_* instances: the kernels of peer_kernels.hip ...
PEER_KERNELS = ["k_peer_barrier", "k_peer_rs", "k_peer_ag", "k_peer_oneshot", "k_peer_sched", "k_peer_sched_push",
                "k_peer_mem_ll", "k_peer_lo_ll"]
# ... and the one-GPU engine's kernels the launch forms run around them (tests/route_cases.py)
ENGINE_KERNELS = ["k_copy_ranks", "k_tree_lds<64, false>", "k_tree<4, false>", "k_broadcast"]
