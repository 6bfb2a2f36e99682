"""MI355X-native allreduce engine with the capabilities of
EngineerCharlie/TenstorrentAllreduce (2D Swing / Recursive-Doubling
allreduce, bandwidth-optimal / latency-optimal / shared-memory variants).

The engine is C++/HIP (``liballred.so``, C-ABI in ``include/allred.h``) plus
the reference's executables (``bin/allred_BO_2D`` ...).  This package is a
thin Python view of that C-ABI for tests and ``bench.py``: device memory and
streams come from PyTorch (plumbing), every computation runs in the library.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Callable, Sequence

import numpy as np

from . import _lib
from ._lib import (ACC_BF16, ACC_FP32, BO, EXEC_FUSED, EXEC_STEPS, LO, MEM, MULTI_FLAT, MULTI_HIER,  # noqa: F401
                   MULTI_LOCAL, OP_ALL_GATHER, OP_REDUCE_SCATTER, RECDUB, RECDUB_1D, SWING, SWING_1D, TRANSPORT_HOST,
                   TRANSPORT_PEER, TRANSPORT_RCCL, ADAMW_PARAM_GROUPS_MAX, AllredError, Args, DistDesc, MultiOpts, MultiPlan, PlanDesc, Report, Schedule, Seg, check, lib)

__all__ = [
    "BO", "LO", "MEM", "SWING", "RECDUB", "SWING_1D", "RECDUB_1D", "get_comm_partner_swing_1D",
    "get_comm_partner_recdub_1D", "EXEC_STEPS", "EXEC_FUSED", "AllredError", "schedule",
    "highest_power_of_two", "get_step_directions", "get_comm_partner_swing_2D", "get_comm_partner_recdub_2D",
    "get_swing_block_comm_indexes", "get_recdub_block_comm_indexes", "normalize_tiles",
    "random_bf16_vector", "constant_bf16_vector", "validate_result_vector", "Plan", "preferred_rank_stride", "bf16_add",
    "bf16_add_masked", "tree_reduce", "broadcast", "parse_args", "run", "run_cli", "Comm", "dist_desc", "dist_allreduce",
    "dist_allreduce_host", "dist_allreduce_pipelined", "tree_broadcast_pipelined", "dist_workspace_bytes", "dist_program_stats", "Peer", "tune", "tuned", "last_launch", "launch_trace",
    "ACC_FP32",
    "ACC_BF16", "multi_plan", "run_multi", "TRANSPORT_RCCL", "TRANSPORT_PEER", "TRANSPORT_HOST", "MULTI_FLAT",
    "MULTI_HIER", "MULTI_LOCAL", "validate_device", "dist_reduce_scatter", "dist_all_gather",
    "dist_reduce_scatter_host", "dist_all_gather_host", "OP_REDUCE_SCATTER", "OP_ALL_GATHER",
    "adamw_hyper", "adamw_hyper_groups", "ADAMW_PARAM_GROUPS_MAX", "mxfp8_dequantize",
]


# ---------------------------------------------------------------- tuning
def tune(key: str, value: int | None = None) -> int:
    """allred_tune_set / allred_tune_get: switch between bit-identical kernel
    forms (A/B); returns the previous value.  Keys: allred.h §Tuning."""
    old = C.c_int64(0)
    check(lib.allred_tune_get(key.encode(), C.byref(old)), f"tune_get({key})")
    if value is not None:
        check(lib.allred_tune_set(key.encode(), int(value)), f"tune_set({key}={value})")
    return old.value


class tuned:
    """with tuned(key=value, ...): the keys set for the block, restored after."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = tune(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            tune(k, v)


def last_launch() -> dict:
    """allred_last_launch: the kernel this thread's last reported launch ran, the
    grid its launcher chose, its static LDS / VGPRs, the workgroups per CU that can
    be resident and the device's CU count."""
    li = _lib.LaunchInfo()
    check(lib.allred_last_launch(C.byref(li)), "last_launch")
    return {"kernel": li.kernel.decode(), "grid": li.grid, "block": li.block, "lds_bytes": li.lds_bytes,
            "vgprs": li.regs, "resident_per_cu": li.resident_per_cu, "cus": li.cus,
            "grid_resident": li.grid <= li.resident_per_cu * li.cus}


class launch_trace:
    """with launch_trace() as tr: every kernel this thread launches in the block
    (allred_launch_trace_begin / _end).  After the block: tr.kernels (the names in
    launch order, template arguments included, the first 64), tr.grids, tr.blocks
    and tr.count (all launches seen, stored or not)."""

    def __init__(self):
        self.kernels, self.grids, self.blocks, self.count = [], [], [], 0

    def __enter__(self):
        check(lib.allred_launch_trace_begin(), "launch_trace_begin")
        return self

    def __exit__(self, *exc):
        rec = (_lib.LaunchRec * _lib.TRACE_CAP)()
        n = C.c_int(0)
        check(lib.allred_launch_trace_end(rec, _lib.TRACE_CAP, C.byref(n)), "launch_trace_end")
        stored = rec[:min(n.value, _lib.TRACE_CAP)]
        self.kernels = [r.kernel.decode() for r in stored]
        self.grids = [r.grid for r in stored]
        self.blocks = [r.block for r in stored]
        self.count = n.value


# ---------------------------------------------------------------- schedule
def highest_power_of_two(v: int) -> int:  # allred_helper.cpp:122
    return lib.allred_highest_power_of_two(v)


def get_step_directions(x: int, y: int) -> int:  # allred_helper.cpp:136
    return lib.allred_get_step_directions(x, y)


def get_comm_partner_swing_2D(node, step, horizontal_step, side, total) -> int:  # allred_helper.cpp:166
    return lib.allred_get_comm_partner_swing_2d(node, step, int(bool(horizontal_step)), side, total)


def get_comm_partner_recdub_2D(node, step, horizontal_step, depth, step_directions, side):
    """allred_helper.cpp:145; returns (partner, updated step_directions)."""
    d = C.c_uint32(step_directions)
    p = lib.allred_get_comm_partner_recdub_2d(node, step, int(bool(horizontal_step)), depth, C.byref(d), side)
    return p, d.value


def get_swing_block_comm_indexes(node, step, blocks, horizontal_step, side, total) -> int:
    """allred_BO_2D.cpp:220; ORs into the 64-bit mask `blocks`, returns it."""
    b = (C.c_uint32 * 2)(blocks & 0xFFFFFFFF, blocks >> 32)
    lib.allred_get_swing_block_comm_indexes(node, step, b, int(bool(horizontal_step)), side, total)
    return b[0] | (b[1] << 32)


def get_recdub_block_comm_indexes(node, step, blocks, horizontal_step, side, total, depth, step_directions=0):
    """allred_BO_2D.cpp:242; returns (mask, step_directions)."""
    b = (C.c_uint32 * 2)(blocks & 0xFFFFFFFF, blocks >> 32)
    d = C.c_uint32(step_directions)
    lib.allred_get_recdub_block_comm_indexes(node, step, b, int(bool(horizontal_step)), side, total, depth,
                                             C.byref(d))
    return b[0] | (b[1] << 32), d.value


def get_comm_partner_swing_1D(node: int, step: int, num_nodes: int) -> int:  # all_red_swing_1D.cpp:32
    return lib.allred_get_comm_partner_swing_1d(node, step, num_nodes)


def get_comm_partner_recdub_1D(node: int, step: int, step_directions: int = 0):  # recdub_multicore_1D.cpp:165
    d = C.c_uint32(step_directions)
    p = lib.allred_get_comm_partner_recdub_1d(node, step, C.byref(d))
    return p, d.value


def normalize_tiles(tiles: int, total_nodes: int, large_buffer: bool) -> int:  # allred_helper.cpp:224
    return lib.allred_normalize_tiles(tiles, total_nodes, int(bool(large_buffer)))


def schedule(algo: int, side: int, total: int | None = None) -> dict:
    """The per-rank schedule of allred_BO_2D.cpp:75-212 (validated)."""
    total = side * side if total is None else total
    s = Schedule()
    check(lib.allred_schedule_build(algo, side, total, C.byref(s)), f"schedule({algo},{side},{total})")
    T, K = s.total, s.steps
    return {
        "algo": s.algo, "side": s.side, "total": T, "steps": K,
        "partner": [[s.partner[r][k] for k in range(K)] for r in range(T)],
        "send": [[s.send[r][k] for k in range(K)] for r in range(T)],
        "recv": [[s.recv[r][k] for k in range(K)] for r in range(T)],
        "dirs": [s.dirs[r] for r in range(T)],
        "tree_order": [[s.tree_order[x][i] for i in range(T)] for x in range(T)],
    }


# ---------------------------------------------------------------- host data
def random_bf16_vector(num_bytes: int, seed: int, rand_max: int = 100, round_mode: int = 0) -> np.ndarray:
    """tt-metal create_random_vector_of_bfloat16 (packed uint32, low half first)."""
    out = np.empty(num_bytes // 4, dtype=np.uint32)
    lib.allred_random_bf16_vector(num_bytes, rand_max, seed, round_mode, out.ctypes.data)
    return out


def constant_bf16_vector(num_bytes: int, value: float) -> np.ndarray:
    out = np.empty(num_bytes // 4, dtype=np.uint32)
    lib.allred_constant_bf16_vector(num_bytes, value, out.ctypes.data)
    return out


def validate_result_vector(result, src0, src1, num_els: int, error: float, total_nodes: int,
                           verbose: bool = False):
    """allred_helper.cpp:18-120; returns (mismatches, max_error)."""
    arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in (result, src0, src1)]
    m = C.c_float(0)
    bad = lib.allred_validate_result_vector(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data,
                                            num_els, error, total_nodes, int(verbose), C.byref(m))
    return int(bad), float(m.value)


def adamw_hyper(lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, step: int = 1,
                max_norm: float = float("inf")) -> np.ndarray:
    """allred_adamw_hyper for optimizer step `step` (1-based) as eight float32: lr, beta1, beta2, eps,
    weight_decay, 1 - beta1^step, sqrt(1 - beta2^step), max_norm.  The bias corrections are computed in
    float64 and rounded once.  Copy the 32 bytes to device memory (16-byte aligned) before the call."""
    b1, b2 = float(betas[0]), float(betas[1])
    bc1 = 1.0 - b1 ** int(step)
    bc2_sqrt = float(np.sqrt(np.float64(1.0 - b2 ** int(step))))
    return np.array([lr, b1, b2, eps, weight_decay, bc1, bc2_sqrt, max_norm], dtype=np.float32)


def adamw_hyper_groups(groups, step: int = 1, max_norm: float = float("inf")) -> np.ndarray:
    """The hyper array of Plan.adamw_all_gather_shards_f32_groups for a list of parameter groups — dicts
    with torch.optim.AdamW's keys lr, betas, eps, weight_decay (a missing key: adamw_hyper's default) —
    as (G, 8) float32, row g made by adamw_hyper.  max_norm is the CALL's (clipping is by the global
    norm over all groups); it is written into every row, and row 0's is the one the kernel reads."""
    groups = list(groups)
    if not 1 <= len(groups) <= ADAMW_PARAM_GROUPS_MAX:
        raise ValueError(f"1 .. {ADAMW_PARAM_GROUPS_MAX} parameter groups, not {len(groups)}")
    keys = ("lr", "betas", "eps", "weight_decay")
    return np.stack([adamw_hyper(**{k: g[k] for k in keys if k in g}, step=step, max_norm=max_norm) for g in groups])


def mxfp8_dequantize(elements_u8, scales_u8) -> np.ndarray:
    """What Plan.all_gather_shards_mxfp8 wrote, as float32: e4m3fn(byte) * 2^(scale - 127), the scale of
    element k being scales_u8[..., k // 32].  elements_u8: (..., n) uint8, n % 32 == 0; scales_u8:
    (..., n / 32) uint8.  NaN for the element byte 0x7F / 0xFF and for every element under a 0xFF scale.
    Exact — every product is a float32, denormals included — with one exception: under rceil a block whose
    amax is within half an e4m3 step of 2^128 holds the element 256 at scale 2^120, which is +-Inf here."""
    e = np.asarray(elements_u8, dtype=np.uint8)
    s = np.asarray(scales_u8, dtype=np.uint8)
    if e.shape[-1] % 32 or s.shape != e.shape[:-1] + (e.shape[-1] // 32,):
        raise ValueError(f"elements {e.shape} and scales {s.shape} do not belong together")
    exp, man = ((e >> 3) & 0xF).astype(np.int32), (e & 7).astype(np.float64)
    mag = np.where(exp == 0, man * 2.0 ** -9, (1.0 + man / 8.0) * np.exp2((exp - 7).astype(np.float64)))
    val = np.where(e & 0x80, -mag, mag)
    val = np.where((e & 0x7F) == 0x7F, np.nan, val)
    scale = np.where(s == 0xFF, np.nan, np.exp2(s.astype(np.float64) - 127.0))
    with np.errstate(over="ignore"):
        return (val * np.repeat(scale, 32, axis=-1)).astype(np.float32)


# ---------------------------------------------------------------- device
def _stream_ptr(stream) -> int | None:
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream  # torch.cuda.Stream


def bf16_add(dst_ptr: int, src_ptr: int, n: int, stream=None) -> None:
    check(lib.allred_bf16_add(dst_ptr, src_ptr, n, _stream_ptr(stream)), "bf16_add")


def bf16_add_masked(dst_ptr: int, src_ptr: int, mask: int, block_elems: int, stream=None) -> None:
    check(lib.allred_bf16_add_masked(dst_ptr, src_ptr, mask, block_elems, _stream_ptr(stream)), "bf16_add_masked")


def tree_reduce(ranks_ptr: int, stride: int, n: int, algo: int, side: int, total: int, out_ptr: int,
                stream=None) -> None:
    check(lib.allred_tree_reduce(ranks_ptr, stride, n, algo, side, total, out_ptr, _stream_ptr(stream)),
          "tree_reduce")


def broadcast(ranks_ptr: int, stride: int, n: int, total: int, src_ptr: int, stream=None) -> None:
    check(lib.allred_broadcast(ranks_ptr, stride, n, total, src_ptr, _stream_ptr(stream)), "broadcast")


def preferred_rank_stride(elems: int) -> int:
    return lib.allred_preferred_rank_stride(elems)


class Plan:
    """N virtual ranks in one GPU's HBM (allred_plan_*).  exec_mode: EXEC_FUSED
    (default, one HBM pass) or EXEC_STEPS (the reference's step structure);
    mem_accum (MEM): ACC_FP32 or ACC_BF16 (the reference's bf16 dest)."""

    def __init__(self, algo: int, variant: int, side: int, elems_per_rank: int, total: int = 0,
                 exec_mode: int = EXEC_FUSED, device: int = -1, mem_accum: int = ACC_FP32):
        d = PlanDesc(algo, variant, exec_mode, side, total, device, elems_per_rank, mem_accum)
        h = C.c_void_p()
        check(lib.allred_plan_create(C.byref(d), C.byref(h)), "plan_create")
        self._h = h
        self.total = total or side * side
        self.elems = elems_per_rank
        self.workspace_bytes = lib.allred_plan_workspace_bytes(h)
        self.stamp_words = lib.allred_plan_stamp_words(h)

    @property
    def launches(self) -> int:
        """Kernel launches one execute enqueues now (fused plans: with the current tune keys)."""
        return lib.allred_plan_launches(self._h)

    def execute(self, ranks_ptr: int, stride: int, workspace_ptr: int | None = None, stream=None,
                stamps_ptr: int | None = None) -> None:
        """stamps_ptr: device memory of stamp_words uint64 (schedule form only)."""
        check(lib.allred_plan_execute_profiled(self._h, ranks_ptr, stride, workspace_ptr, stamps_ptr,
                                               _stream_ptr(stream)), "plan_execute")

    def reduce_scatter(self, ranks_ptr: int, stride: int, out_ptr: int | None = None, out_stride: int = 0,
                       workspace_ptr: int | None = None, stream=None) -> None:
        """allred_plan_reduce_scatter (BO plans): block b of the allreduce to rank b's
        row, or — fused plans — to out_ptr + b * out_stride elements, ranks only read."""
        check(lib.allred_plan_reduce_scatter(self._h, ranks_ptr, stride, out_ptr or None, out_stride, workspace_ptr,
                                             _stream_ptr(stream)), "plan_reduce_scatter")

    def all_gather(self, ranks_ptr: int, stride: int, in_ptr: int | None = None, in_stride: int = 0,
                   workspace_ptr: int | None = None, stream=None) -> None:
        """allred_plan_all_gather (BO plans): block b of rank b — or, fused plans, of
        in_ptr + b * in_stride elements — copied bit for bit to block b of every rank."""
        check(lib.allred_plan_all_gather(self._h, ranks_ptr, stride, in_ptr or None, in_stride, workspace_ptr,
                                         _stream_ptr(stream)), "plan_all_gather")

    @staticmethod
    def _buckets(buckets):
        """a sequence of (ranks_ptr, stride, elems_per_rank) as an allred_bucket array (None when empty)"""
        items = [(int(p), int(s), int(n)) for p, s, n in buckets]
        return ((_lib.Bucket * len(items))(*items) if items else None), len(items)

    def execute_group(self, buckets, stream=None) -> None:
        """allred_plan_execute_group (fused BO plans): the BO allreduce of every (ranks_ptr, stride,
        elems_per_rank) of the list, the small whole-tile buckets sharing kernel launches; the
        plan supplies the schedule only."""
        arr, count = self._buckets(buckets)
        check(lib.allred_plan_execute_group(self._h, arr, count, _stream_ptr(stream)), "plan_execute_group")

    def reduce_scatter_group(self, buckets, stream=None) -> None:
        """allred_plan_reduce_scatter_group: the in-place reduce-scatter of every bucket of the list."""
        arr, count = self._buckets(buckets)
        check(lib.allred_plan_reduce_scatter_group(self._h, arr, count, _stream_ptr(stream)),
              "plan_reduce_scatter_group")

    def group_launches(self, buckets) -> int:
        """Kernel launches execute_group would enqueue for the list now (with the current tune keys)."""
        arr, count = self._buckets(buckets)
        st = lib.allred_plan_group_launches(self._h, arr, count)
        if st < 0:
            raise AllredError(st, "plan_group_launches")
        return st

    @staticmethod
    def _shard_buckets(buckets):
        """a sequence of (ranks_ptr, stride, elems_per_rank) — in place — or (ranks_ptr, stride,
        elems_per_rank, shard_ptr, shard_stride) as an allred_shard_bucket array (None when empty)"""
        items = []
        for b in buckets:
            p, s, n = b[:3]
            shard, shard_stride = b[3:] if len(b) > 3 else (None, 0)
            items.append((int(p), int(s), int(n), int(shard) if shard else None, int(shard_stride)))
        return ((_lib.ShardBucket * len(items))(*items) if items else None), len(items)

    def reduce_scatter_shards(self, buckets, stream=None) -> None:
        """allred_plan_reduce_scatter_shards (fused BO plans): the reduce-scatter of every bucket of
        the list, block b to rank b's row (3-tuples) or to shard_ptr + b * shard_stride elements
        (5-tuples, the rank rows only read); the small whole-tile buckets share kernel launches."""
        arr, count = self._shard_buckets(buckets)
        check(lib.allred_plan_reduce_scatter_shards(self._h, arr, count, _stream_ptr(stream)),
              "plan_reduce_scatter_shards")

    def all_gather_shards(self, buckets, stream=None) -> None:
        """allred_plan_all_gather_shards: block b of rank b — or of the bucket's shard — copied bit
        for bit to block b of every rank, for every bucket of the list."""
        arr, count = self._shard_buckets(buckets)
        check(lib.allred_plan_all_gather_shards(self._h, arr, count, _stream_ptr(stream)), "plan_all_gather_shards")

    def shards_launches(self, buckets, op: int) -> int:
        """Kernel launches reduce_scatter_shards (op = OP_REDUCE_SCATTER) or all_gather_shards
        (OP_ALL_GATHER) would enqueue for the list now (with the current tune keys)."""
        arr, count = self._shard_buckets(buckets)
        st = lib.allred_plan_shards_launches(self._h, arr, count, op)
        if st < 0:
            raise AllredError(st, "plan_shards_launches")
        return st

    @staticmethod
    def _shard_buckets_f32(buckets):
        """a sequence of (ranks_ptr, stride, elems_per_rank, shard_ptr, shard_stride) — bf16 rank rows,
        an fp32 shard, its stride in floats — as an allred_shard_bucket_f32 array (None when empty)"""
        items = [(int(p), int(s), int(n), int(shard) if shard else None, int(shard_stride))
                 for p, s, n, shard, shard_stride in buckets]
        return ((_lib.ShardBucketF32 * len(items))(*items) if items else None), len(items)

    def reduce_scatter_shards_f32(self, buckets, scale: float = 1.0, accumulate: bool = False, stream=None) -> None:
        """allred_plan_reduce_scatter_shards_f32 (fused BO plans): tree b of every bucket summed in
        fp32 without intermediate rounding, times scale, stored to — accumulate: added into — the
        fp32 block at shard_ptr + b * shard_stride floats; the rank rows are only read."""
        arr, count = self._shard_buckets_f32(buckets)
        flags = _lib.SHARD_ACCUMULATE if accumulate else 0
        check(lib.allred_plan_reduce_scatter_shards_f32(self._h, arr, count, float(scale), flags, _stream_ptr(stream)),
              "plan_reduce_scatter_shards_f32")

    def all_gather_shards_f32(self, buckets, stream=None) -> None:
        """allred_plan_all_gather_shards_f32: block b of the fp32 shard rounded once to bf16 (RNE)
        into block b of every rank row, for every bucket of the list; the shards are only read."""
        arr, count = self._shard_buckets_f32(buckets)
        check(lib.allred_plan_all_gather_shards_f32(self._h, arr, count, _stream_ptr(stream)),
              "plan_all_gather_shards_f32")

    def shards_f32_launches(self, buckets, op: int) -> int:
        """Kernel launches reduce_scatter_shards_f32 (op = OP_REDUCE_SCATTER) or all_gather_shards_f32
        (OP_ALL_GATHER) would enqueue for the list: one per ALLRED_GROUP_MAX buckets."""
        arr, count = self._shard_buckets_f32(buckets)
        st = lib.allred_plan_shards_f32_launches(self._h, arr, count, op)
        if st < 0:
            raise AllredError(st, "plan_shards_f32_launches")
        return st

    def reduce_scatter_shards_f32_norm(self, buckets, norm_sq_ptr, norm_ws_ptr, scale: float = 1.0,
                                       accumulate: bool = False, stream=None) -> None:
        """allred_plan_reduce_scatter_shards_f32_norm: reduce_scatter_shards_f32 — the same shard
        bits — which also leaves, in the same launches, norm_sq[b] = the sum of the squares of what
        it stored into block b of every bucket (`total` floats at norm_sq_ptr, device).  norm_ws_ptr:
        shards_f32_norm_workspace_bytes(buckets) bytes of device memory, 16-byte aligned, the first
        64 zeroed once by the caller; one workspace is never in flight on two streams."""
        arr, count = self._shard_buckets_f32(buckets)
        flags = _lib.SHARD_ACCUMULATE if accumulate else 0
        check(lib.allred_plan_reduce_scatter_shards_f32_norm(self._h, arr, count, float(scale), flags, int(norm_sq_ptr) or None,
                                                             int(norm_ws_ptr) or None, _stream_ptr(stream)),
              "plan_reduce_scatter_shards_f32_norm")

    def shards_f32_norm_workspace_bytes(self, buckets) -> int:
        """Bytes of the workspace reduce_scatter_shards_f32_norm needs for the list: 64 + 4 per
        256-element tile of a rank row; 0 for a list the call would refuse."""
        arr, count = self._shard_buckets_f32(buckets)
        return int(lib.allred_plan_shards_f32_norm_workspace_bytes(self._h, arr, count))

    @staticmethod
    def _adamw_buckets_f32(buckets):
        """a sequence of (ranks_ptr, stride, elems_per_rank, param_ptr, grad_ptr, exp_avg_ptr, exp_avg_sq_ptr,
        shard_stride) — bf16 rank rows, four fp32 planes at one stride in floats — as an
        allred_adamw_bucket_f32 array (None when empty)"""
        items = [(int(p), int(s), int(n)) + tuple(int(x) if x else None for x in planes) + (int(shard_stride),)
                 for p, s, n, *planes, shard_stride in buckets]
        return ((_lib.AdamwBucketF32 * len(items))(*items) if items else None), len(items)

    def adamw_all_gather_shards_f32(self, buckets, hyper_ptr, norm_sq_ptr=None, info_ptr=None, zero_grad: bool = False,
                                    stream=None) -> None:
        """allred_plan_adamw_all_gather_shards_f32: the clipped AdamW step of allred.h on the fp32 planes
        of every bucket, and block b of the new parameters rounded once to bf16 into block b of every
        rank row — one launch per ALLRED_ADAMW_GROUP_MAX buckets.  hyper_ptr: the 32 bytes of
        adamw_hyper(..) in device memory, 16-byte aligned; norm_sq_ptr: what
        reduce_scatter_shards_f32_norm left (None: no clipping, no skip); info_ptr: 4 floats that
        receive {N, c, skipped, 0} (None: not wanted); zero_grad: +0.0f over every gradient read."""
        arr, count = self._adamw_buckets_f32(buckets)
        flags = _lib.ADAMW_ZERO_GRAD if zero_grad else 0
        check(lib.allred_plan_adamw_all_gather_shards_f32(self._h, arr, count, int(hyper_ptr) or None,
                                                          int(norm_sq_ptr or 0) or None, int(info_ptr or 0) or None, flags,
                                                          _stream_ptr(stream)),
              "plan_adamw_all_gather_shards_f32")

    def adamw_all_gather_shards_f32_groups(self, buckets, group_of, hyper_ptr, ngroups: int, norm_sq_ptr=None, info_ptr=None,
                                           zero_grad: bool = False, stream=None) -> None:
        """allred_plan_adamw_all_gather_shards_f32_groups: adamw_all_gather_shards_f32 with a hyperparameter
        set per parameter group, still one launch per ALLRED_ADAMW_GROUP_MAX buckets.  group_of: one
        group index per bucket (None: every bucket in group 0); hyper_ptr: the ngroups x 32 bytes of
        adamw_hyper_groups(..) in device memory, 16-byte aligned.  N, the skip and the clip
        coefficient are the call's (max_norm: row 0's); everything else is the group's."""
        arr, count = self._adamw_buckets_f32(buckets)
        groups = None
        if group_of is not None:
            if len(group_of) != count:
                raise ValueError(f"{len(group_of)} group indices for {count} buckets")
            if any(not 0 <= int(g) <= 255 for g in group_of):
                raise ValueError("a group index is one byte")
            groups = (C.c_uint8 * max(count, 1))(*[int(g) for g in group_of])
        flags = _lib.ADAMW_ZERO_GRAD if zero_grad else 0
        check(lib.allred_plan_adamw_all_gather_shards_f32_groups(self._h, arr, groups, count, int(hyper_ptr) or None, int(ngroups),
                                                                 int(norm_sq_ptr or 0) or None, int(info_ptr or 0) or None,
                                                                 flags, _stream_ptr(stream)),
              "plan_adamw_all_gather_shards_f32_groups")

    def adamw_shards_f32_launches(self, buckets) -> int:
        """Kernel launches adamw_all_gather_shards_f32 — and adamw_all_gather_shards_f32_groups, whatever
        the groups — would enqueue for the list: one per ALLRED_ADAMW_GROUP_MAX buckets."""
        arr, count = self._adamw_buckets_f32(buckets)
        st = lib.allred_plan_adamw_shards_f32_launches(self._h, arr, count)
        if st < 0:
            raise AllredError(st, "plan_adamw_shards_f32_launches")
        return st

    @staticmethod
    def _mx_buckets_f32(buckets):
        """a sequence of (rows_ptr, row_stride, scales_ptr, scale_stride, elems_per_rank, shard_ptr, shard_stride) —
        e4m3 element rows and E8M0 scale rows with strides in bytes, an fp32 shard with its stride in floats —
        as an allred_mx_bucket_f32 array (None when empty)"""
        items = [(int(rows) if rows else None, int(rs), int(scales) if scales else None, int(ss), int(n),
                  int(shard) if shard else None, int(shard_stride))
                 for rows, rs, scales, ss, n, shard, shard_stride in buckets]
        return ((_lib.MxBucketF32 * len(items))(*items) if items else None), len(items)

    def all_gather_shards_mxfp8(self, buckets, rceil: bool = False, stream=None) -> None:
        """allred_plan_all_gather_shards_mxfp8: block b of the fp32 shard quantised to OCP MXFP8 — e4m3fn
        bytes into block b of every rank's element row, one E8M0 scale byte per 32 elements into every
        rank's scale row — for every bucket of the list, one launch per ALLRED_MX_GROUP_MAX buckets; the
        shards are only read.  rceil: the scale exponent rounded up (no finite element saturates)
        instead of the OCP floor rule.  mxfp8_dequantize gives the values back."""
        arr, count = self._mx_buckets_f32(buckets)
        flags = _lib.MX_SCALE_RCEIL if rceil else 0
        check(lib.allred_plan_all_gather_shards_mxfp8(self._h, arr, count, flags, _stream_ptr(stream)),
              "plan_all_gather_shards_mxfp8")

    def shards_mxfp8_launches(self, buckets) -> int:
        """Kernel launches all_gather_shards_mxfp8 would enqueue for the list: one per ALLRED_MX_GROUP_MAX buckets."""
        arr, count = self._mx_buckets_f32(buckets)
        st = lib.allred_plan_all_gather_shards_mxfp8_launches(self._h, arr, count)
        if st < 0:
            raise AllredError(st, "plan_all_gather_shards_mxfp8_launches")
        return st

    @staticmethod
    def _mx2d_buckets_f32(buckets):
        """a sequence of (rows_ptr, row_stride, scales_ptr, scale_stride, t_rows_ptr, t_row_stride, t_scales_ptr,
        t_scale_stride, elems_per_rank, cols, shard_ptr, shard_stride) — allred_mx2d_bucket_f32's order; None (or 0)
        for rows_ptr and scales_ptr selects the column-wise outputs only — as an array of them (None when empty)"""
        items = [tuple((int(v) if v else None) if k in (0, 2, 4, 6, 10) else int(v) for k, v in enumerate(b)) for b in buckets]
        return ((_lib.Mx2dBucketF32 * len(items))(*items) if items else None), len(items)

    def all_gather_shards_mxfp8_2d(self, buckets, rceil: bool = False, stream=None) -> None:
        """allred_plan_all_gather_shards_mxfp8_2d: every bucket is ONE row-major fp32 matrix W[nrows][cols] in
        shard blocks; every rank receives what all_gather_shards_mxfp8 writes (MX blocks along cols: the operand
        of Y = X W^T) where rows are given, and always the column-wise copy — W^T as linear MX rows, MX blocks
        along the rows of W: the operand of dX = dY W — both rounded once from fp32, from one read of the shard.
        One launch per ALLRED_MX2D_GROUP_MAX buckets.  mxfp8_dequantize on the t rows gives W^T back."""
        arr, count = self._mx2d_buckets_f32(buckets)
        flags = _lib.MX_SCALE_RCEIL if rceil else 0
        check(lib.allred_plan_all_gather_shards_mxfp8_2d(self._h, arr, count, flags, _stream_ptr(stream)),
              "plan_all_gather_shards_mxfp8_2d")

    def shards_mxfp8_2d_launches(self, buckets) -> int:
        """Kernel launches all_gather_shards_mxfp8_2d would enqueue for the list: one per ALLRED_MX2D_GROUP_MAX buckets."""
        arr, count = self._mx2d_buckets_f32(buckets)
        st = lib.allred_plan_all_gather_shards_mxfp8_2d_launches(self._h, arr, count)
        if st < 0:
            raise AllredError(st, "plan_all_gather_shards_mxfp8_2d_launches")
        return st

    @staticmethod
    def _adamw_mx_buckets_f32(buckets):
        """a sequence of (rows_ptr, row_stride, scales_ptr, scale_stride, elems_per_rank, param_ptr, grad_ptr,
        exp_avg_ptr, exp_avg_sq_ptr, shard_stride) — e4m3 element rows and E8M0 scale rows with strides in
        bytes, four fp32 planes at one stride in floats — as an allred_adamw_mx_bucket_f32 array (None when empty)"""
        items = [(int(rows) if rows else None, int(rs), int(scales) if scales else None, int(ss), int(n))
                 + tuple(int(x) if x else None for x in planes) + (int(shard_stride),)
                 for rows, rs, scales, ss, n, *planes, shard_stride in buckets]
        return ((_lib.AdamwMxBucketF32 * len(items))(*items) if items else None), len(items)

    def adamw_all_gather_shards_mxfp8(self, buckets, group_of, hyper_ptr, ngroups: int, norm_sq_ptr=None, info_ptr=None,
                                      zero_grad: bool = False, rceil: bool = False, stream=None) -> None:
        """allred_plan_adamw_all_gather_shards_mxfp8: adamw_all_gather_shards_f32_groups' update of the four
        planes, with the new parameters quantised once, from fp32, to OCP MXFP8 into every rank's element
        row and scale row as all_gather_shards_mxfp8 writes them — one launch per ALLRED_ADAMW_MX_GROUP_MAX
        buckets.  group_of, hyper_ptr, ngroups, norm_sq_ptr, info_ptr and zero_grad: as the groups call
        (ngroups = 1 with group_of = None: one set); rceil: the scale exponent rounded up."""
        arr, count = self._adamw_mx_buckets_f32(buckets)
        groups = None
        if group_of is not None:
            if len(group_of) != count:
                raise ValueError(f"{len(group_of)} group indices for {count} buckets")
            if any(not 0 <= int(g) <= 255 for g in group_of):
                raise ValueError("a group index is one byte")
            groups = (C.c_uint8 * max(count, 1))(*[int(g) for g in group_of])
        flags = (_lib.ADAMW_ZERO_GRAD if zero_grad else 0) | (_lib.ADAMW_MX_RCEIL if rceil else 0)
        check(lib.allred_plan_adamw_all_gather_shards_mxfp8(self._h, arr, groups, count, int(hyper_ptr) or None, int(ngroups),
                                                            int(norm_sq_ptr or 0) or None, int(info_ptr or 0) or None,
                                                            flags, _stream_ptr(stream)),
              "plan_adamw_all_gather_shards_mxfp8")

    def adamw_shards_mxfp8_launches(self, buckets) -> int:
        """Kernel launches adamw_all_gather_shards_mxfp8 would enqueue for the list: one per
        ALLRED_ADAMW_MX_GROUP_MAX buckets, whatever the groups."""
        arr, count = self._adamw_mx_buckets_f32(buckets)
        st = lib.allred_plan_adamw_shards_mxfp8_launches(self._h, arr, count)
        if st < 0:
            raise AllredError(st, "plan_adamw_shards_mxfp8_launches")
        return st

    def rank_zones(self, stamps: np.ndarray):
        """Per-rank ALL_RED_LOOP (start, end) in 100 MHz ticks from host stamps."""
        st = np.ascontiguousarray(stamps, dtype=np.uint64)
        zs = np.zeros(self.total, dtype=np.uint64)
        ze = np.zeros(self.total, dtype=np.uint64)
        check(lib.allred_plan_rank_zones(self._h, st.ctypes.data, zs.ctypes.data, ze.ctypes.data), "plan_rank_zones")
        return zs, ze

    def close(self):
        if self._h:
            lib.allred_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- program surface
def parse_args(argv: Sequence[str], variant: int = BO) -> Args:
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    a = Args()
    check(lib.allred_args_parse(len(argv), arr, variant, C.byref(a)), "args_parse")
    return a


def run(argv: Sequence[str], variant: int = BO, verbose: bool = False, exec_mode: int | None = None,
        inputs: np.ndarray | None = None, outputs: bool = False):
    """AllredConfig(argv) + RunProgram() in-process (allred_helper.hpp:47-97).
    Returns the Report; with inputs (a (total, elems) uint16 array of arbitrary
    rank vectors: validation skipped, mismatches -1) or outputs=True (every
    rank's result wanted) it returns (Report, (total, elems) uint16 array or
    None), as run_multi does (allred_run_io)."""
    a = parse_args(argv, variant)
    if exec_mode is not None:
        a.exec = exec_mode
    r = Report()
    if inputs is None and not outputs:
        check(lib.allred_run(C.byref(a), int(verbose), C.byref(r)), "run")
        return r
    n = a.num_tiles * 1024
    out = np.zeros((a.total_nodes, n), dtype=np.uint16) if outputs else None
    inp = None
    if inputs is not None:
        inp = np.ascontiguousarray(inputs, dtype=np.uint16)
        if inp.shape != (a.total_nodes, n):
            raise ValueError(f"inputs must be ({a.total_nodes}, {n})")
    check(lib.allred_run_io(C.byref(a), int(verbose), C.byref(r), None if inp is None else inp.ctypes.data,
                            None if out is None else out.ctypes.data, None), "run_io")
    return r, out


def validate_device(ranks_ptr: int, stride: int, n: int, rows: int, src0_ptr: int, src1_ptr: int, mult: float,
                    error: float, round_mode: int = 0, stream=None) -> list:
    """allred_validate_device: validate_result_vector on the GPU for `rows`
    device-resident rows in one launch (k_validate).  Returns one dict per row:
    bad (the host validator's count), first_bad (lowest bad element index, None
    when the row has none), max_error (largest non-NaN |actual - expected| over
    the bad elements, 0.0 when none)."""
    rec = (_lib.RankCheck * max(rows, 1))()
    check(lib.allred_validate_device(ranks_ptr, stride, n, rows, src0_ptr, src1_ptr, mult, error, round_mode, rec,
                                     _stream_ptr(stream)), "validate_device")
    return [{"bad": int(x.bad), "first_bad": None if x.first_bad == 2 ** 64 - 1 else int(x.first_bad),
             "max_error": float(x.max_error)} for x in rec[:rows]]


def run_cli(binary: str, args: Sequence[str], env: dict | None = None, timeout: float = 300):
    """Run bin/<binary> (allred_BO_2D / allred_LO_2D / allred_mem_2D) like the reference."""
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([os.path.join(_lib.BIN_DIR, binary), *map(str, args)], capture_output=True, text=True,
                          env=e, timeout=timeout)


def multi_plan(argv: Sequence[str], variant: int = BO, gpus: int | None = None, check_all: bool = False) -> MultiPlan:
    """The plan of allred_run across GPUs (allred_multi_plan_build): pure host
    computation, no HIP call.  gpus overrides argv[10] / ALLRED_GPUS."""
    a = parse_args(argv, variant)
    if gpus is not None:
        a.gpus = gpus
    p = MultiPlan()
    check(lib.allred_multi_plan_build(C.byref(a), int(check_all), C.byref(p)), "multi_plan_build")
    return p


def run_multi(argv: Sequence[str], variant: int = BO, gpus: int | None = None, transport: int = TRANSPORT_RCCL,
              share_device: bool = False, timeout_ms: int = 0, verbose: bool = False, outputs: bool = True,
              inputs: np.ndarray | None = None):
    """allred_run across GPUs with an explicit backend (allred_run_multi).
    inputs: None (the reference's generated, validated inputs) or a (total,
    elems) uint16 array of arbitrary rank vectors (validation skipped).
    Returns (Report, every rank's result as a (total, elems) uint16 array or None)."""
    a = parse_args(argv, variant)
    if gpus is not None:
        a.gpus = gpus
    n = a.num_tiles * 1024
    r = Report()
    out = np.zeros((a.total_nodes, n), dtype=np.uint16) if outputs else None
    inp = None
    if inputs is not None:
        inp = np.ascontiguousarray(inputs, dtype=np.uint16)
        if inp.shape != (a.total_nodes, n):
            raise ValueError(f"inputs must be ({a.total_nodes}, {n})")
    o = MultiOpts(transport, int(share_device), timeout_ms, 0)
    check(lib.allred_run_multi(C.byref(a), C.byref(o), int(verbose), C.byref(r),
                               None if inp is None else inp.ctypes.data, None if out is None else out.ctypes.data),
          "run_multi")
    return r, out


# ---------------------------------------------------------------- multi-GPU
class Comm:
    """One RCCL communicator per process/GPU (allred_comm_*)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES)()
        check(lib.allred_comm_get_unique_id(buf), "comm_get_unique_id")
        return bytes(buf)

    def __init__(self, uid: bytes, nranks: int, rank: int, device: int):
        buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        check(lib.allred_comm_init(buf, nranks, rank, device, C.byref(h)), "comm_init")
        self._h = h
        self.nranks, self.rank = nranks, rank

    @classmethod
    def init_all(cls, devices: Sequence[int]) -> list:
        """One communicator per device in this process (allred_comm_init_all)."""
        devs = (C.c_int * len(devices))(*devices)
        hs = (C.c_void_p * len(devices))()
        check(lib.allred_comm_init_all(len(devices), devs, hs), "comm_init_all")
        out = []
        for i, h in enumerate(hs):
            c = cls.__new__(cls)
            c._h = C.c_void_p(h)
            c.nranks, c.rank = len(devices), i
            out.append(c)
        return out

    def set_timeout(self, ms: int) -> None:
        check(lib.allred_comm_set_timeout(self._h, ms), "comm_set_timeout")

    def wait(self, stream=None) -> None:
        """Bounded stream drain (allred_comm_wait): ALLRED_ERR_TRANSPORT past the deadline."""
        check(lib.allred_comm_wait(self._h, _stream_ptr(stream)), "comm_wait")

    @property
    def aborted(self) -> bool:
        return bool(lib.allred_comm_aborted(self._h))

    def close(self):
        if self._h:
            lib.allred_comm_destroy(self._h)
            self._h = None


def dist_desc(algo: int, variant: int, side: int, total: int, elems: int, local_ranks: int = 1,
              local_side: int = 1, local_algo: int = SWING, channels: int = 0, mem_accum: int = ACC_FP32) -> DistDesc:
    return DistDesc(algo, variant, side, total, elems, local_ranks, local_side, local_algo, channels, mem_accum)


def dist_workspace_bytes(desc: DistDesc) -> int:
    return lib.allred_dist_workspace_bytes(C.byref(desc))


def dist_program_stats(desc: DistDesc, rank: int) -> dict:
    """The cached per-rank program: exchange steps, add launches, send+recv segments."""
    k, a, g = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib.allred_dist_program_stats(C.byref(desc), rank, C.byref(k), C.byref(a), C.byref(g)), "dist_program_stats")
    return {"steps": k.value, "add_launches": a.value, "segments": g.value}


def dist_allreduce(comm: Comm, desc: DistDesc, buf_ptr: int, workspace_ptr: int, stream=None) -> None:
    check(lib.allred_dist_allreduce(comm._h, C.byref(desc), buf_ptr, workspace_ptr, _stream_ptr(stream)),
          "dist_allreduce")


def dist_allreduce_pipelined(comm: Comm, desc: DistDesc, cur_ptr: int | None, workspace_ptr: int, stream=None) -> None:
    """The hierarchical step pipelined across buckets (allred_dist_allreduce_pipelined):
    K buckets = K + 1 calls b0, b1, ..., None; workspace = 2 * dist_workspace_bytes(desc)."""
    check(lib.allred_dist_allreduce_pipelined(comm._h, C.byref(desc), cur_ptr or None, workspace_ptr,
                                              _stream_ptr(stream)), "dist_allreduce_pipelined")


def tree_broadcast_pipelined(cur_ptr: int, prev_ptr: int, stride: int, n: int, algo: int, side: int, total: int,
                             cur_out_ptr: int, prev_src_ptr: int, stream=None) -> None:
    check(lib.allred_tree_broadcast_pipelined(cur_ptr, prev_ptr, stride, n, algo, side, total, cur_out_ptr,
                                              prev_src_ptr, _stream_ptr(stream)), "tree_broadcast_pipelined")


def dist_reduce_scatter(comm: Comm, desc: DistDesc, buf_ptr: int, workspace_ptr: int, stream=None) -> None:
    """The reduce-scatter half of dist_allreduce's BO program (allred_dist_reduce_scatter):
    rank r's block r final, its other blocks unspecified."""
    check(lib.allred_dist_reduce_scatter(comm._h, C.byref(desc), buf_ptr, workspace_ptr, _stream_ptr(stream)),
          "dist_reduce_scatter")


def dist_all_gather(comm: Comm, desc: DistDesc, buf_ptr: int, workspace_ptr: int, stream=None) -> None:
    """The all-gather half (allred_dist_all_gather): every rank gets every owner's block."""
    check(lib.allred_dist_all_gather(comm._h, C.byref(desc), buf_ptr, workspace_ptr, _stream_ptr(stream)),
          "dist_all_gather")


def dist_allreduce_host(desc: DistDesc, rank: int, buf: np.ndarray, scratch: np.ndarray,
                        exchange: Callable[[int, list, list], None]) -> None:
    """Host-memory twin: `exchange(peer, sends, recvs)` gets lists of writable
    uint8 numpy views and must send every send view / fill every recv view."""
    _dist_host(lib.allred_dist_allreduce_host, "dist_allreduce_host", desc, rank, buf, scratch, exchange)


def dist_reduce_scatter_host(desc: DistDesc, rank: int, buf: np.ndarray, scratch: np.ndarray,
                             exchange: Callable[[int, list, list], None]) -> None:
    """Host-memory twin of dist_reduce_scatter (exchange as dist_allreduce_host's)."""
    _dist_host(lib.allred_dist_reduce_scatter_host, "dist_reduce_scatter_host", desc, rank, buf, scratch, exchange)


def dist_all_gather_host(desc: DistDesc, rank: int, buf: np.ndarray, scratch: np.ndarray,
                         exchange: Callable[[int, list, list], None]) -> None:
    """Host-memory twin of dist_all_gather (exchange as dist_allreduce_host's)."""
    _dist_host(lib.allred_dist_all_gather_host, "dist_all_gather_host", desc, rank, buf, scratch, exchange)


def _dist_host(fn, what: str, desc: DistDesc, rank: int, buf: np.ndarray, scratch: np.ndarray, exchange) -> None:
    def _cb(_ctx, peer, nsend, send, nrecv, recv):
        try:
            def views(segs, n):
                out = []
                for i in range(n):
                    s = segs[i]
                    out.append(np.ctypeslib.as_array((C.c_uint8 * s.bytes).from_address(s.ptr)))
                return out
            exchange(peer, views(send, nsend), views(recv, nrecv))
            return 0
        except Exception:  # pragma: no cover - surfaced as ALLRED_ERR_TRANSPORT
            import traceback
            traceback.print_exc()
            return 1

    cb = _lib.EXCHANGE_FN(_cb)
    assert buf.dtype == np.uint16 and scratch.dtype == np.uint16
    check(fn(C.byref(desc), rank, buf.ctypes.data, scratch.ctypes.data, cb, None), what)


PEER_TIMEOUT, PEER_WIN_CACHED, PEER_FLAGS_CACHED = _lib.PEER_TIMEOUT, _lib.PEER_WIN_CACHED, _lib.PEER_FLAGS_CACHED


class Peer:
    """Peer-mapped one-shot allreduce across GPUs (allred_peer_*): the
    allred_mem_2D variant over xGMI.  handle() -> exchange with every rank ->
    connect(list of all ranks' handles in rank order)."""

    def __init__(self, nranks: int, rank: int, device: int, max_elems: int):
        h = C.c_void_p()
        check(lib.allred_peer_create(nranks, rank, device, max_elems, C.byref(h)), "peer_create")
        self._h = h
        self.nranks, self.rank = nranks, rank

    def handle(self) -> bytes:
        buf = (C.c_uint8 * _lib.PEER_HANDLE_BYTES)()
        check(lib.allred_peer_handle(self._h, buf), "peer_handle")
        return bytes(buf)

    def connect(self, handles: Sequence[bytes]) -> None:
        blob = b"".join(handles)
        arr = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        check(lib.allred_peer_connect(self._h, arr), "peer_connect")

    @staticmethod
    def connect_all(peers: Sequence["Peer"]) -> None:
        """The peers of ONE process (peers[q] = rank q), mapped into each other
        without IPC (allred_peer_connect_all)."""
        arr = (C.c_void_p * len(peers))(*[p._h.value for p in peers])
        check(lib.allred_peer_connect_all(len(peers), arr), "peer_connect_all")

    def allreduce(self, buf_ptr: int, elems: int, stream=None, local_ranks: int = 1, local_side: int = 1,
                  local_algo: int = SWING, workspace_ptr: int | None = None, check_status: bool = False) -> None:
        """check_status: synchronise the stream and raise AllredError(ERR_TRANSPORT)
        if a peer wait timed out (the bytes are then wrong).  Without it the
        caller must call check() (or status()) before using the result."""
        check(lib.allred_peer_allreduce(self._h, buf_ptr, elems, local_ranks, local_side, local_algo, workspace_ptr,
                                        _stream_ptr(stream)), "peer_allreduce")
        if check_status:
            self.check(stream)

    def allreduce_pipelined2(self, cur_ptr: int | None, elems: int, stream=None, local_ranks: int = 64,
                             local_side: int = 8, local_algo: int = SWING) -> None:
        """The hierarchical step pipelined two buckets deep (k_hier_x2): starts cur,
        sums the owned tiles of the previous call's bucket, writes the rows of the
        bucket started two calls earlier; cur None finishes everything pending.
        K buckets = K + 1 calls: b0, b1, ..., b_{K-1}, None."""
        check(lib.allred_peer_allreduce_pipelined2(self._h, cur_ptr or None, elems, local_ranks, local_side,
                                                   local_algo, _stream_ptr(stream)), "peer_allreduce_pipelined2")

    def dist_allreduce(self, desc: DistDesc, buf_ptr: int, workspace_ptr: int | None = None, stream=None,
                       check_status: bool = False) -> None:
        """dist_allreduce's program (same desc, same bits) over the peer windows."""
        check(lib.allred_peer_dist_allreduce(self._h, C.byref(desc), buf_ptr, workspace_ptr, _stream_ptr(stream)),
              "peer_dist_allreduce")
        if check_status:
            self.check(stream)

    def check(self, stream=None) -> None:
        """allred_peer_check: sync `stream`, raise if any call so far timed out."""
        check(lib.allred_peer_check(self._h, _stream_ptr(stream)), "peer timeout (a peer never arrived)")

    def set_oneshot_max(self, nbytes: int) -> None:
        """Buckets of at most nbytes run as one kernel (same bits either way)."""
        check(lib.allred_peer_set_oneshot_max(self._h, nbytes), "peer_set_oneshot_max")

    def set_hier_ll(self, mode) -> None:
        """64 local ranks: 1 (or True, the default) the hierarchical step as one
        launch with LL push hand-offs, reducing and writing waves in every
        workgroup (k_hier_ws); 0 (or False) the launch form.  Same result bits."""
        check(lib.allred_peer_set_hier_ll(self._h, int(mode)), "peer_set_hier_ll")

    def set_lo_ll_max(self, nbytes: int) -> None:
        """One-channel LO buckets up to nbytes take the LL-push program (same bits; 0 = never)."""
        check(lib.allred_peer_set_lo_ll_max(self._h, nbytes), "peer_set_lo_ll_max")

    def set_mem_ll_max(self, nbytes: int) -> None:
        """mem_2D buckets up to nbytes take the LL-push form (same bits; 0 = never)."""
        check(lib.allred_peer_set_mem_ll_max(self._h, nbytes), "peer_set_mem_ll_max")

    def set_sched_push(self, min_bytes: int) -> None:
        """BO buckets of >= min_bytes in the push form of the scheduled program (0 = never)."""
        check(lib.allred_peer_set_sched_push(self._h, min_bytes), "peer_set_sched_push")

    def set_max_groups(self, groups: int) -> None:
        """Grid cap of the hierarchical one-kernel forms (0 = one full grid per GPU);
        processes sharing a GPU need groups <= 512 / processes."""
        check(lib.allred_peer_set_max_groups(self._h, groups), "peer_set_max_groups")

    def status(self) -> int:
        v = C.c_uint32(0)
        check(lib.allred_peer_status(self._h, C.byref(v)), "peer_status")
        return v.value

    def clear_status(self) -> None:
        """allred_peer_clear_status: the sticky timeout bit cleared (no kernel of this peer in flight)"""
        check(lib.allred_peer_clear_status(self._h), "peer_clear_status")

    def close(self):
        if self._h:
            lib.allred_peer_destroy(self._h)
            self._h = None
