"""The shard-family kernels through the replay soak (tests/soak.py): k_tree_group_f32, k_tree_group_f32_norm,
k_ag_group_f32, k_adamw_ag_group_f32, k_adamw_ag_groups_f32 and k_ag_group_mxfp8 at every instantiated rank
count and both values of their bool (tests/soak_cases.py, SHARD_CASES), and the norm hand-off in four more
arrangements (HANDOFF_CASES), each under `idle`, `uniform` and `uneven` load.

What the other modules settle — the bits — is taken from the same references: tests/f32_tree.py,
tests/f32_norm.py, tests/adamw_ref.py and tests/mxfp8_ref.py, on two seeds.  What is new here is when the
kernels run: one capture, soak.R replays back to back, the two datasets alternating in the same buffers,
every buffer — rank rows with skew and guard row, flat shard and plane buffers with their guard, norm_sq
between its guards, the small hyper / norm_sq / info buffer — restored before and compared whole after
every replay, on the device.  The AdamW planes are restored on every replay.  The norm workspace is never
restored: its counter is zeroed once and must be zero after every replay; its guards are compared, its
partials are unspecified.  The fp32 data is finite (soak_cases.finite_planes / finite_floats, hard_inputs.cancel
for the rows), so nothing is compared by class; the MXFP8 outputs are bytes.

Arrangement (c), `warm`: ONE int32 buffer of 256 + total * WARM_STRIDE + 32 words, B = its first 128-byte
aligned address at or behind 256 bytes in; shard = B + 16, shard_stride = 336 floats, norm_ws = B + 1040 — in
the gap behind block 0.  tests/soak_cases.py states the lines; tests/test_soak_table.py checks them.  The
whole buffer is restored and compared but for the workspace's partials."""
import functools

import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import f32_norm
import f32_norm_cases as ncases
import f32_tree
import soak_cases as sc
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)
import test_gpu_adamw_groups as groups  # noqa: E402
import test_gpu_adamw_shards as one  # noqa: E402
import test_gpu_shards_f32 as base  # noqa: E402
import test_gpu_shards_f32_norm as norm  # noqa: E402
import test_gpu_shards_mxfp8 as mxt  # noqa: E402

pytestmark = pytest.mark.gpu
SENT32 = base.SENT32
loads = pytest.mark.parametrize("mode", soak.MODES)


def finite(images, what):
    for im in images:
        assert not f32_tree.is_nan32(np.ascontiguousarray(im).view(np.float32)).any(), f"{what}: a NaN would be compared by class"
    return images


def row_image(b, data):
    im = b.host.copy()
    im[:b.total, :b.n] = data
    return im


def shard_bufs(name, shards, staged, want):
    """staged / want: per dataset the list of host images of shards.buf"""
    return [soak.SoakBuf(f"{name} {k}", d, [s[k] for s in staged], finite([w[k] for w in want], name))
            for k, d in enumerate(shards.buf)]


def norm_bufs(nm, wants):
    """norm_sq between its guards, restored to NaN; the workspace: guards and counter, never restored"""
    G, words = norm.GUARD, nm.bytes // 4
    sq_want = []
    for w in wants:
        im = nm.sq_host.copy()
        im[G:G + nm.total] = np.asarray(w, dtype=np.float32).view(np.uint32)
        sq_want.append(im)
    head = np.full(G + 16, SENT32, dtype=np.uint32)
    head[G:] = 0
    tail = np.full(G, SENT32, dtype=np.uint32)
    return [soak.SoakBuf("norm_sq", nm.sq, [nm.sq_host, nm.sq_host], finite(sq_want, "norm_sq")),
            soak.SoakBuf("workspace: front guard and counter", nm.ws, None, [head, head], slice(0, G + 16)),
            soak.SoakBuf("workspace: back guard", nm.ws, None, [tail, tail], slice(G + words, 2 * G + words))]


@functools.lru_cache(maxsize=None)
def tree_data(total, tiles, seed):
    return ncases.bucket_list(t.SWING, sc.SIDE[total], total, tiles, seed=seed)


def old_blocks(datas, seed):
    return [sc.finite_floats(seed + i, s.shape) for i, (_, s) in enumerate(datas)]


def tree_case(c, plan):
    """k_tree_group_f32 / k_tree_group_f32_norm, flag = ACC; the `warm` arrangement has its own buffers"""
    total, acc, with_norm = c["total"], c["flag"], c["family"] == "norm"
    datas = [tree_data(total, c["tiles"], seed) for seed in sc.SEEDS]
    buckets = norm.make_buckets(datas[0])
    olds = [old_blocks(d, 50 + seed) if acc else None for d, seed in zip(datas, sc.SEEDS)]
    values = [ncases.stored(d, sc.SCALE, o) for d, o in zip(datas, olds)]
    bufs = [soak.SoakBuf(f"bucket {i} rows", b.buf, [row_image(b, d[i][0]) for d in datas], [row_image(b, d[i][0]) for d in datas])
            for i, b in enumerate(buckets)]
    if c.get("arrangement") == "warm":
        args, more, keep = warm_buffers(total, buckets[0], olds, values)
        bufs += more
        sq = base.to_dev32(np.full(2 * norm.GUARD + total, SENT32, dtype=np.uint32))
        sq_host = np.full(2 * norm.GUARD + total, SENT32, dtype=np.uint32)
        sq_host[norm.GUARD:norm.GUARD + total] = norm.NAN32
        sq_want = []
        for v in values:
            im = sq_host.copy()
            im[norm.GUARD:norm.GUARD + total] = f32_norm.expect_norm_sq(v).view(np.uint32)
            sq_want.append(im)
        bufs.append(soak.SoakBuf("norm_sq", sq, [sq_host, sq_host], finite(sq_want, "norm_sq")))
        sq_ptr, ws_ptr = sq.data_ptr() + 4 * norm.GUARD, keep["ws_ptr"]
        assert plan.shards_f32_norm_workspace_bytes(args) == 64 + 4 * total
    else:
        shards = base.Shards(buckets, "flat")
        args = shards.args()
        staged = [shards.expected(o) if acc else shards.host for o in olds]
        bufs += shard_bufs("shards", shards, staged, [shards.expected(v) for v in values])
        keep = shards
        if with_norm:
            nm = norm.Norm(plan, args, total)
            bufs += norm_bufs(nm, [f32_norm.expect_norm_sq(v) for v in values])
            sq_ptr, ws_ptr, keep = nm.sq_ptr, nm.ws_ptr, (shards, nm)

    def call(s):
        if with_norm:
            plan.reduce_scatter_shards_f32_norm(args, sq_ptr, ws_ptr, sc.SCALE, accumulate=acc, stream=s)
        else:
            plan.reduce_scatter_shards_f32(args, sc.SCALE, accumulate=acc, stream=s)
    case = soak.Case(bufs, call)
    case.keep = (buckets, keep)
    return case


def warm_buffers(total, bucket, olds, values):
    """arrangement (c): the shard blocks and the workspace in one buffer (module docstring)"""
    blocks, ws, partials, nbytes = sc.warm_layout(total)
    lead = 256
    dev = torch.empty((lead + nbytes + sc.LINE) // 4 + 64, dtype=torch.int32, device=soak.DEV)
    B = (dev.data_ptr() + lead + sc.LINE - 1) // sc.LINE * sc.LINE
    off = B - dev.data_ptr()          # bytes from the buffer's head to B
    assert B % sc.LINE == 0 and off >= lead and off + nbytes <= 4 * dev.numel()

    def image(blocks_f32):
        im = np.full(dev.numel(), SENT32, dtype=np.uint32)
        im[(off + ws[0]) // 4:(off + ws[0] + sc.COUNTER_BYTES) // 4] = 0          # the counter: zero, and zero again after every launch
        if blocks_f32 is not None:
            for b, (lo, hi) in enumerate(blocks):
                im[(off + lo) // 4:(off + hi) // 4] = np.ascontiguousarray(blocks_f32[b]).view(np.uint32)
        return im
    staged = [image(None if o is None else o[0]) for o in olds]
    want = finite([image(v[0]) for v in values], "the warm buffer")
    p0, p1 = (off + partials[0]) // 4, (off + partials[1]) // 4
    dev.copy_(soak.as_int(staged[0]))
    # compared in two windows around the partials, which are unspecified; restored whole: the partials of the replay
    # before are gone, so each replay's finalizer reads what THIS replay stored or the sentinel
    bufs = [soak.SoakBuf("warm buffer up to the partials", dev, staged, [w[:p0] for w in want], slice(0, p0)),
            soak.SoakBuf("warm buffer behind the partials", dev, None, [w[p1:] for w in want], slice(p1, dev.numel()))]
    args = [bucket.arg + (B + sc.WARM_SHARD_OFF, sc.WARM_STRIDE)]
    return args, bufs, {"dev": dev, "ws_ptr": B + sc.WARM_WS_OFF}


def ag_case(c, plan):
    total = c["total"]
    buckets = [base.Bucket(base.inputs("soft", total, 256 * total * k, 5), None, None if i % 2 == 0 else 256 * total * k)
               for i, k in enumerate(c["tiles"])]
    shards = base.Shards(buckets, "flat")
    src = [[sc.finite_floats(1000 * seed + i, (total, b.blk)) for i, b in enumerate(buckets)] for seed in sc.SEEDS]
    images = [shards.expected(s) for s in src]
    bufs = [soak.SoakBuf(f"bucket {i} rows", b.buf, [b.host, b.host], [b.after_all_gather(f32_tree.bf16_rne(s[i])) for s in src])
            for i, b in enumerate(buckets)]
    bufs += shard_bufs("shards", shards, images, images)
    args = shards.args()
    case = soak.Case(bufs, lambda s: plan.all_gather_shards_f32(args, s))
    case.keep = (buckets, shards)
    return case


def adamw_case(c, plan):
    total, zero, grouped = c["total"], c["flag"], c["family"] == "groups"
    buckets = one.rows_buckets(total, c["tiles"])
    data = [one.make_data(buckets, 100 * seed, sc.finite_planes) for seed in sc.SEEDS]
    planes = one.Planes(buckets, "flat", data[0])
    nsq = adamw_cases.norm_sq(total)
    small = groups.SmallG(gc.hyper_array(2), nsq) if grouped else one.Small(adamw_cases.hyper(), nsq)
    want = [gc.expect(d, sc.GROUP_OF, nsq, total, zero) if grouped else one.expect(d, adamw_cases.hyper(), nsq, total, zero) for d in data]
    bufs = [soak.SoakBuf(f"bucket {i} rows", b.buf, [b.host, b.host], [b.after_all_gather(w[1][i]) for w in want])
            for i, b in enumerate(buckets)]
    for k in range(4):
        staged = [planes.s[k].expected([x[k] for x in d]) for d in data]
        after = [planes.s[k].expected([v[k] for v in w[0]]) for w in want]
        bufs += shard_bufs(one.NAMES[k], planes.s[k], staged, after)
    info = []
    for w in want:
        im = small.host.copy()
        im[small.INFO:small.INFO + 4] = np.asarray(w[2], dtype=np.float32).view(np.uint32)
        info.append(im)
    bufs.append(soak.SoakBuf("hyper / norm_sq / info", small.buf, [small.host, small.host], finite(info, "info")))
    args = planes.args()

    def call(s):
        if grouped:
            plan.adamw_all_gather_shards_f32_groups(args, sc.GROUP_OF, small.hyper, 2, small.norm_sq, small.info, zero_grad=zero, stream=s)
        else:
            plan.adamw_all_gather_shards_f32(args, small.hyper, small.norm_sq, small.info, zero_grad=zero, stream=s)
    case = soak.Case(bufs, call)
    case.keep = (buckets, planes, small)
    return case


def mx_case(c, plan):
    total, rceil = c["total"], c["flag"]
    buckets, _ = mxt.unequal(total)
    keys = [[(total, 256 * k, 10 * seed + i) for i, k in enumerate(c["tiles"])] for seed in sc.SEEDS]   # mxt.cases' keys
    shards = base.Shards(buckets, "flat")
    images = [shards.expected([mxt.cases(*key) for key in ks]) for ks in keys]
    bufs = []
    for i, b in enumerate(buckets):
        after = [b.after(*mxt.expected(*ks[i], rceil)) for ks in keys]
        for j, name in enumerate(("element rows", "scale rows")):
            bufs.append(soak.SoakBuf(f"bucket {i} {name}", b.buf[j], [b.host[j], b.host[j]], [a[j] for a in after]))
    bufs += [soak.SoakBuf(f"shards {k}", d, [im[k] for im in images], [im[k] for im in images]) for k, d in enumerate(shards.buf)]
    args = shards.args()
    case = soak.Case(bufs, lambda s: plan.all_gather_shards_mxfp8(args, rceil=rceil, stream=s))
    case.keep = (buckets, shards)
    return case


BUILD = {"tree": tree_case, "norm": tree_case, "ag": ag_case, "adamw": adamw_case, "groups": adamw_case, "mxfp8": mx_case}


def run(c, mode):
    total = c["total"]
    plan = base.any_plan(t.SWING, sc.SIDE[total], total)
    try:
        case = BUILD[c["family"]](c, plan)
        with t.tuned(pipe_grid=c["grid"]):
            _, trace, _ = soak.soak(case, soak.R, mode)
        assert trace.kernels == [sc.kernel_name(c["family"], total, c["flag"])] * c["launches"], trace.kernels
        return trace
    finally:
        plan.close()


@loads
@pytest.mark.parametrize("c", sc.SHARD_CASES, ids=[sc.case_id(c) for c in sc.SHARD_CASES])
def test_shard_kernel_soaked(c, mode):
    """the UNEQUAL list, flat, pipe_grid 5: every workgroup walks at least three tiles"""
    trace = run(c, mode)
    tiles = c["total"] * sum(c["tiles"])
    assert trace.grids == [sc.GRID] and tiles >= 3 * sc.GRID, (trace.grids, tiles)


@loads
@pytest.mark.parametrize("c", sc.HANDOFF_CASES, ids=[sc.case_id(c) for c in sc.HANDOFF_CASES])
def test_norm_hand_off_soaked(c, mode):
    trace = run(c, mode)
    if c["arrangement"] in ("grid", "warm"):
        assert trace.grids == [c["total"]], f"one workgroup per tile: {trace.grids}"
