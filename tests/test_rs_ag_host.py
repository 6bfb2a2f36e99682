"""Reduce-scatter and all-gather across ranks on CPU: the halves of the
per-rank BO step program (dist.cpp) through their host twins,
allred_dist_reduce_scatter_host / allred_dist_all_gather_host, over gloo
worlds of 2, 4 and 8 processes.  They run the first S / last S steps of the
same cached program the allreduce runs, so every comparison is bit-exact:
rank r's block r against the oracle's BO allreduce, the all-gather as a pure
16-bit copy, and the two in sequence against allred_dist_allreduce_host."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {2: (2, 2), 4: (2, 4), 8: (4, 8)}
ALGOS = (0, 1, 2, 3)   # RecDub, Swing, 1D RecDub, 1D Swing


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def gloo_exchange(peer, sends, recvs):
    reqs = [dist.isend(torch.from_numpy(v), peer, tag=i) for i, v in enumerate(sends)]
    reqs += [dist.irecv(torch.from_numpy(v), peer, tag=i) for i, v in enumerate(recvs)]
    for r in reqs:
        r.wait()


def worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    import tenstorrentallreduce_amd as t
    dist.init_process_group("gloo", rank=rank, world_size=world)
    side2d, total = GRIDS[world]
    n = 8 * total * 3
    blk = n // total
    own = slice(rank * blk, (rank + 1) * blk)
    fails = []
    for check in (0, 1):
        with t.tuned(check=check):
            for algo in ALGOS:
                side = 1 if algo >= 2 else side2d
                tag = (check, algo)
                desc = t.dist_desc(algo, t.BO, side, total, n, channels=1)
                scratch = np.zeros(2 * n, dtype=np.uint16)
                # reduce-scatter: block r of rank r is the oracle BO allreduce's block r
                rng = np.random.default_rng(1000 * world + 10 * algo + check)
                data = [rng.integers(0x3F80, 0x42C8, n).astype(np.uint16) for _ in range(world)]
                want = [d.copy() for d in data]
                oracle.allreduce("bo", algo, side, want, total)
                buf = data[rank].copy()
                t.dist_reduce_scatter_host(desc, rank, buf, scratch, gloo_exchange)
                if not np.array_equal(buf[own], want[rank][own]):
                    fails.append(("rs", tag, int((buf[own] != want[rank][own]).sum())))
                # ... then the all-gather: the allreduce, and dist_allreduce_host's bits (channels = 1)
                t.dist_all_gather_host(desc, rank, buf, scratch, gloo_exchange)
                if not np.array_equal(buf, want[rank]):
                    fails.append(("rs+ag vs oracle", tag, int((buf != want[rank]).sum())))
                whole = data[rank].copy()
                t.dist_allreduce_host(desc, rank, whole, scratch, gloo_exchange)
                if not np.array_equal(buf, whole):
                    fails.append(("rs+ag vs allreduce", tag, int((buf != whole).sum())))
                # all-gather alone on arbitrary 16-bit patterns (NaN / inf payloads): a pure copy
                raw = [rng.integers(0, 0x10000, n).astype(np.uint16) for _ in range(world)]
                buf = raw[rank].copy()
                t.dist_all_gather_host(desc, rank, buf, scratch, gloo_exchange)
                for b in range(total):
                    sl = slice(b * blk, (b + 1) * blk)
                    if not np.array_equal(buf[sl], raw[b][sl]):
                        fails.append(("ag", tag, b))
                # channels = 0 is the plain schedule too
                auto = t.dist_desc(algo, t.BO, side, total, n, channels=0)
                buf = raw[rank].copy()
                t.dist_all_gather_host(auto, rank, buf, scratch, gloo_exchange)
                if not all(np.array_equal(buf[b * blk:(b + 1) * blk], raw[b][b * blk:(b + 1) * blk])
                           for b in range(total)):
                    fails.append(("ag channels=0", tag))
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, fails))


@pytest.mark.parametrize("world", [2, 4, 8])
def test_reduce_scatter_all_gather_over_gloo(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, fails in results:
        assert fails == [], (rank, fails)


def test_unsupported_descs_refused_before_any_exchange():
    """channels = 2, local_ranks = 4, LO and MEM: ALLRED_ERR_UNSUPPORTED, and the
    exchange callback never runs."""
    sys.path.insert(0, ROOT)
    import tenstorrentallreduce_amd as t
    side, total = 4, 8
    n = 8 * total * 3
    calls = []

    def exchange(peer, sends, recvs):
        calls.append(peer)

    descs = [t.dist_desc(t.SWING, t.BO, side, total, n, channels=2),
             t.dist_desc(t.SWING, t.BO, side, total, n, local_ranks=4, local_side=2),
             t.dist_desc(t.SWING, t.LO, side, total, n),
             t.dist_desc(t.SWING, t.MEM, side, total, n)]
    for desc in descs:
        for fn in (t.dist_reduce_scatter_host, t.dist_all_gather_host):
            buf = np.zeros(4 * n, dtype=np.uint16)
            with pytest.raises(t.AllredError) as e:
                fn(desc, 0, buf, np.zeros(2 * n, dtype=np.uint16), exchange)
            assert e.value.status == t._lib.ERR_UNSUPPORTED
            assert not buf.any()
    assert calls == []
