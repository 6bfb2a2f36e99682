"""Child process of tests/test_gpu_rs_ag_multidevice.py: ONE rank of an RCCL world,
on the GPU of its rank.  Runs allred_dist_reduce_scatter, then allred_dist_all_gather
on the same bucket, then allred_dist_all_gather alone on arbitrary 16-bit data, for
every schedule and with check mode off and on, and writes what it got to an .npz
file for the parent to compare with the oracle.  The inputs come from
tests/test_gpu_rs_ag_multidevice.py's rank_inputs, the same on both sides.

usage: gpu_rs_ag_child.py <rank> <world> <unique id, hex> <out.npz>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))   # the parent module imports the oracle
sys.path.insert(0, HERE)

import torch  # noqa: E402
import tenstorrentallreduce_amd as t  # noqa: E402
from test_gpu_rs_ag_multidevice import ALGOS, GRIDS, elems, rank_inputs  # noqa: E402


def main():
    rank, world, uid, out_path = int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4]
    torch.cuda.set_device(rank)
    dev = f"cuda:{rank}"
    comm = t.Comm(uid, world, rank, rank)
    side2d, total = GRIDS[world]
    n = elems(world)
    s = torch.cuda.current_stream()
    got = {}
    try:
        for check in (0, 1):
            with t.tuned(check=check):
                for algo in ALGOS:
                    desc = t.dist_desc(algo, t.BO, 1 if algo >= 2 else side2d, total, n, channels=1)
                    ws = torch.empty(t.dist_workspace_bytes(desc), dtype=torch.uint8, device=dev)
                    data, raw = rank_inputs(world, algo, check)
                    buf = torch.from_numpy(data[rank].view(np.int16)).to(dev)
                    t.dist_reduce_scatter(comm, desc, buf.data_ptr(), ws.data_ptr(), s)
                    comm.wait(s)
                    got[f"rs_{check}_{algo}"] = buf.cpu().numpy().view(np.uint16)
                    t.dist_all_gather(comm, desc, buf.data_ptr(), ws.data_ptr(), s)
                    comm.wait(s)
                    got[f"rsag_{check}_{algo}"] = buf.cpu().numpy().view(np.uint16)
                    buf = torch.from_numpy(raw[rank].view(np.int16)).to(dev)
                    t.dist_all_gather(comm, desc, buf.data_ptr(), ws.data_ptr(), s)
                    comm.wait(s)
                    got[f"ag_{check}_{algo}"] = buf.cpu().numpy().view(np.uint16)
    finally:
        comm.close()
    np.savez(out_path, **got)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
