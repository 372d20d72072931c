"""One rank of the two-process parameter-mode test (tests/test_gpu_basis.py starts two of these through
torch.distributed.run; they share GPU 0).  Every rank: its member block of a C3 ensemble, collective="ipc", the same basis
on every rank (grape_set_basis: each rank expands its own copy and projects the exchanged row), the same penalties, a few
evaluations of parameter arrays written to <out>.rank<r>.npz.  Fresh processes only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    import quoptimalcontrol_jl_amd as qoc
    from quoptimalcontrol_jl_amd.distributed import sharded_engine

    out, E, N, data = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), np.load(sys.argv[4])
    rank = int(os.environ["RANK"])
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    w = qoc.workloads.config("C3", E=E, N=N)
    sg = sharded_engine(w, dev, collective="ipc", penalties=(data["amp"], data["var"]))
    res = {"collective": np.array(sg.collective), "error": np.array(getattr(sg, "attach_error", ""))}
    if sg.collective == "ipc":
        sg.local.set_basis(data["phi"], data["x0"])
        Fs, Gs = [], []
        for th in data["thetas"]:
            F, G = sg.local.eval(th)
            Fs.append(F)
            Gs.append(G)
        res["F"], res["G"] = np.array(Fs), np.array(Gs)
        res["x"] = sg.local.controls(data["thetas"][0])
        res["names"] = np.array(";".join(sg.local.kernel_names()))
    np.savez(f"{out}.rank{rank}.npz", **res)
    dist.barrier()
    sg.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
