"""One rank of the two-process penalty test (tests/test_gpu_penalties.py starts two of these through torch.distributed.run;
they share GPU 0).  Every rank: its member block of a C3 ensemble, collective="ipc", the same C3 / C4 weights on every rank
(the library lets rank 0 alone add them), one evaluation written to <out>.rank<r>.npz.  Fresh processes only."""
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

    out, E, N = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    rank = int(os.environ["RANK"])
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    w = qoc.workloads.config("C3", E=E, N=N)
    amp = np.linspace(0.3, 0.9, w.K)
    var = np.linspace(0.8, 0.2, w.K)
    amp[1] = 0.0
    sg = sharded_engine(w, dev, collective="ipc", penalties=(amp, var))
    res = {"collective": np.array(sg.collective), "error": np.array(getattr(sg, "attach_error", ""))}
    if sg.collective == "ipc":
        F, G = sg.eval(w.x)
        res["F"], res["G"] = F, G
    np.savez(f"{out}.rank{rank}.npz", **res)
    dist.barrier()
    sg.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
