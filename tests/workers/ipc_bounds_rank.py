"""One rank of the two-process bounds test (tests/test_gpu_bounds.py starts two of these through torch.distributed.run; they
share GPU 0).  Every rank: its member block of a C3 ensemble, collective="ipc", the same bounds on every rank
(grape_set_bounds: each rank saturates its own copy and applies the slope to the exchanged row), the same penalties, a few
evaluations of raw pulses -- then the same again with a basis -- written to <out>.rank<r>.npz.  Fresh processes only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import signal
    signal.alarm(240)                                        # this rank's own time limit: a stuck exchange ends here
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
        sg.local.set_bounds(data["lo"], data["hi"])
        ev = [sg.local.eval(u) for u in data["us"]]
        res["F"], res["G"] = np.array([e[0] for e in ev]), np.array([e[1] for e in ev])
        res["x"] = sg.local.controls(data["us"][0])
        res["names"] = np.array(";".join(sg.local.kernel_names()))
        sg.local.set_basis(data["phi"], data["x0"])
        ev = [sg.local.eval(th) for th in data["thetas"]]
        res["F_basis"], res["G_basis"] = np.array([e[0] for e in ev]), np.array([e[1] for e in ev])
        res["names_basis"] = np.array(";".join(sg.local.kernel_names()))
    np.savez(f"{out}.rank{rank}.npz", **res)
    dist.barrier()
    sg.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
