"""Step time of the C3 and C4 configs with the control penalties off and on (grape_set_penalties): host grape_eval
calls, two contexts evaluated in alternating rounds so that clock drift hits both alike; median of the round means.
Usage: python tools/penalty_time.py [rounds] [calls_per_round]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quoptimalcontrol_jl_amd as qoc  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    for name in ("C3", "C4"):
        w = qoc.workloads.config(name)
        n = calls if name == "C3" else max(5, calls // 20)
        engs = {}
        for mode in ("off", "on"):
            engs[mode] = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
            if mode == "on":
                engs[mode].set_penalties(np.full(w.K, 1e-3), np.full(w.K, 1e-2))
            for _ in range(5):
                engs[mode].eval(w.x)
        t = {"off": [], "on": []}
        for _ in range(rounds):
            for mode in ("off", "on"):
                eng = engs[mode]
                t0 = time.perf_counter()
                for _ in range(n):
                    eng.eval(w.x)
                t[mode].append((time.perf_counter() - t0) / n)
        off, on = float(np.median(t["off"])), float(np.median(t["on"]))
        print(f"{name} E={w.E} N={w.N} K={w.K}: off {off * 1e6:.2f} us  on {on * 1e6:.2f} us  "
              f"delta {(on - off) * 1e6:+.2f} us ({(on / off - 1) * 100:+.2f} %)", flush=True)
        print(f"  kernels off: {';'.join(engs['off'].kernel_names())}", flush=True)
        print(f"  kernels on:  {';'.join(engs['on'].kernel_names())}", flush=True)
        for eng in engs.values():
            eng.close()


if __name__ == "__main__":
    main()
