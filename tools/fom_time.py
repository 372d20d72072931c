"""Blocking host->host time of grape_eval (F and G) and of grape_eval_fom (F alone) for C3 (E = 1024, N = 500), C2 and C1:
ONE context per config in one process, the two calls measured in alternating blocks after a warm-up so that clock drift
and other tenants' work hit both alike; per call: median over the blocks of the block means, and the spread between
blocks (half the 10 % .. 90 % range).  C3 also times fom with a batch of 8 control arrays (per call and per array).
Usage: python tools/fom_time.py [blocks] [calls_per_block] [out_file]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quoptimalcontrol_jl_amd as qoc  # noqa: E402


def stats(samples):
    s = np.asarray(samples) * 1e6
    return float(np.median(s)), float(0.5 * (np.percentile(s, 90) - np.percentile(s, 10)))


def main():
    blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    say(f"# tools/fom_time.py: {blocks} alternating blocks of {calls} blocking host->host calls per config, one context;")
    say("# us per call: median of the block means +- half the 10..90 % range between blocks")
    for name in ("C3", "C2", "C1"):
        w = qoc.workloads.config(name)
        B = 8 if name == "C3" else 1
        eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0, max_batch=B)
        xf = np.ascontiguousarray(w.x.T)
        G = np.empty_like(xf)
        rng = np.random.default_rng(1)
        X = np.stack([w.x] + [w.x + 0.01 * rng.standard_normal(w.x.shape) for _ in range(B - 1)])
        Xf = np.ascontiguousarray(np.swapaxes(X, 1, 2))          # the library's layout, as eval_cm's xf: no copies in the loop
        Fb = np.empty(B)
        lib, h = eng._lib, eng._h

        def fom_cm(buf, n_x):
            rc = lib.grape_eval_fom(h, n_x, buf.ctypes.data, Fb.ctypes.data, None)
            if rc:
                eng._check(rc)
            return Fb[0]
        todo = {"eval": lambda: eng.eval_cm(xf, G), "fom": lambda: fom_cm(xf, 1)}
        if B > 1:
            todo["fom8"] = lambda: fom_cm(Xf, B)
        names = {}
        for key, fn in todo.items():                          # warm-up: code objects, LDS grants, the wait estimate
            for _ in range(50):
                fn()
            names[key] = ";".join(eng.kernel_names())
        t = {key: [] for key in todo}
        for _ in range(blocks):
            for key, fn in todo.items():
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                t[key].append((time.perf_counter() - t0) / calls)
        F_eval, F_fom = eng.eval_cm(xf, G), fom_cm(xf, 1)
        ev, ev_s = stats(t["eval"])
        fo, fo_s = stats(t["fom"])
        say(f"{name} n={w.n} E={w.E} N={w.N} K={w.K}: grape_eval {ev:.2f} +- {ev_s:.2f} us   grape_eval_fom {fo:.2f} +- {fo_s:.2f} us   "
            f"ratio {fo / ev:.3f}   below eval by {ev - fo:.2f} us (spread {max(ev_s, fo_s):.2f} us)   |F_fom - F_eval| = {abs(F_fom - F_eval):.1e}")
        if B > 1:
            f8, f8_s = stats(t["fom8"])
            say(f"{name} batch of {B}: grape_eval_fom {f8:.2f} +- {f8_s:.2f} us per call, {f8 / B:.2f} us per array   "
                f"ratio per array to grape_eval {f8 / B / ev:.3f}")
        for key in todo:
            say(f"  kernels {key}: {names[key]}")
        eng.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
