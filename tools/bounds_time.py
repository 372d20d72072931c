"""What the smooth amplitude bounds (grape_set_bounds) cost on the headline config -- C3: 4 x 4, K = 4, N = 500, E = 1024 --
blocking host->host as tools/basis_time.py measures parameter mode:

  1. slice mode, bounds only, a basis only (M = 16 Fourier columns) and bounds + that basis on ONE context, alternating
     blocks after a warm-up (clock drift and other tenants' work hit all alike); per call: median over the blocks of the
     block means, and the spread between blocks (half the 10 % .. 90 % range).  Bounds only adds bounds_saturate_kernel in
     place of the upload and bounds_slope_kernel behind the evaluation; with a basis the two are fused into the basis kernels.
  2. slice-mode grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, given
     with --other): fresh child processes, this / other / this / other, each through the same raw ctypes calls (the other
     build need not export the new entry point).  They must agree within the block-to-block spread and return the same F
     bit for bit: a context without bounds did not move.

Usage: python tools/bounds_time.py [--blocks 21] [--calls 300] [--other PATH/libgrape_hip.so] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quoptimalcontrol_jl_amd as qoc  # noqa: E402
from basis_time import basis, child, stats  # noqa: E402

BOUND = 0.8                                                    # C3's guess lies in (0, 1): the upper bound bites


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--other", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.blocks, a.calls)
    out = open(a.out, "w") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    w = qoc.workloads.config("C3")
    phi = basis(w)
    M = phi.shape[1]
    say(f"# tools/bounds_time.py: C3 n={w.n} K={w.K} N={w.N} E={w.E}, bounds (-{BOUND}, {BOUND}) on every control, "
        f"M = {M} Fourier columns; blocking host->host calls")
    say(f"# 1. one context, {a.blocks} alternating blocks of {a.calls} calls; us per call: median of the block means "
        "+- half the 10..90 % range between blocks")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    xf, tf = np.ascontiguousarray(w.x.T), np.zeros((M, w.K))
    Gx, Gt = np.empty_like(xf), np.empty_like(tf)
    keys = ("slice", "bounds", "param", "bounds+param")
    names, t, F = {}, {k: [] for k in keys}, {}

    def mode(key):
        eng.set_bounds(*((-BOUND, BOUND) if "bounds" in key else (None, None)))
        eng.set_basis(phi if "param" in key else None, 0.5 * w.x if "param" in key else None)
        return (lambda: eng.eval_cm(tf, Gt)) if "param" in key else (lambda: eng.eval_cm(xf, Gx))
    for key in keys:
        fn = mode(key)
        for _ in range(100):
            fn()
        names[key] = ";".join(eng.kernel_names())
    for _ in range(a.blocks):
        for key in keys:
            fn = mode(key)                                   # (the setters synchronise: outside the timed loop)
            F[key] = fn()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            t[key].append((time.perf_counter() - t0) / a.calls)
    sl, sl_s = stats(t["slice"])
    say(f"slice mode        grape_eval {sl:.2f} +- {sl_s:.2f} us   F = {F['slice']!r}")
    for key, label in (("bounds", "bounds only      "), ("param", "basis only       "), ("bounds+param", "bounds + basis   ")):
        v, s = stats(t[key])
        say(f"{label} grape_eval {v:.2f} +- {s:.2f} us   above slice mode by {v - sl:.2f} us (spread {max(sl_s, s):.2f} us)   "
            f"F = {F[key]!r}")
    for key in keys:
        say(f"  kernels {key}: {names[key]}")
    eng.close()
    if a.other:
        say(f"# 2. slice-mode grape_eval, fresh processes in turn, {a.blocks} blocks of {a.calls} calls each: this build / the other build")
        res = {"this": [], "other": []}
        for rnd in range(2):
            for key, path in (("this", qoc.library_path()), ("other", a.other)):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--blocks", str(a.blocks),
                                    "--calls", str(a.calls)], capture_output=True, text=True, timeout=300)
                if p.returncode:
                    say(f"{key}: child failed: {p.stderr[-500:]}")
                    continue
                d = json.loads(p.stdout.strip().splitlines()[-1])
                res[key].append(d)
                say(f"{key:5s} build, run {rnd + 1}: grape_eval {d['us']:.2f} +- {d['spread']:.2f} us   F = {d['F']!r}   ABI {d['abi']}")
        if res["this"] and res["other"]:
            a_, b_ = np.mean([d["us"] for d in res["this"]]), np.mean([d["us"] for d in res["other"]])
            sp = max(d["spread"] for d in res["this"] + res["other"])
            say(f"this build {a_:.2f} us, other build {b_:.2f} us: difference {a_ - b_:+.2f} us, block-to-block spread {sp:.2f} us; "
                f"F equal: {res['this'][0]['F'] == res['other'][0]['F']}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
