"""What parameter mode (grape_set_basis) costs on the headline config -- C3: 4 x 4, K = 4, N = 500, E = 1024 -- with M = 16
Fourier columns, blocking host->host as tools/fom_time.py measures it:

  1. slice mode against parameter mode on ONE context, alternating blocks after a warm-up (clock drift and other tenants'
     work hit both alike); per call: median over the blocks of the block means, and the spread between blocks (half the
     10 % .. 90 % range).  The difference is what basis_expand_kernel + basis_project_kernel add.
  2. slice-mode grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, given
     with --other): fresh child processes, this / other / this / other, each through the same raw ctypes calls (the other
     build need not export the new entry points).  They must agree within the block-to-block spread: nothing existing moved.
  3. grape_lbfgs in slice mode and over the 16 coefficients per control: iterations, evaluations and wall time until both
     have reached a common F (the higher of the two minima after `--iterations` iterations).

Usage: python tools/basis_time.py [--blocks 21] [--calls 300] [--other PATH/libgrape_hip.so] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quoptimalcontrol_jl_amd as qoc  # noqa: E402
from quoptimalcontrol_jl_amd.engine import GrapeConfig, MAX_DEVICES, _cm  # noqa: E402

M_FREQ = 8                                                     # 2 x 8 = 16 columns


def stats(samples):
    s = np.asarray(samples) * 1e6
    return float(np.median(s)), float(0.5 * (np.percentile(s, 90) - np.percentile(s, 10)))


def basis(w):
    return qoc.fourier_basis(w.N, w.T, 2 * np.pi / w.T * np.arange(1, M_FREQ + 1))


def child(lib_path, blocks, calls):
    """slice-mode grape_eval through raw ctypes on the library at lib_path; prints one JSON line"""
    w = qoc.workloads.config("C3")
    L = C.CDLL(lib_path)
    ids = (C.c_int32 * MAX_DEVICES)(*([0] * MAX_DEVICES))
    cfg = GrapeConfig(qoc.engine.SYS_TYPE_CODES[w.sys_type], 0, w.n, w.K, w.N, w.E, float(w.T), 0, 0, 0, 0, -1, 1, 0, 0, ids, 0, 0)
    h = C.c_void_p()
    assert L.grape_create(C.byref(cfg), C.byref(h)) == 0
    ops = [_cm(w.A), _cm(w.B), _cm(w.Xi), _cm(w.Xt), np.ascontiguousarray(w.wts, dtype=np.float64)]
    assert L.grape_set_operators(h, *[C.c_void_p(a.ctypes.data) for a in ops]) == 0
    xf = np.ascontiguousarray(w.x.T)
    G, F = np.empty_like(xf), C.c_double()
    px, pg, pF = C.c_void_p(xf.ctypes.data), C.c_void_p(G.ctypes.data), C.byref(F)
    for _ in range(200):
        assert L.grape_eval(h, px, pF, pg) == 0
    t = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(calls):
            L.grape_eval(h, px, pF, pg)
        t.append((time.perf_counter() - t0) / calls)
    L.grape_destroy(h)
    med, spread = stats(t)
    print(json.dumps({"us": med, "spread": spread, "F": F.value, "abi": L.grape_abi_version()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=60)
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
    say(f"# tools/basis_time.py: C3 n={w.n} K={w.K} N={w.N} E={w.E}, M = {M} Fourier columns; blocking host->host calls")
    say(f"# 1. one context, {a.blocks} alternating blocks of {a.calls} calls; us per call: median of the block means "
        "+- half the 10..90 % range between blocks")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    xf, tf = np.ascontiguousarray(w.x.T), np.zeros((M, w.K))
    Gx, Gt, Gi = np.empty_like(xf), np.empty_like(tf), np.empty_like(xf)
    # "ident": the identity basis, M = N -- the most projection workgroups a basis can have (K N / 4), each publishing
    names, t = {}, {"slice": [], "param": [], "ident": []}

    def mode(key):
        if key == "ident":
            eng.set_basis(np.eye(w.N), None)
            return lambda: eng.eval_cm(xf, Gi)
        eng.set_basis(phi if key == "param" else None, w.x if key == "param" else None)
        return (lambda: eng.eval_cm(tf, Gt)) if key == "param" else (lambda: eng.eval_cm(xf, Gx))
    for key in t:
        fn = mode(key)
        for _ in range(100):
            fn()
        names[key] = ";".join(eng.kernel_names())
    for _ in range(a.blocks):
        for key in t:
            fn = mode(key)                                   # (set_basis synchronises: outside the timed loop)
            fn()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            t[key].append((time.perf_counter() - t0) / a.calls)
    F_param = mode("param")()
    F_slice = mode("slice")()
    sl, sl_s = stats(t["slice"])
    pa, pa_s = stats(t["param"])
    say(f"slice mode      grape_eval {sl:.2f} +- {sl_s:.2f} us")
    say(f"parameter mode  grape_eval {pa:.2f} +- {pa_s:.2f} us   above slice mode by {pa - sl:.2f} us (spread {max(sl_s, pa_s):.2f} us)   "
        f"F(theta = 0, x0 = x) {F_param!r} vs F(x) {F_slice!r}")
    idn, idn_s = stats(t["ident"])
    say(f"identity basis  grape_eval {idn:.2f} +- {idn_s:.2f} us   above slice mode by {idn - sl:.2f} us   (M = N = {w.N}: "
        f"{(w.K * w.N + 3) // 4} projection workgroups)")
    for key in t:
        say(f"  kernels {key}: {names[key]}")
    # 3. the device-resident optimiser
    say(f"# 3. grape_lbfgs (Hager-Zhang), slice mode against M = {M}: until both have reached the higher of their minima "
        f"after {a.iterations} iterations")
    runs = {}
    for key in ("slice", "param"):
        mode(key)
        start = w.x if key == "slice" else np.zeros((w.K, M))
        eng.lbfgs(start, iterations=3)                       # warm-up
        runs[key] = (start, eng.lbfgs(start, iterations=a.iterations)[1])
    target = max(r[1]["minimum"] for r in runs.values())
    for key in ("slice", "param"):
        mode(key)
        start, full = runs[key]
        info = full
        for k in range(1, a.iterations + 1):
            info = eng.lbfgs(start, iterations=k)[1]
            if info["minimum"] <= target:
                break
        say(f"{key:6s} vector length {start.size:5d}: minimum after {a.iterations} iterations {full['minimum']:.9f} "
            f"({full['evaluations']} evaluations, {full['seconds'] * 1e3:.2f} ms); F <= {target:.9f} after {info['iterations']} "
            f"iterations, {info['evaluations']} evaluations, {info['seconds'] * 1e3:.2f} ms "
            f"({info['seconds'] * 1e6 / max(1, info['evaluations']):.1f} us per evaluation)")
    eng.close()
    # 2. this build against the other one, slice mode
    if a.other:
        say(f"# 2. slice-mode grape_eval, fresh processes in turn, {a.blocks} blocks of {a.calls} calls each: this build / the other build")
        res = {"this": [], "other": []}
        for rnd in range(2):
            for key, path in (("this", qoc.library_path()), ("other", a.other)):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--blocks", str(a.blocks),
                                    "--calls", str(a.calls)], capture_output=True, text=True, timeout=600)
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
