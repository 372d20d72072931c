"""What the read-out along the trajectory (grape_eval_observables) costs on the headline config -- C3: 4 x 4 UnitaryGate,
K = 4, N = 500, E = 1024 -- blocking host->host, as tools/bounds_time.py measures:

  1. grape_eval and grape_eval_observables with n_obs = 1, 4 and 16 (shared probes, y only) on ONE context, alternating
     blocks after a warm-up (clock drift and other tenants' work hit all alike); per call: median over the blocks of the block
     means, and the spread between blocks (half the 10 % .. 90 % range).  The read-out's call also copies y to the host.
  2. the kernels' own time from GRAPE_FLAG_TIME_KERNELS (HIP events around the launches of an evaluation) on a second
     context: the mean of an evaluation alone and of one with observe_kernel behind it; the difference is the new kernel's.
  3. grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, given with
     --other): fresh child processes, this / other / this / other, each through the same raw ctypes calls (the other build
     need not export the new entry point).  They must agree within the block-to-block spread and return the same F bit for
     bit: a context that never asks for the read-out did not move.

Usage: python tools/observe_time.py [--blocks 21] [--calls 300] [--other PATH/libgrape_hip.so] [--out FILE]"""
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
from basis_time import child, stats  # noqa: E402

N_OBS = (1, 4, 16)


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
    m = w.Xi.shape[2]
    rng = np.random.default_rng(1)
    O = rng.standard_normal((16, w.n, m)) + 1j * rng.standard_normal((16, w.n, m))
    O[0] = w.Xi[0]
    say(f"# tools/observe_time.py: C3 n={w.n} m={m} K={w.K} N={w.N} E={w.E}; blocking host->host calls; y is "
        f"(E, n_obs, N+1) complex128 = {16 * w.E * (w.N + 1) / 1e6:.1f} MB per probe")
    say(f"# 1. one context, {a.blocks} alternating blocks of {a.calls} calls; us per call: median of the block means "
        "+- half the 10..90 % range between blocks")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    xf = np.ascontiguousarray(w.x.T)
    G = np.empty_like(xf)
    fns = {"eval": lambda: eng.eval_cm(xf, G)}
    for j in N_OBS:
        fns[f"observe n_obs={j}"] = (lambda j=j: eng.observe(w.x, O[:j], want_F=True)[1])
    names, t, F = {}, {k: [] for k in fns}, {}
    for key, fn in fns.items():
        for _ in range(30):
            fn()
        names[key] = ";".join(eng.kernel_names())
    for _ in range(a.blocks):
        for key, fn in fns.items():
            calls = a.calls if key == "eval" else max(1, a.calls // 10)     # (the read-out's calls move megabytes to the host)
            F[key] = fn()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t[key].append((time.perf_counter() - t0) / calls)
    ev, ev_s = stats(t["eval"])
    say(f"grape_eval                        {ev:.2f} +- {ev_s:.2f} us   F = {F['eval']!r}")
    for j in N_OBS:
        v, s = stats(t[f"observe n_obs={j}"])
        say(f"grape_eval_observables n_obs={j:<2d}  {v:.2f} +- {s:.2f} us   above grape_eval by {v - ev:.2f} us   "
            f"F equal: {F[f'observe n_obs={j}'] == F['eval']}")
    for key in fns:
        say(f"  kernels {key}: {names[key]}")
    eng.close()

    say("# 2. kernel time per evaluation from HIP events (GRAPE_FLAG_TIME_KERNELS), 200 evaluations each")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0, flags=qoc.engine.FLAG_TIME_KERNELS)
    for _ in range(20):
        eng.eval_cm(xf, G)
    eng.kernel_time(reset=True)
    for _ in range(200):
        eng.eval_cm(xf, G)
    ms, cnt = eng.kernel_time(reset=True)
    base = 1e3 * ms / cnt
    say(f"evaluation alone                  {base:.2f} us")
    for j in N_OBS:
        for _ in range(5):
            eng.observe(w.x, O[:j])
        eng.kernel_time(reset=True)
        for _ in range(200):
            eng.observe(w.x, O[:j])
        ms, cnt = eng.kernel_time(reset=True)
        say(f"with observe_kernel, n_obs={j:<2d}     {1e3 * ms / cnt:.2f} us   observe_kernel alone {1e3 * ms / cnt - base:.2f} us")
    eng.close()

    if a.other:
        say(f"# 3. grape_eval, fresh processes in turn, {a.blocks} blocks of {a.calls} calls each: this build / the other build")
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
