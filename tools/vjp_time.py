"""What the vector-Jacobian product of the trajectory read-out (grape_eval_vjp) costs on the headline config -- C3: 4 x 4
UnitaryGate, K = 4, N = 500, E = 1024 -- blocking host->host, as tools/observe_time.py measures:

  1. grape_eval, grape_eval under a one-term running cost (the nearest existing work: one pair of backward walks per member
     behind the sweep) and observe_vjp with n_obs = 1, 4 and 16 (shared probes, ybar and Xbar_final) on ONE context,
     alternating blocks after a warm-up (clock drift and other tenants' work hit all alike); per call: median over the blocks
     of the block means, and the spread between blocks (half the 10 % .. 90 % range).  The VJP's call also copies ybar to
     the device, (E, n_obs, N+1) complex128.
  2. the kernels' own time from GRAPE_FLAG_TIME_KERNELS (HIP events around the launches of an evaluation) on a second
     context: the mean of an evaluation alone, of one under the running cost, and of one with trajectory_vjp_kernel and
     vjp_sum_kernel behind it; the differences are the running-cost kernels' and the new kernels'.
  3. grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, given with
     --other): fresh child processes, this / other / this / other, each through the same raw ctypes calls (the other build
     need not export the new entry point).  "Did not move" holds only if the difference lies inside the spread between this
     build's own processes; F must be equal bit for bit.

Usage: python tools/vjp_time.py [--blocks 21] [--calls 300] [--other PATH/libgrape_hip.so] [--out FILE]"""
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
    ybar = rng.standard_normal((w.E, 16, w.N + 1)) + 1j * rng.standard_normal((w.E, 16, w.N + 1))
    xbar = rng.standard_normal((w.E, w.n, m)) + 1j * rng.standard_normal((w.E, w.n, m))
    yb = {j: np.ascontiguousarray(ybar[:, :j]) for j in N_OBS}
    R, rho = w.Xt[None], np.full((1, w.N), 1.0 / w.N)
    say(f"# tools/vjp_time.py: C3 n={w.n} m={m} K={w.K} N={w.N} E={w.E}; blocking host->host calls; ybar is "
        f"(E, n_obs, N+1) complex128 = {16 * w.E * (w.N + 1) / 1e6:.1f} MB per probe, uploaded by every call")
    say(f"# 1. one context, {a.blocks} alternating blocks of {a.calls} calls; us per call: median of the block means "
        "+- half the 10..90 % range between blocks")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    xf = np.ascontiguousarray(w.x.T)
    G = np.empty_like(xf)

    fns = {"eval": lambda: eng.eval_cm(xf, G)}
    for j in N_OBS:
        fns[f"vjp n_obs={j}"] = (lambda j=j: eng.observe_vjp(w.x, O[:j], ybar=yb[j], xbar_final=xbar))
    names, t, F = {}, {k: [] for k in list(fns) + ["eval_rc"]}, {}
    for key, fn in fns.items():
        for _ in range(30 if key == "eval" else 3):
            fn()
        names[key] = ";".join(eng.kernel_names())
    for _ in range(a.blocks):
        for key, fn in fns.items():
            calls = a.calls if key == "eval" else max(1, a.calls // 30)     # (the VJP's calls move megabytes to the device)
            F[key] = fn()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t[key].append((time.perf_counter() - t0) / calls)
        eng.set_running_cost(R, rho)                           # the setter stays outside the timed region
        eng.eval_cm(xf, G)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            eng.eval_cm(xf, G)
        t["eval_rc"].append((time.perf_counter() - t0) / a.calls)
        names["eval_rc"] = ";".join(eng.kernel_names())
        eng.set_running_cost(None)
    ev, ev_s = stats(t["eval"])
    rc, rc_s = stats(t["eval_rc"])
    say(f"grape_eval                         {ev:.2f} +- {ev_s:.2f} us   F = {F['eval']!r}")
    say(f"grape_eval, one-term running cost  {rc:.2f} +- {rc_s:.2f} us   above grape_eval by {rc - ev:.2f} us")
    for j in N_OBS:
        v, s = stats(t[f"vjp n_obs={j}"])
        say(f"grape_eval_vjp n_obs={j:<2d}            {v:.2f} +- {s:.2f} us   above grape_eval by {v - ev:.2f} us   "
            f"({16 * w.E * (w.N + 1) * j / 1e6:.1f} MB of ybar per call)")
    for key in names:
        say(f"  kernels {key}: {names[key]}")
    G1 = eng.observe_vjp(w.x, O[:4], ybar=yb[4], xbar_final=xbar)
    G2 = eng.observe_vjp(w.x, O[:4], ybar=yb[4], xbar_final=xbar)
    say(f"  observe_vjp bitwise call to call: {np.array_equal(G1, G2)}; eval F after it unchanged: {eng.eval_cm(xf, G) == F['eval']}")
    eng.close()

    say("# 2. kernel time per evaluation from HIP events (GRAPE_FLAG_TIME_KERNELS), 200 evaluations each (VJP: 40)")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0, flags=qoc.engine.FLAG_TIME_KERNELS)
    for _ in range(20):
        eng.eval_cm(xf, G)
    eng.kernel_time(reset=True)
    for _ in range(200):
        eng.eval_cm(xf, G)
    ms, cnt = eng.kernel_time(reset=True)
    base = 1e3 * ms / cnt
    say(f"evaluation alone                   {base:.2f} us")
    eng.set_running_cost(R, rho)
    for _ in range(5):
        eng.eval_cm(xf, G)
    eng.kernel_time(reset=True)
    for _ in range(200):
        eng.eval_cm(xf, G)
    ms, cnt = eng.kernel_time(reset=True)
    say(f"with a one-term running cost       {1e3 * ms / cnt:.2f} us   running_cost_kernel + fold alone {1e3 * ms / cnt - base:.2f} us")
    eng.set_running_cost(None)
    for j in N_OBS:
        for _ in range(3):
            eng.observe_vjp(w.x, O[:j], ybar=yb[j], xbar_final=xbar)
        eng.kernel_time(reset=True)
        for _ in range(40):
            eng.observe_vjp(w.x, O[:j], ybar=yb[j], xbar_final=xbar)
        ms, cnt = eng.kernel_time(reset=True)
        say(f"with the VJP kernels, n_obs={j:<2d}     {1e3 * ms / cnt:.2f} us   trajectory_vjp_kernel + vjp_sum_kernel alone "
            f"{1e3 * ms / cnt - base:.2f} us")
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
        if len(res["this"]) == 2 and res["other"]:
            a_, b_ = np.mean([d["us"] for d in res["this"]]), np.mean([d["us"] for d in res["other"]])
            own = abs(res["this"][0]["us"] - res["this"][1]["us"])
            sp = max(d["spread"] for d in res["this"] + res["other"])
            say(f"this build {a_:.2f} us, other build {b_:.2f} us: difference {a_ - b_:+.2f} us; this build's own two processes "
                f"differ by {own:.2f} us, block-to-block spread {sp:.2f} us; F equal: {res['this'][0]['F'] == res['other'][0]['F']}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
