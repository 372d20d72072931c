"""What the soft worst-case objective (grape_set_risk) costs on the headline config -- C3: 4 x 4, K = 4, N = 500, E = 1024 --
blocking host->host as tools/bounds_time.py measures the bounds:

  1. grape_eval with the risk off and on (beta = 4) on ONE context, alternating blocks after a warm-up (clock drift and other
     tenants' work hit both alike); per call: median over the blocks of the block means, and the spread between blocks (half
     the 10 % .. 90 % range).  On: the sweep also writes the members' unweighted rows (16 MB), risk_weights_kernel and the
     two-stage weighted reduction read them, and the staged publication stands in for reduce_rows_mf_kernel.
  2. grape_eval with the risk off of THIS build against another build of the library (the parent commit's libgrape_hip.so,
     given with --other): fresh child processes, this / other / this / other, each through the same raw ctypes calls (the
     other build need not export the new entry points).  The difference must lie inside the spread between this build's own
     processes, and F must be the same bit for bit: a context without a risk did not move.

Usage: python tools/risk_time.py [--blocks 21] [--calls 300] [--other PATH/libgrape_hip.so] [--out FILE]"""
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

BETA = 4.0


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
    say(f"# tools/risk_time.py: C3 n={w.n} K={w.K} N={w.N} E={w.E}, beta = {BETA}; blocking host->host calls")
    say(f"# 1. one context, {a.blocks} alternating blocks of {a.calls} calls; us per call: median of the block means "
        "+- half the 10..90 % range between blocks")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    xf = np.ascontiguousarray(w.x.T)
    G = np.empty_like(xf)
    keys = ("off", "on")
    names, t, F, ws = {}, {k: [] for k in keys}, {}, {}

    def mode(key):
        eng.set_risk(BETA if key == "on" else 0.0)
        return lambda: eng.eval_cm(xf, G)
    for key in keys:
        fn = mode(key)
        for _ in range(100):
            fn()
        names[key] = ";".join(eng.kernel_names())
        ws[key] = eng.info["workspace_bytes"]
    for _ in range(a.blocks):
        for key in keys:
            fn = mode(key)                                   # (the setter synchronises: outside the timed loop)
            F[key] = fn()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            t[key].append((time.perf_counter() - t0) / a.calls)
    off, off_s = stats(t["off"])
    on, on_s = stats(t["on"])
    p = eng.risk_weights()
    say(f"risk off          grape_eval {off:.2f} +- {off_s:.2f} us   F = {F['off']!r}")
    say(f"risk on (beta={BETA:g}) grape_eval {on:.2f} +- {on_s:.2f} us   above the mean by {on - off:.2f} us (spread "
        f"{max(off_s, on_s):.2f} us)   F = {F['on']!r}")
    say(f"  p: sum {p.sum()!r} (W = {w.wts.sum()!r}), max p_k / w_k = {(p / w.wts).max():.4f}, min {(p / w.wts).min():.4f}")
    say(f"  workspace_bytes: {ws['off']} before the first evaluation under a risk, {ws['on']} with its buffers")
    for key in keys:
        say(f"  kernels {key}: {names[key]}")
    eng.close()
    if a.other:
        say(f"# 2. grape_eval, risk off, fresh processes in turn, {a.blocks} blocks of {a.calls} calls each: this build / the other build")
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
            say(f"this build {a_:.2f} us, other build {b_:.2f} us: difference {a_ - b_:+.2f} us; between this build's own processes "
                f"{own:.2f} us, block-to-block spread {sp:.2f} us; F equal: {res['this'][0]['F'] == res['other'][0]['F']}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
