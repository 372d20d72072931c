"""What a running cost (grape_set_running_cost) costs on the headline config -- C3: 4 x 4, K = 4, N = 500, E = 1024 --
blocking host->host, with the method of tools/basis_time.py:

  1. one context, alternating blocks after a warm-up: the term off, one C6 term (R = Xt), four terms; per call the median
     over the blocks of the block means and the spread between blocks (half the 10 % .. 90 % range).
  2. the off path of THIS build against another build of the library (the parent commit's libgrape_hip.so, --other): fresh
     child processes in turn through the same raw ctypes calls; F must be equal bit for bit and the times must agree within
     the block-to-block spread.
  --profile-child: one context with one C6 term evaluating in a loop, for a `rocprofv3 --kernel-trace --stats` run of its
     own (the kernel's own time; the program goes behind `--`).

Usage: python tools/running_cost_time.py [--blocks 21] [--calls 300] [--other PATH/libgrape_hip.so] [--out FILE]"""
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


def terms(w, J):
    rng = np.random.default_rng(1)
    R = rng.standard_normal((J, w.E, w.n, w.n)) + 1j * rng.standard_normal((J, w.E, w.n, w.n))
    R[0] = w.Xt
    rho = np.full((J, w.N), -1.0 / (w.N * w.n * w.n))
    return R, rho


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--other", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--profile-child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.blocks, a.calls)
    w = qoc.workloads.config("C3")
    if a.profile_child:
        with qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0) as eng:
            eng.set_running_cost(*terms(w, 1))
            xf = np.ascontiguousarray(w.x.T)
            G = np.empty_like(xf)
            for _ in range(a.profile_child):
                eng.eval_cm(xf, G)
        return
    out = open(a.out, "w") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    say(f"# tools/running_cost_time.py: C3 n={w.n} K={w.K} N={w.N} E={w.E}; blocking host->host calls")
    say(f"# 1. one context, {a.blocks} alternating blocks of {a.calls} calls; us per call: median of the block means "
        "+- half the 10..90 % range between blocks")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    xf = np.ascontiguousarray(w.x.T)
    G = np.empty_like(xf)
    settings = {"off": None, "one C6 term": terms(w, 1), "four terms": terms(w, 4)}
    t, names, Fs = {k: [] for k in settings}, {}, {}

    def mode(key):
        if settings[key] is None:
            eng.set_running_cost(None)
        else:
            eng.set_running_cost(*settings[key])
    for key in settings:
        mode(key)
        for _ in range(100):
            Fs[key] = eng.eval_cm(xf, G)
        names[key] = ";".join(eng.kernel_names())
    for _ in range(a.blocks):
        for key in settings:
            mode(key)                                        # (synchronises: outside the timed loop)
            eng.eval_cm(xf, G)
            t0 = time.perf_counter()
            for _ in range(a.calls):
                eng.eval_cm(xf, G)
            t[key].append((time.perf_counter() - t0) / a.calls)
    base = stats(t["off"])
    for key in settings:
        med, sp = stats(t[key])
        say(f"{key:12s} grape_eval {med:8.2f} +- {sp:.2f} us   above off by {med - base[0]:8.2f} us   F = {Fs[key]!r}")
    for key in settings:
        say(f"  kernels {key}: {names[key]}")
    info = eng.info
    say(f"  unitary_flow {info['unitary_flow']} lane_pair {info['lane_pair']} S {info['slices_per_lane']} W {info['waves_per_member']}")
    eng.close()
    if a.other:
        say(f"# 2. off path, fresh processes in turn, {a.blocks} blocks of {a.calls} calls each: this build / the other build")
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
