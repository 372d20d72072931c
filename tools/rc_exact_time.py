"""What the exact gradient of the running cost (grape_set_running_cost_derivative, GRAPE_TRAJ_EXACT) costs on the headline config
-- C3: 4 x 4 UnitaryGate, K = 4, N = 500, E = 1024 -- in ONE process and ONE context, in alternating blocks after a warm-up
block (every block sets each variant in turn and times it); per variant the median over the blocks of the block means and the
spread between blocks (half the 10 % .. 90 % range):

  (a) grape_eval_device from HIP events (torch.cuda.Event around a block of back-to-back calls on one stream):
        without a running cost
        with a one-term cost (C6: R = Xt), first order:  + running_cost_kernel + running_cost_fold_kernel
        with it, exact:   + running_cost_exact_kernel + traj_frechet_rows_kernel + running_cost_fold_kernel
  (b) grape_eval, host array to host array, blocking: the same three variants, wall clock.
  (c) grape_eval (no running cost) of THIS build against another build of the library (the parent commit's libgrape_hip.so,
      --other): fresh child processes in turn.  "Did not move" holds only if the difference lies inside the spread between
      this build's own processes; F must be equal bit for bit.

Usage: python tools/rc_exact_time.py [--blocks 11] [--calls 20] [--other PATH/libgrape_hip.so] [--out FILE]"""
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

VARIANTS = ("no running cost", "first order", "exact")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=11)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--other", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.blocks, a.calls)
    import torch
    out = open(a.out, "w") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    w = qoc.workloads.config("C3")
    m = w.Xi.shape[2]
    E, N, K, n = w.E, w.N, w.K, w.n
    R = np.asarray(w.Xt, complex)[None]                        # one term, the C6 probe
    rho = np.full((1, N), -1.5 / (N * n * n))
    xd = torch.from_numpy(np.ascontiguousarray(w.x.T)).cuda()
    fg = torch.empty(K * N + 1, dtype=torch.float64, device="cuda")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    ws0 = eng.info["workspace_bytes"]
    say(f"# tools/rc_exact_time.py: C3 n={n} m={m} K={K} N={N} E={E}; one-term running cost (R = Xt)")

    def setting(variant):
        if variant == "no running cost":
            eng.set_running_cost(None)
            return
        eng.set_running_cost_derivative("exact" if variant == "exact" else "first_order")
        eng.set_running_cost(R, rho)

    def gpu_us(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e-3 * e0.elapsed_time(e1) / calls              # seconds per call (stats() reports us)

    def wall(fn, calls):
        fn()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t0) / calls

    t, names, F = {}, {}, {}
    for blk in range(a.blocks + 1):
        rec = {}
        for v in VARIANTS:
            setting(v)
            rec[f"dev {v}"] = gpu_us(lambda: eng.eval_device(xd.data_ptr(), fg.data_ptr()), a.calls)
            names[v] = ";".join(eng.kernel_names())
            rec[f"host {v}"] = wall(lambda: eng.eval(w.x), a.calls)
            F[v] = eng.eval(w.x)[0]
        if blk:
            for k, val in rec.items():
                t.setdefault(k, []).append(val)
    say(f"# (a) grape_eval_device from HIP events, (b) grape_eval host -> host blocking; {a.blocks} alternating blocks of {a.calls} "
        "back-to-back calls (one warm-up block in front); us per call: median of the block means +- half the 10..90 % range")
    base_d, base_h = stats(t["dev no running cost"])[0], stats(t["host no running cost"])[0]
    for v in VARIANTS:
        d, d_s = stats(t[f"dev {v}"])
        h, h_s = stats(t[f"host {v}"])
        say(f"{v:16s} device {d:8.2f} +- {d_s:5.2f} us ({d - base_d:+8.2f})   host {h:8.2f} +- {h_s:5.2f} us ({h - base_h:+8.2f})   F = {F[v]!r}")
    for v in VARIANTS:
        say(f"  kernels, {v}: {names[v]}")
    say(f"  F with the cost, first order == exact (J keeps its bits): {F['first order'] == F['exact']}")
    ws1 = eng.info["workspace_bytes"]
    say(f"  grape_info.workspace_bytes: {ws0 / 1e6:.1f} MB at creation, {ws1 / 1e6:.1f} MB at the end "
        f"(+{(ws1 - ws0) / 1e6:.1f} MB: the members' rows and the per-slice blocks)")
    eng.close()

    if a.other:
        say("# (c) grape_eval without a running cost, fresh processes in turn, 21 blocks of 300 calls each: this build / the other build")
        res = {"this": [], "other": []}
        for rnd in range(2):
            for key, path in (("this", qoc.library_path()), ("other", a.other)):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--blocks", "21", "--calls", "300"],
                                   capture_output=True, text=True, timeout=300)
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
