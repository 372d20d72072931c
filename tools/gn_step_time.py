"""What one Levenberg-Marquardt inner solve costs on the headline config -- C3: 4 x 4 UnitaryGate, K = 4, N = 500, E = 1024 -- for
n_obs = 1, 4 and 16 shared probes with per-member weight blocks (3 (N+1) n_obs E doubles: 12 / 49 / 197 MB) and wf, in ONE
process and ONE context, in alternating blocks after a warm-up block; per variant the median over the blocks of the block means
and the spread between blocks (half the 10 % .. 90 % range):

  (a) blocking, host to host: what fit_trajectory's host path does per iteration for a solve of 20 CG iterations (observe, the
      weights in NumPy, observe_vjp, then gauss_newton._cg over observe_gnvp, cg_rtol = 0) against ONE GrapeEngine.gn_step
      (cg_iter = 20, cg_rtol = 0), and gn_step with cg_iter = 0 (the sweep, the upload, the residuals and the pull-back alone)
  (b) per CG iteration: (gn_step(20) - gn_step(0)) / 20 from (a), wall clock with the host's look at the record after every
      block of 4 in it, against trajectory_gnvp_kernel + vjp_sum_kernel alone from HIP events (gnvp_device, d_x = NULL, the
      same per-member weights).  gn_step is blocking on the context's own stream, so HIP events cannot bracket its kernels from outside; the
      kernels' own times come from a kernel trace of `--trace-child` (rocprofv3 --kernel-trace --stats -- python
      tools/gn_step_time.py --trace-child), which runs 5 solves per probe count and nothing else
  (c) grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, --other): fresh
      child processes in turn.  "Did not move" holds only if the difference lies inside the spread between each build's own
      two processes; F must be equal bit for bit.

Usage: python tools/gn_step_time.py [--blocks 7] [--other PATH/libgrape_hip.so] [--out FILE]"""
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
from quoptimalcontrol_jl_amd import gauss_newton as gn  # noqa: E402

N_OBS = (1, 4, 16)
CG = 20


def problem():
    w = qoc.workloads.config("C3")
    m = w.Xi.shape[2]
    E, N, n = w.E, w.N, w.n
    rng = np.random.default_rng(1)
    cplx = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    O = cplx(16, n, m)
    O[0] = w.Xi[0]
    la, lb, lc = rng.uniform(0.3, 1.2, (E, 16, N + 1)), rng.standard_normal((E, 16, N + 1)), rng.uniform(0.3, 1.2, (E, 16, N + 1))
    planes = np.stack([la * la, la * lb, lb * lb + lc * lc])      # positive definite blocks per member, (3, E, 16, N+1)
    return w, m, O, planes, rng.uniform(0.2, 1.5, E), cplx(E, 16, N + 1), cplx(E, n, m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--other", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.blocks, a.calls)
    w, m, O, planes, wf, yt, xt = problem()
    E, N, K, n = w.E, w.N, w.K, w.n
    lam = 1.0
    if not a.trace_child:
        import torch
        torch.zeros(1, device="cuda")                             # (torch opens the device first, as in the other timing tools)
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)

    def device_solve(j, iters=CG):
        return eng.gn_step(w.x, O[:j], y_target=yt[:, :j], w=planes[:, :, :j], xf_target=xt, wf=wf, lam=lam, cg_iter=iters, cg_rtol=0.0)

    if a.trace_child:
        for j in N_OBS:
            for _ in range(5):
                device_solve(j)
        eng.close()
        return
    out = open(a.out, "w") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def host_solve(j):
        """fit_trajectory's host path at one x: the residuals, the gradient, 20 CG iterations over observe_gnvp"""
        Oj, wj = O[:j], planes[:, :, :j]
        y, Xf = eng.observe(w.x, Oj, final=True)
        r, d = y - yt[:, :j], Xf - xt
        ybar, xbar = gn.apply_weights(wj, r), wf[:, None, None] * d
        L = 0.5 * float(np.sum(np.real(np.conj(r) * ybar))) + 0.5 * float(np.sum(np.real(np.conj(d) * xbar)))
        g = eng.observe_vjp(w.x, Oj, ybar=ybar, xbar_final=xbar)
        H = gn.gn_operator(eng, w.x, Oj, wj, wf)
        p, Ap = gn._cg(lambda v: H(v) + lam * v, -g, CG, 0.0)
        return L, g, p

    def wall(fn, calls):
        fn()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t0) / calls

    say(f"# tools/gn_step_time.py: C3 n={n} m={m} K={K} N={N} E={E}; per-member weight blocks, "
        f"{24 * E * (N + 1) / 1e6:.1f} MB per probe; one solve = {CG} CG iterations, cg_rtol = 0, lam = {lam}")
    say(f"# (a) blocking host -> host, {a.blocks} alternating blocks (one warm-up block in front); ms per solve: median of the block "
        "means +- half the 10..90 % range between blocks")
    t = {}
    for blk in range(a.blocks + 1):
        rec = {}
        for j in N_OBS:
            rec[f"host {j}"] = wall(lambda: host_solve(j), 1)
            rec[f"dev {j}"] = wall(lambda: device_solve(j), 3)
            rec[f"dev0 {j}"] = wall(lambda: device_solve(j, 0), 3)
        if blk:
            for k, v in rec.items():
                t.setdefault(k, []).append(v)
    ms = lambda k: tuple(1e-3 * v for v in stats(t[k]))
    per_it = {}
    for j in N_OBS:
        (h, hs), (d, ds), (d0, d0s) = ms(f"host {j}"), ms(f"dev {j}"), ms(f"dev0 {j}")
        per_it[j] = stats((np.asarray(t[f"dev {j}"]) - np.asarray(t[f"dev0 {j}"])) / CG)
        say(f"n_obs={j:<2d} host path {h:9.2f} +- {hs:6.2f} ms   gn_step {d:8.2f} +- {ds:5.2f} ms   host / gn_step = {h / d:6.1f}   "
            f"gn_step(cg_iter = 0) {d0:8.2f} +- {d0s:5.2f} ms")
    L, g, p = host_solve(4)
    s = device_solve(4)
    say(f"  n_obs = 4: |L_dev - L_host| / L = {abs(s['loss'] - L) / L:.2e}   |g_dev - g_host|_inf / |g|_inf = "
        f"{np.abs(s['g'] - g).max() / np.abs(g).max():.2e}   |p_dev - p_host| / |p| = {np.linalg.norm(s['p'] - p) / np.linalg.norm(p):.2e} "
        f"({CG} truncated iterations)   status {s['status']} iterations {s['iterations']}")
    say(f"  kernels: {';'.join(eng.kernel_names())}")

    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    cm = qoc.engine._cm
    xd, xdd, wfd = dev(w.x.T), dev(np.random.default_rng(2).standard_normal((N, K))), dev(wf)
    Gd = torch.empty((N, K), dtype=torch.float64, device="cuda")
    fg = torch.empty(K * N + 1, dtype=torch.float64, device="cuda")
    Xfd = torch.empty((E, m, n), dtype=torch.complex128, device="cuda")
    say(f"# (b) per CG iteration, us: gn_step's (wall clock, the look at the record after every block of 4 in it) against the "
        f"product's kernels alone (HIP events, {a.blocks} blocks of 40 back-to-back gnvp_device(NULL) calls)")
    for j in N_OBS:
        Od, wd = dev(cm(O[:j])), dev(planes[:, :, :j])        # (the same per-member blocks: like against like)
        eng.observe_device(xd.data_ptr(), 0, False, 0, 0, Xfd.data_ptr(), fg.data_ptr())
        tk = []
        for blk in range(a.blocks + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            call = lambda: eng.observe_gnvp_device(0, xdd.data_ptr(), j, False, Od.data_ptr(), 1, wd.data_ptr(), wfd.data_ptr(), Gd.data_ptr())
            call()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(40):
                call()
            e1.record()
            e1.synchronize()
            if blk:
                tk.append(1e-3 * e0.elapsed_time(e1) / 40)
        k_us, k_s = stats(tk)
        say(f"n_obs={j:<2d} gn_step per iteration {per_it[j][0]:8.2f} +- {per_it[j][1]:5.2f} us   trajectory_gnvp_kernel + vjp_sum_kernel "
            f"{k_us:8.2f} +- {k_s:5.2f} us   difference {per_it[j][0] - k_us:+8.2f} us")
    say(f"  workspace_bytes {eng.info['workspace_bytes']}")
    eng.close()

    if a.other:
        say("# (c) grape_eval, fresh processes in turn, 21 blocks of 300 calls each: this build / the other build")
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
        if len(res["this"]) == 2 and len(res["other"]) == 2:
            a_, b_ = np.mean([d["us"] for d in res["this"]]), np.mean([d["us"] for d in res["other"]])
            own = abs(res["this"][0]["us"] - res["this"][1]["us"])
            oth = abs(res["other"][0]["us"] - res["other"][1]["us"])
            say(f"this build {a_:.2f} us, other build {b_:.2f} us: difference {a_ - b_:+.2f} us; this build's own two processes "
                f"differ by {own:.2f} us, the other build's by {oth:.2f} us; F equal: {res['this'][0]['F'] == res['other'][0]['F']}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
