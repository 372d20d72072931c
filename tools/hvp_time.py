"""What the second-order product along the trajectory (grape_eval_hvp / grape_eval_hvp_device) costs on the headline config
-- C3: 4 x 4 UnitaryGate, K = 4, N = 500, E = 1024 -- for n_obs = 1, 4 and 16 shared probes, in ONE process and ONE context,
in alternating blocks after a warm-up block; per variant the median over the blocks of the block means and the spread between
blocks (half the 10 % .. 90 % range):

  (a) the kernels' own time from HIP events (torch.cuda.Event around a block of back-to-back reuse calls on one stream, d_x =
      NULL: no sweep, no pulse map), the direct instances (GRAPE_TRAJ_STAGED=0):
        trajectory_hvp_kernel + vjp_sum_kernel                      hvp_device
        the work it fuses, launched in the same blocks:             one jvp_device (trajectory_jvp_kernel) and two vjp_device
                                                                    (trajectory_vjp_kernel + vjp_sum_kernel each)
  (b) one Newton-CG inner step at one linearisation point -- J v, then H v from the hand-made (ybar_dot, Xbar_dot) -- wall
      clock ending in a synchronise: through the host forms (two evaluations, every array crosses the bus), the device forms
      with d_x (two sweeps), and the device forms with reuse behind one observe_device (no sweep: what a CG iteration costs).
  (c) grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, --other): fresh
      child processes in turn.  "Did not move" holds only if the difference lies inside the spread between this build's own
      processes; F must be equal bit for bit.

Usage: python tools/hvp_time.py [--blocks 15] [--calls 40] [--other PATH/libgrape_hip.so] [--out FILE]"""
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
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40)
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
    rng = np.random.default_rng(1)
    cplx = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    O = cplx(16, n, m)
    O[0] = w.Xi[0]
    ybar, ybdot, xbar, xbdot = cplx(E, 16, N + 1), cplx(E, 16, N + 1), cplx(E, n, m), cplx(E, n, m)
    xdot = rng.standard_normal((K, N))
    cm = qoc.engine._cm
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    xd, xdd = dev(w.x.T), dev(xdot.T)
    Od = {j: dev(cm(O[:j])) for j in N_OBS}
    ybd = {j: dev(ybar[:, :j]) for j in N_OBS}
    ybdd = {j: dev(ybdot[:, :j]) for j in N_OBS}
    yb = {j: np.ascontiguousarray(ybar[:, :j]) for j in N_OBS}
    ybt = {j: np.ascontiguousarray(ybdot[:, :j]) for j in N_OBS}
    xbd, xbdd = dev(cm(xbar)), dev(cm(xbdot))
    yd = {j: torch.empty((E, j, N + 1), dtype=torch.complex128, device="cuda") for j in N_OBS}
    ydd = {j: torch.empty((E, j, N + 1), dtype=torch.complex128, device="cuda") for j in N_OBS}
    Xfd = torch.empty((E, m, n), dtype=torch.complex128, device="cuda")
    Xdd = torch.empty((E, m, n), dtype=torch.complex128, device="cuda")
    fg = torch.empty(K * N + 1, dtype=torch.float64, device="cuda")
    Gd = torch.empty((N, K), dtype=torch.float64, device="cuda")
    os.environ["GRAPE_TRAJ_STAGED"] = "0"                      # the direct instances throughout: like against like
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    say(f"# tools/hvp_time.py: C3 n={n} m={m} K={K} N={N} E={E}; ybar / ybar_dot are (E, n_obs, N+1) complex128 = "
        f"{16 * E * (N + 1) / 1e6:.1f} MB per probe; direct instances (GRAPE_TRAJ_STAGED=0)")

    def obs(j):
        eng.observe_device(xd.data_ptr(), j, False, Od[j].data_ptr(), yd[j].data_ptr(), Xfd.data_ptr(), fg.data_ptr())

    def vjp(j, reuse):
        eng.observe_vjp_device(0 if reuse else xd.data_ptr(), j, False, Od[j].data_ptr(), ybd[j].data_ptr(), xbd.data_ptr(), Gd.data_ptr())

    def jvp(j, reuse):
        eng.observe_jvp_device(0 if reuse else xd.data_ptr(), xdd.data_ptr(), j, False, Od[j].data_ptr(), ydd[j].data_ptr(), Xdd.data_ptr())

    def hvp(j, reuse):
        eng.observe_hvp_device(0 if reuse else xd.data_ptr(), xdd.data_ptr(), j, False, Od[j].data_ptr(), ybd[j].data_ptr(), xbd.data_ptr(),
                               ybdd[j].data_ptr(), xbdd.data_ptr(), Gd.data_ptr())

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

    # ------------------------------------------------------------------------------------------------------------------- (a)
    say(f"# (a) kernel time from HIP events, {a.blocks} alternating blocks of {a.calls} back-to-back reuse calls (one warm-up block "
        "in front); us per call: median of the block means +- half the 10..90 % range between blocks")
    t, names = {}, {}
    obs(16)
    for blk in range(a.blocks + 1):
        rec = {}
        for j in N_OBS:
            rec[f"hvp {j}"] = gpu_us(lambda: hvp(j, True), a.calls)
            names[f"hvp {j}"] = ";".join(eng.kernel_names())
            rec[f"jvp {j}"] = gpu_us(lambda: jvp(j, True), a.calls)
            rec[f"vjp {j}"] = gpu_us(lambda: vjp(j, True), a.calls)
        if blk:
            for k, v in rec.items():
                t.setdefault(k, []).append(v)
    for j in N_OBS:
        hv, hv_s = stats(t[f"hvp {j}"])
        jv, jv_s = stats(t[f"jvp {j}"])
        vj, vj_s = stats(t[f"vjp {j}"])
        fused, fused_s = stats(np.asarray(t[f"jvp {j}"]) + 2.0 * np.asarray(t[f"vjp {j}"]))
        say(f"n_obs={j:<2d} trajectory_hvp_kernel + vjp_sum_kernel {hv:8.2f} +- {hv_s:5.2f} us   trajectory_jvp_kernel {jv:8.2f} +- {jv_s:5.2f} us   "
            f"trajectory_vjp_kernel + vjp_sum_kernel {vj:8.2f} +- {vj_s:5.2f} us   jvp + 2 vjp (per block) {fused:8.2f} +- {fused_s:5.2f} us   "
            f"hvp / (jvp + 2 vjp) = {hv / fused:.2f}")
    say(f"  kernels hvp 16: {names['hvp 16']}")

    # ------------------------------------------------------------------------------------------------------------------- (b)
    say("# (b) one Newton-CG inner step (J v, then H v) at one point, wall clock ending in a synchronise; us per step")

    def wall(fn, calls):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls

    def host_step(j):
        eng.observe_jvp(w.x, xdot, O[:j], final=True)
        eng.observe_hvp(w.x, xdot, O[:j], yb[j], xbar, ybt[j], xbdot)

    def dev_step(j, reuse):
        jvp(j, reuse)
        hvp(j, reuse)

    tb = {}
    for blk in range(a.blocks):
        for j in N_OBS:
            tb.setdefault(f"host {j}", []).append(wall(lambda: host_step(j), max(2, a.calls // (2 * j))))
            tb.setdefault(f"dev {j}", []).append(wall(lambda: dev_step(j, False), a.calls))
            obs(j)
            tb.setdefault(f"reuse {j}", []).append(wall(lambda: dev_step(j, True), a.calls))
    for j in N_OBS:
        h, h_s = stats(tb[f"host {j}"])
        d, d_s = stats(tb[f"dev {j}"])
        r, r_s = stats(tb[f"reuse {j}"])
        say(f"n_obs={j:<2d} host forms {h:10.2f} +- {h_s:7.2f}   device forms {d:8.2f} +- {d_s:5.2f}   device forms with reuse {r:8.2f} +- {r_s:5.2f}")
    Gh = eng.observe_hvp(w.x, xdot, O[:4], yb[4], xbar, ybt[4], xbdot)
    hvp(4, False)
    torch.cuda.synchronize()
    G_d = Gd.cpu().numpy().T.copy()
    hvp(4, True)
    torch.cuda.synchronize()
    say(f"  device = host, bit for bit (n_obs = 4): Gdot {np.array_equal(G_d, Gh)}, reuse {np.array_equal(Gd.cpu().numpy().T, Gh)}")
    eng.close()

    # ------------------------------------------------------------------------------------------------------------------- (c)
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
