"""What the exact derivative mode of the trajectory pull-back / push-forward (grape_set_trajectory_derivative, GRAPE_TRAJ_EXACT)
costs on the headline config -- C3: 4 x 4 UnitaryGate, K = 4, N = 500, E = 1024 -- for n_obs = 1, 4 and 16 shared probes, in
ONE process and ONE context, in alternating blocks after a warm-up block (every block switches the mode, takes a fresh
read-out and times both modes' reuse calls); per variant the median over the blocks of the block means and the spread between
blocks (half the 10 % .. 90 % range):

  (a) the kernels' own time from HIP events (torch.cuda.Event around a block of back-to-back calls on one stream), the device
      forms with d_x = NULL (no sweep, no pulse map), GRAPE_TRAJ_STAGED=0 so that first order runs its direct instance too:
        pull-back     first order: trajectory_vjp_kernel + vjp_sum_kernel
                      exact:       trajectory_vjp_exact_kernel + traj_frechet_rows_kernel + vjp_sum_kernel
        push-forward  first order: trajectory_jvp_kernel
                      exact:       traj_frechet_dir_kernel + trajectory_jvp_exact_kernel
  (b) one Gauss-Newton inner step, J v then J' w along one stored trajectory (reuse behind one observe_device), wall clock
      ending in a synchronise, in both modes.
  (c) grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, --other): fresh
      child processes in turn.  "Did not move" holds only if the difference lies inside the spread between this build's own
      processes; F must be equal bit for bit.

Usage: python tools/traj_exact_time.py [--blocks 11] [--calls 20] [--other PATH/libgrape_hip.so] [--out FILE]"""
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
MODES = ("first_order", "exact")


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
    rng = np.random.default_rng(1)
    O = rng.standard_normal((16, n, m)) + 1j * rng.standard_normal((16, n, m))
    O[0] = w.Xi[0]
    ybar = rng.standard_normal((E, 16, N + 1)) + 1j * rng.standard_normal((E, 16, N + 1))
    xbar = rng.standard_normal((E, n, m)) + 1j * rng.standard_normal((E, n, m))
    xdot = rng.standard_normal((K, N))
    cm = qoc.engine._cm
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    xd, xdd = dev(w.x.T), dev(xdot.T)
    Od = {j: dev(cm(O[:j])) for j in N_OBS}
    ybd = {j: dev(ybar[:, :j]) for j in N_OBS}
    xbd = dev(cm(xbar))
    yd = {j: torch.empty((E, j, N + 1), dtype=torch.complex128, device="cuda") for j in N_OBS}
    ydd = {j: torch.empty((E, j, N + 1), dtype=torch.complex128, device="cuda") for j in N_OBS}
    Xfd = torch.empty((E, m, n), dtype=torch.complex128, device="cuda")
    Xdd = torch.empty((E, m, n), dtype=torch.complex128, device="cuda")
    fg = torch.empty(K * N + 1, dtype=torch.float64, device="cuda")
    Gd = torch.empty((N, K), dtype=torch.float64, device="cuda")
    os.environ["GRAPE_TRAJ_STAGED"] = "0"                      # the direct instances throughout: like against like
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    ws0 = eng.info["workspace_bytes"]
    say(f"# tools/traj_exact_time.py: C3 n={n} m={m} K={K} N={N} E={E}; direct instances (GRAPE_TRAJ_STAGED=0); reuse calls (d_x = NULL)")

    def obs(j):
        eng.observe_device(xd.data_ptr(), j, False, Od[j].data_ptr(), yd[j].data_ptr(), Xfd.data_ptr(), fg.data_ptr())

    def vjp(j):
        eng.observe_vjp_device(0, j, False, Od[j].data_ptr(), ybd[j].data_ptr(), xbd.data_ptr(), Gd.data_ptr())

    def jvp(j):
        eng.observe_jvp_device(0, xdd.data_ptr(), j, False, Od[j].data_ptr(), ydd[j].data_ptr(), Xdd.data_ptr())

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
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls

    def gn_step(j):
        jvp(j)
        vjp(j)

    # ------------------------------------------------------------------------------------------------------------- (a), (b)
    t, names = {}, {}
    for blk in range(a.blocks + 1):
        rec = {"eval_device": gpu_us(lambda: eng.eval_device(xd.data_ptr(), fg.data_ptr()), a.calls)}
        for mode in MODES:
            eng.set_trajectory_derivative(mode)
            for j in N_OBS:
                obs(j)                                         # the trajectory both reuse calls run along
                rec[f"vjp {mode} {j}"] = gpu_us(lambda: vjp(j), a.calls)
                names[f"vjp {mode}"] = ";".join(eng.kernel_names())
                rec[f"jvp {mode} {j}"] = gpu_us(lambda: jvp(j), a.calls)
                names[f"jvp {mode}"] = ";".join(eng.kernel_names())
                rec[f"gn {mode} {j}"] = wall(lambda: gn_step(j), a.calls)
        if blk:
            for k, v in rec.items():
                t.setdefault(k, []).append(v)
    say(f"# (a) kernel time from HIP events, {a.blocks} alternating blocks of {a.calls} back-to-back calls (one warm-up block in "
        "front); us per call: median of the block means +- half the 10..90 % range between blocks")
    ev, ev_s = stats(t["eval_device"])
    say(f"grape_eval_device (a first-order evaluation)          {ev:8.2f} +- {ev_s:5.2f} us")
    for what, label in (("vjp", "pull-back   "), ("jvp", "push-forward")):
        for j in N_OBS:
            f, f_s = stats(t[f"{what} first_order {j}"])
            x, x_s = stats(t[f"{what} exact {j}"])
            say(f"{label} n_obs={j:<2d} first order {f:8.2f} +- {f_s:5.2f} us   exact {x:8.2f} +- {x_s:5.2f} us   exact / first order = {x / f:.2f}   "
                f"exact / grape_eval_device = {x / ev:.2f}")
    for k in sorted(names):
        say(f"  kernels {k}: {names[k]}")
    say("# (b) one Gauss-Newton inner step (J v, then J' w) along one stored trajectory, wall clock ending in a synchronise; us per step")
    for j in N_OBS:
        f, f_s = stats(t[f"gn first_order {j}"])
        x, x_s = stats(t[f"gn exact {j}"])
        say(f"n_obs={j:<2d} first order {f:8.2f} +- {f_s:5.2f}   exact {x:8.2f} +- {x_s:5.2f}   exact / first order = {x / f:.2f}")
    ws1 = eng.info["workspace_bytes"]
    say(f"  grape_info.workspace_bytes: {ws0 / 1e6:.1f} MB before the first exact call, {ws1 / 1e6:.1f} MB after "
        f"(+{(ws1 - ws0) / 1e6:.1f} MB: the per-slice blocks and the kept pulse)")
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
