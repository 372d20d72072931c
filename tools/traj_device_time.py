"""What the device-resident trajectory read-out and VJP (grape_eval_observables_device / grape_eval_vjp_device) cost on the
headline config -- C3: 4 x 4 UnitaryGate, K = 4, N = 500, E = 1024 -- for n_obs = 1, 4 and 16 shared probes (section (a): 1, 2, 4, 8, 12, 16):

  (a) the direct against the staged instance of each kernel, on device-resident arrays, from HIP events (torch.cuda.Event
      around a block of back-to-back calls on one stream): ONE process, ONE context, alternating blocks after a warm-up; per
      variant the median over the blocks of the block means and the spread between blocks (half the 10 % .. 90 % range).
      The pull-back is timed through the reuse (d_x = NULL: trajectory_vjp_kernel + vjp_sum_kernel twice, nothing else); the
      read-out as observe_device minus grape_eval_device, both timed the same way in the same blocks.  These figures decide
      kObsStagedMaxProbes / kVjpStagedMaxProbes in csrc/grape_api.cpp.
  (b) the host forms against the device forms end to end (wall clock, the device forms followed by a synchronise), with the
      library's own choice of instance.
  (c) one autograd step (forward, backward) of a log-barrier loss through autograd.trajectory (CPU tensors) and through
      autograd.trajectory_device (CUDA tensors), with and without the reuse of the stored trajectory.
  (d) grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, --other): fresh
      child processes in turn.  "Did not move" holds only if the difference lies inside the spread between this build's own
      processes; F must be equal bit for bit.

Usage: python tools/traj_device_time.py [--blocks 15] [--calls 40] [--other PATH/libgrape_hip.so] [--out FILE]"""
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
N_OBS_A = (1, 2, 4, 8, 12, 16)                               # section (a): where the staged instances stop winning


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
    from quoptimalcontrol_jl_amd import autograd
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
    cm = qoc.engine._cm
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    xd = dev(w.x.T)
    Od = {j: dev(cm(O[:j])) for j in N_OBS_A}
    ybd = {j: dev(ybar[:, :j]) for j in N_OBS_A}
    yb = {j: np.ascontiguousarray(ybar[:, :j]) for j in N_OBS}
    xbd = dev(cm(xbar))
    yd = {j: torch.empty((E, j, N + 1), dtype=torch.complex128, device="cuda") for j in N_OBS_A}
    Xfd = torch.empty((E, m, n), dtype=torch.complex128, device="cuda")
    fg = torch.empty(K * N + 1, dtype=torch.float64, device="cuda")
    Gd = torch.empty((N, K), dtype=torch.float64, device="cuda")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    say(f"# tools/traj_device_time.py: C3 n={n} m={m} K={K} N={N} E={E}; y / ybar are (E, n_obs, N+1) complex128 = "
        f"{16 * E * (N + 1) / 1e6:.1f} MB per probe; a member's block is {16 * (N + 1)} B per probe")

    def obs(j):
        eng.observe_device(xd.data_ptr(), j, False, Od[j].data_ptr(), yd[j].data_ptr(), Xfd.data_ptr(), fg.data_ptr())

    def vjp(j, reuse):
        eng.observe_vjp_device(0 if reuse else xd.data_ptr(), j, False, Od[j].data_ptr(), ybd[j].data_ptr(), xbd.data_ptr(), Gd.data_ptr())

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
    say(f"# (a) direct against staged instance, HIP events, {a.blocks} alternating blocks of {a.calls} back-to-back calls; us per "
        "call: median of the block means +- half the 10..90 % range between blocks")
    t, names, bits = {}, {}, {}
    for _ in range(a.blocks + 1):                             # (block 0 is the warm-up)
        first = not t
        rec = {}
        os.environ.pop("GRAPE_TRAJ_STAGED", None)
        rec["eval_device"] = gpu_us(lambda: eng.eval_device(xd.data_ptr(), fg.data_ptr()), a.calls)
        for j in N_OBS_A:
            for staged in ("0", "1"):
                os.environ["GRAPE_TRAJ_STAGED"] = staged
                rec[f"obs {j} {staged}"] = gpu_us(lambda: obs(j), a.calls)
                if first:
                    names[f"obs {j} {staged}"] = ";".join(eng.kernel_names())
                    bits[f"obs {j} {staged}"] = yd[j].cpu().numpy().copy()
                vjp(j, False)
                rec[f"vjp {j} {staged}"] = gpu_us(lambda: vjp(j, True), a.calls)
                if first:
                    names[f"vjp {j} {staged}"] = ";".join(eng.kernel_names())
                    bits[f"vjp {j} {staged}"] = Gd.cpu().numpy().copy()
        os.environ.pop("GRAPE_TRAJ_STAGED", None)
        if not first:
            for k, v in rec.items():
                t.setdefault(k, []).append(v)
        else:
            t["eval_device"] = []
    ev, ev_s = stats(t["eval_device"])
    say(f"grape_eval_device                            {ev:8.2f} +- {ev_s:5.2f} us")
    for j in N_OBS_A:
        for kind, label in (("obs", "observe_device"), ("vjp", "vjp_device, reuse")):
            d, d_s = stats(t[f"{kind} {j} 0"])
            s, s_s = stats(t[f"{kind} {j} 1"])
            diff = np.asarray(t[f"{kind} {j} 0"]) - np.asarray(t[f"{kind} {j} 1"])
            g, g_s = stats(diff)
            base = ev if kind == "obs" else 0.0
            same = np.array_equal(bits[f"{kind} {j} 0"], bits[f"{kind} {j} 1"])
            say(f"{label:18s} n_obs={j:<2d} direct {d:8.2f} +- {d_s:5.2f} us   staged {s:8.2f} +- {s_s:5.2f} us   direct - staged "
                f"{g:+8.2f} +- {g_s:5.2f} us (per block)   kernel(s) alone: direct {d - base:7.2f} staged {s - base:7.2f} us   bits equal: {same}")
    for k in ("obs 16 0", "obs 16 1", "vjp 16 0", "vjp 16 1"):
        say(f"  kernels {k}: {names[k]}")

    # ------------------------------------------------------------------------------------------------------------------- (b)
    say("# (b) host forms against device forms end to end (wall clock; device forms + synchronise; the library's own choice of "
        f"instance), {a.blocks} alternating blocks; us per call")

    def wall(fn, calls, sync):
        fn()
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
            if sync:
                torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls

    tb = {}
    for blk in range(a.blocks):
        for j in N_OBS:
            hc = max(2, a.calls // (2 * j))                   # (the host forms move megabytes per call)
            tb.setdefault(f"h_obs {j}", []).append(wall(lambda: eng.observe(w.x, O[:j], final=True), hc, False))
            tb.setdefault(f"d_obs {j}", []).append(wall(lambda: obs(j), a.calls, True))
            tb.setdefault(f"h_vjp {j}", []).append(wall(lambda: eng.observe_vjp(w.x, O[:j], ybar=yb[j], xbar_final=xbar), hc, False))
            tb.setdefault(f"d_vjp {j}", []).append(wall(lambda: vjp(j, False), a.calls, True))
            obs(j)
            tb.setdefault(f"r_vjp {j}", []).append(wall(lambda: vjp(j, True), a.calls, True))
    for j in N_OBS:
        ho, ho_s = stats(tb[f"h_obs {j}"])
        do, do_s = stats(tb[f"d_obs {j}"])
        hv, hv_s = stats(tb[f"h_vjp {j}"])
        dv, dv_s = stats(tb[f"d_vjp {j}"])
        rv, rv_s = stats(tb[f"r_vjp {j}"])
        say(f"n_obs={j:<2d} read-out: host {ho:9.2f} +- {ho_s:6.2f}  device {do:8.2f} +- {do_s:5.2f}   VJP: host {hv:9.2f} +- {hv_s:6.2f}  "
            f"device {dv:8.2f} +- {dv_s:5.2f}  device, reuse {rv:8.2f} +- {rv_s:5.2f}   step (read-out + VJP): host {ho + hv:9.2f}  "
            f"device {do + dv:8.2f}  device with reuse {do + rv:8.2f}")
    y_h, X_h = eng.observe(w.x, O[:4], final=True)
    obs(4)
    torch.cuda.synchronize()
    G_h = eng.observe_vjp(w.x, O[:4], ybar=yb[4], xbar_final=xbar)
    vjp(4, False)
    torch.cuda.synchronize()
    say(f"  device = host, bit for bit (n_obs = 4): y {np.array_equal(yd[4].cpu().numpy(), y_h)}, "
        f"X_final {np.array_equal(np.swapaxes(Xfd.cpu().numpy(), -1, -2), X_h)}, G {np.array_equal(Gd.cpu().numpy().T, G_h)}")

    # ------------------------------------------------------------------------------------------------------------------- (c)
    say("# (c) one autograd step (forward + backward) of l = -mean log(1 - |y|^2 / 256); wall clock with a final synchronise; us per step")

    def step(x, j, device, reuse=True):
        x.grad = None
        if device:
            y = autograd.trajectory_device(eng, x, opsd[j], final=False, reuse=reuse)
        else:
            y = autograd.trajectory(eng, x, O[:j], final=False)
        (-torch.log1p(-y.abs() ** 2 / 256.0).mean()).backward()   # (|y|^2 <= |O|^2 |X|^2 < 256 for these probes)
        return x.grad

    opsd = {j: dev(O[:j]) for j in N_OBS}
    xc = torch.tensor(w.x, dtype=torch.float64, requires_grad=True)
    xg = torch.tensor(w.x, dtype=torch.float64, device="cuda", requires_grad=True)
    tc = {}
    for blk in range(max(3, a.blocks // 3)):
        for j in N_OBS:
            tc.setdefault(f"cpu {j}", []).append(wall(lambda: step(xc, j, False), 2, False))
            tc.setdefault(f"gpu {j}", []).append(wall(lambda: step(xg, j, True, False), a.calls // 2, True))
            tc.setdefault(f"gpu_reuse {j}", []).append(wall(lambda: step(xg, j, True, True), a.calls // 2, True))
    for j in N_OBS:
        c_, c_s = stats(tc[f"cpu {j}"])
        g_, g_s = stats(tc[f"gpu {j}"])
        r_, r_s = stats(tc[f"gpu_reuse {j}"])
        gc = step(xc, j, False).numpy().copy()
        gg = step(xg, j, True).cpu().numpy()
        say(f"n_obs={j:<2d} trajectory (CPU tensors) {c_:10.2f} +- {c_s:7.2f}   trajectory_device {g_:8.2f} +- {g_s:5.2f}   with reuse "
            f"{r_:8.2f} +- {r_s:5.2f}   |dG|_inf / |G|_inf between the two = {np.abs(gg - gc).max() / np.abs(gc).max():.1e}")
    eng.close()

    # ------------------------------------------------------------------------------------------------------------------- (d)
    if a.other:
        say(f"# (d) grape_eval, fresh processes in turn, 21 blocks of 300 calls each: this build / the other build")
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
