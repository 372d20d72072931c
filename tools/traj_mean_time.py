"""What the ensemble-averaged trajectory calls (grape_eval_observables_mean / _vjp_mean / _jvp_mean) cost next to the per-member
host forms they replace, on the headline config -- C3: 4 x 4 UnitaryGate, K = 4, N = 500, E = 1024 -- blocking host->host:

  1. ONE context, alternating blocks behind a warm-up, for 1 / 4 / 16 probes (shared probes, y and the final states):
       observe      against observe_mean        (the per-member form copies (E, n_obs, N+1) complex128 down)
       observe_vjp  against observe_vjp_mean    (the per-member form takes the explicit broadcast cotangents v_k ybar: it scans
                                                 them for non-finite entries and copies them up; building them is NOT timed)
       observe_jvp  against observe_jvp_mean
     and grape_eval itself.  Per call: the median over the blocks of the block means, and the spread between blocks (half the
     10 .. 90 % range).  The pull-back pair must agree bit for bit; that is checked and printed.
  2. one autograd step (forward + backward, CPU tensors) of a log-barrier loss on the averaged populations,
     -sum log(1 + eps - |sum_k w_k y[k, j, s]|^2 / c_j), through autograd.trajectory + a torch sum over the members against
     autograd.trajectory_mean, alternating blocks.
  3. the two new kernels alone, from HIP events: the lines of tools/ubench/traj_mean_rate (built from csrc/traj_mean.hip itself;
     --ubench PATH, default tools/ubench/traj_mean_rate; skipped with a note if the program is not there).
  4. grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, --other): fresh child
     processes in turn, --rounds pairs, the build that goes first alternating from pair to pair.  "Did not move" holds only
     if the difference of the means lies inside the spread between this build's own processes (largest minus smallest); F
     must be equal bit for bit.

Usage: python tools/traj_mean_time.py [--blocks 15] [--calls 20] [--other PATH/libgrape_hip.so] [--rounds 4] [--ubench PATH]
       [--out FILE]"""
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


def explicit(v, cot):
    out = np.empty((len(v),) + cot.shape, complex)
    w = v.reshape((len(v),) + (1,) * cot.ndim)
    out.real = w * cot.real
    out.imag = w * cot.imag
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--other", default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--ubench", default=os.path.join(ROOT, "tools", "ubench", "traj_mean_rate"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, 21, 300)
    out = open(a.out, "w") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    w = qoc.workloads.config("C3")
    m, E, N = w.Xi.shape[2], w.E, w.N
    rng = np.random.default_rng(1)
    O = rng.standard_normal((16, w.n, m)) + 1j * rng.standard_normal((16, w.n, m))
    O[0] = w.Xi[0]
    wts = np.ascontiguousarray(w.wts, dtype=np.float64)
    ybar = rng.standard_normal((16, N + 1)) + 1j * rng.standard_normal((16, N + 1))
    xbar = rng.standard_normal((w.n, m)) + 1j * rng.standard_normal((w.n, m))
    xdot = rng.standard_normal(w.x.shape)
    yb_full = {j: explicit(wts, ybar[:j]) for j in N_OBS}
    xb_full = explicit(wts, xbar)
    say(f"# tools/traj_mean_time.py: C3 n={w.n} m={m} K={w.K} N={N} E={E}; blocking host->host calls; a per-member y block is "
        f"{16 * E * (N + 1) / 1e6:.1f} MB per probe, an averaged one {16 * (N + 1) / 1e3:.1f} KB")
    say(f"# 1. one context, {a.blocks} alternating blocks of {a.calls} calls behind a warm-up; us per call: median of the block "
        "means +- half the 10..90 % range between blocks")
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, N, device=0)
    xf = np.ascontiguousarray(w.x.T)
    G = np.empty_like(xf)
    fns = {"eval": lambda: eng.eval_cm(xf, G)}
    for j in N_OBS:
        fns[f"observe {j}"] = lambda j=j: eng.observe(w.x, O[:j], final=True)
        fns[f"observe_mean {j}"] = lambda j=j: eng.observe_mean(w.x, O[:j], final=True)
        fns[f"observe_vjp {j}"] = lambda j=j: eng.observe_vjp(w.x, O[:j], ybar=yb_full[j], xbar_final=xb_full)
        fns[f"observe_vjp_mean {j}"] = lambda j=j: eng.observe_vjp_mean(w.x, O[:j], ybar_mean=ybar[:j], xbar_mean=xbar)
        fns[f"observe_jvp {j}"] = lambda j=j: eng.observe_jvp(w.x, xdot, O[:j], final=True)
        fns[f"observe_jvp_mean {j}"] = lambda j=j: eng.observe_jvp_mean(w.x, xdot, O[:j], final=True)
    names, t = {}, {k: [] for k in fns}
    for key, fn in fns.items():
        for _ in range(3):
            fn()
        names[key] = ";".join(eng.kernel_names())
    for _ in range(a.blocks):
        for key, fn in fns.items():
            calls = 10 * a.calls if key == "eval" else a.calls
            fn()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t[key].append((time.perf_counter() - t0) / calls)
    ev, ev_s = stats(t["eval"])
    say(f"grape_eval                     {ev:9.2f} +- {ev_s:6.2f} us")
    for base in ("observe", "observe_vjp", "observe_jvp"):
        for j in N_OBS:
            p, p_s = stats(t[f"{base} {j}"])
            q, q_s = stats(t[f"{base}_mean {j}"])
            verdict = "faster" if p - q > max(p_s, q_s) else ("slower" if q - p > max(p_s, q_s) else "within the spread")
            say(f"{base:11s} n_obs={j:<2d}  per member {p:9.2f} +- {p_s:6.2f} us   mean form {q:9.2f} +- {q_s:6.2f} us   "
                f"mean / per member = {q / p:.3f} ({verdict})   mean form above grape_eval by {q - ev:.2f} us")
    for key in ("observe_mean 4", "observe_vjp_mean 4", "observe_jvp_mean 4"):
        say(f"  kernels {key}: {names[key]}")
    same = all(np.array_equal(eng.observe_vjp(w.x, O[:j], ybar=yb_full[j], xbar_final=xb_full),
                              eng.observe_vjp_mean(w.x, O[:j], ybar_mean=ybar[:j], xbar_mean=xbar)) for j in N_OBS)
    y4, ym4 = eng.observe(w.x, O[:4]), eng.observe_mean(w.x, O[:4])
    dev = np.abs(ym4 - np.tensordot(wts, y4, 1)).max()
    say(f"  observe_vjp_mean = observe_vjp on the explicit cotangents, bit for bit, at 1 / 4 / 16 probes: {same}; "
        f"|observe_mean - NumPy's weighted sum of observe|_inf = {dev:.2e}")

    say(f"# 2. one autograd step (forward + backward, CPU tensors) of a log-barrier loss on the averaged populations, "
        f"{a.blocks} alternating blocks of {max(1, a.calls // 4)} steps")
    import torch
    from quoptimalcontrol_jl_amd import autograd
    wt = torch.tensor(wts)
    scale = {j: torch.tensor(np.sum(np.abs(O[:j]) ** 2, axis=(1, 2)) * m * wts.sum() ** 2)[:, None] for j in N_OBS}

    def step(j, mean):
        x = torch.tensor(w.x, dtype=torch.float64, requires_grad=True)
        if mean:
            ym = autograd.trajectory_mean(eng, x, O[:j], final=False)
        else:
            y = autograd.trajectory(eng, x, O[:j], final=False)
            ym = torch.einsum("k,kjs->js", wt.to(y.dtype), y)
        loss = -torch.log(1.0 + 1e-3 - ym.abs() ** 2 / scale[j]).sum()      # (|y_mean|^2 <= scale: Cauchy-Schwarz)
        loss.backward()
        return loss.item(), x.grad.numpy()

    ts = {(j, mean): [] for j in N_OBS for mean in (False, True)}
    steps = max(1, a.calls // 4)
    for blk in range(a.blocks + 1):
        for key in ts:
            t0 = time.perf_counter()
            for _ in range(steps):
                res = step(*key)
            if blk:
                ts[key].append((time.perf_counter() - t0) / steps)
    for j in N_OBS:
        p, p_s = stats(ts[j, False])
        q, q_s = stats(ts[j, True])
        (l0, g0), (l1, g1) = step(j, False), step(j, True)
        say(f"autograd step n_obs={j:<2d}  trajectory + torch sum {p:9.2f} +- {p_s:6.2f} us   trajectory_mean {q:9.2f} +- {q_s:6.2f} us   "
            f"ratio {q / p:.3f}   |loss difference| = {abs(l0 - l1):.1e}, |grad difference|_inf / |grad|_inf = "
            f"{np.abs(g0 - g1).max() / np.abs(g0).max():.1e}")
    eng.close()

    say("# 3. the two new kernels alone (HIP events)")
    if os.path.exists(a.ubench):
        p = subprocess.run([a.ubench, "15", "50"], capture_output=True, text=True, timeout=300)
        for line in (p.stdout if p.returncode == 0 else f"traj_mean_rate failed: {p.stderr[-500:]}").splitlines():
            say(line)
    else:
        say(f"not measured: {a.ubench} is not built (hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-fast-math -ffp-contract=on "
            "tools/ubench/traj_mean_rate.hip -o tools/ubench/traj_mean_rate)")

    if a.other:
        say(f"# 4. grape_eval, fresh processes in turn, 21 blocks of 300 calls each, {a.rounds} pairs, the first build of a pair alternating")
        res = {"this": [], "other": []}
        for rnd in range(a.rounds):
            pair = (("this", qoc.library_path()), ("other", a.other))
            for key, path in (pair if rnd % 2 == 0 else pair[::-1]):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], capture_output=True, text=True,
                                   timeout=300)
                if p.returncode:
                    say(f"{key}: child failed: {p.stderr[-500:]}")
                    continue
                d = json.loads(p.stdout.strip().splitlines()[-1])
                res[key].append(d)
                say(f"{key:5s} build, pair {rnd + 1}: grape_eval {d['us']:.2f} +- {d['spread']:.2f} us   F = {d['F']!r}   ABI {d['abi']}")
        if len(res["this"]) >= 2 and res["other"]:
            ta, tb = [d["us"] for d in res["this"]], [d["us"] for d in res["other"]]
            a_, b_ = np.mean(ta), np.mean(tb)
            own, theirs = max(ta) - min(ta), max(tb) - min(tb)
            sp = max(d["spread"] for d in res["this"] + res["other"])
            Fs = {d["F"] for d in res["this"] + res["other"]}
            say(f"this build {a_:.2f} us, other build {b_:.2f} us: difference of the means {a_ - b_:+.2f} us; this build's own "
                f"processes span {own:.2f} us, the other build's {theirs:.2f} us, block-to-block spread <= {sp:.2f} us; F equal in "
                f"every process: {len(Fs) == 1}; inside this build's own spread: {abs(a_ - b_) <= own}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
