"""What the fused Gauss-Newton product along the trajectory (grape_eval_gnvp / grape_eval_gnvp_device) costs on the headline
config -- C3: 4 x 4 UnitaryGate, K = 4, N = 500, E = 1024 -- for n_obs = 1, 4 and 16 shared probes, in ONE process and ONE
context, in alternating blocks after a warm-up block; per variant the median over the blocks of the block means and the
spread between blocks (half the 10 % .. 90 % range):

  (a) the kernels' own time from HIP events (torch.cuda.Event around a block of back-to-back reuse calls on one stream, d_x =
      NULL: no sweep, no pulse map), the direct instances (GRAPE_TRAJ_STAGED=0):
        trajectory_gnvp_kernel + vjp_sum_kernel                     gnvp_device
        the work it fuses, launched in the same blocks:             one jvp_device (trajectory_jvp_kernel) and one vjp_device
                                                                    (trajectory_vjp_kernel + vjp_sum_kernel)
  (b) one CG iteration of a Gauss-Newton step at one linearisation point, HIP events: gnvp_device(NULL) with shared block
      weights, against jvp_device(NULL), the weights applied by a torch multiply on the GPU, vjp_device(NULL)
      -- and the device bytes the fused path does not allocate (ydot, ybar, and per-member copies of shared weights).
  (c) grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, --other): fresh
      child processes in turn.  "Did not move" holds only if the difference lies inside the spread between this build's own
      processes; F must be equal bit for bit.

Usage: python tools/gnvp_time.py [--blocks 15] [--calls 40] [--other PATH/libgrape_hip.so] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

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
    xdot = rng.standard_normal((K, N))
    la, lb, lc = rng.uniform(0.3, 1.2, (16, N + 1)), rng.standard_normal((16, N + 1)), rng.uniform(0.3, 1.2, (16, N + 1))
    planes = np.stack([la * la, la * lb, lb * lb + lc * lc])      # shared positive definite blocks, (3, 16, N+1)
    wf = rng.uniform(0.2, 1.5, E)
    cm = qoc.engine._cm
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    xd, xdd, wfd = dev(w.x.T), dev(xdot.T), dev(wf)
    Od = {j: dev(cm(O[:j])) for j in N_OBS}
    wd = {j: dev(planes[:, :j]) for j in N_OBS}
    yd = {j: torch.empty((E, j, N + 1), dtype=torch.complex128, device="cuda") for j in N_OBS}
    ydd = {j: torch.empty((E, j, N + 1), dtype=torch.complex128, device="cuda") for j in N_OBS}
    ybd = {j: torch.empty((E, j, N + 1), dtype=torch.complex128, device="cuda") for j in N_OBS}
    Xfd = torch.empty((E, m, n), dtype=torch.complex128, device="cuda")
    Xdd = torch.empty((E, m, n), dtype=torch.complex128, device="cuda")
    Xbd = torch.empty((E, m, n), dtype=torch.complex128, device="cuda")
    fg = torch.empty(K * N + 1, dtype=torch.float64, device="cuda")
    Gd = torch.empty((N, K), dtype=torch.float64, device="cuda")
    os.environ["GRAPE_TRAJ_STAGED"] = "0"                      # the direct instances throughout: like against like
    eng = qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=0)
    say(f"# tools/gnvp_time.py: C3 n={n} m={m} K={K} N={N} E={E}; ydot / ybar are (E, n_obs, N+1) complex128 = "
        f"{16 * E * (N + 1) / 1e6:.1f} MB per probe each; direct instances (GRAPE_TRAJ_STAGED=0)")

    def obs(j):
        eng.observe_device(xd.data_ptr(), j, False, Od[j].data_ptr(), yd[j].data_ptr(), Xfd.data_ptr(), fg.data_ptr())

    def vjp(j):
        eng.observe_vjp_device(0, j, False, Od[j].data_ptr(), ybd[j].data_ptr(), Xbd.data_ptr(), Gd.data_ptr())

    def jvp(j):
        eng.observe_jvp_device(0, xdd.data_ptr(), j, False, Od[j].data_ptr(), ydd[j].data_ptr(), Xdd.data_ptr())

    def gnvp(j):
        eng.observe_gnvp_device(0, xdd.data_ptr(), j, False, Od[j].data_ptr(), 0, wd[j].data_ptr(), wfd.data_ptr(), Gd.data_ptr())

    def weigh(j):
        """ybar = W ydot, Xbar = wf Xdot_N with torch on the GPU (what a caller of the composed path does between the calls)"""
        re, im = ydd[j].real, ydd[j].imag
        torch.complex(wd[j][0] * re + wd[j][1] * im, wd[j][1] * re + wd[j][2] * im, out=ybd[j])
        torch.mul(Xdd, wfd[:, None, None], out=Xbd)

    def composed(j):
        jvp(j)
        weigh(j)
        vjp(j)

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

    say(f"# (a), (b) HIP events, {a.blocks} alternating blocks of {a.calls} back-to-back reuse calls (one warm-up block in "
        "front); us per call: median of the block means +- half the 10..90 % range between blocks")
    t, names = {}, {}
    obs(16)
    for j in N_OBS:                                            # (cotangents of the right size for the kernel-only timing of the VJP)
        jvp(j)
        weigh(j)
    for blk in range(a.blocks + 1):
        rec = {}
        for j in N_OBS:
            rec[f"gnvp {j}"] = gpu_us(lambda: gnvp(j), a.calls)
            names[f"gnvp {j}"] = ";".join(eng.kernel_names())
            rec[f"jvp {j}"] = gpu_us(lambda: jvp(j), a.calls)
            rec[f"vjp {j}"] = gpu_us(lambda: vjp(j), a.calls)
            rec[f"cg {j}"] = gpu_us(lambda: composed(j), a.calls)
        if blk:
            for k, v in rec.items():
                t.setdefault(k, []).append(v)
    say("# (a) the kernels")
    for j in N_OBS:
        gn, gn_s = stats(t[f"gnvp {j}"])
        jv, jv_s = stats(t[f"jvp {j}"])
        vj, vj_s = stats(t[f"vjp {j}"])
        pair, pair_s = stats(np.asarray(t[f"jvp {j}"]) + np.asarray(t[f"vjp {j}"]))
        say(f"n_obs={j:<2d} trajectory_gnvp_kernel + vjp_sum_kernel {gn:8.2f} +- {gn_s:5.2f} us   trajectory_jvp_kernel {jv:8.2f} +- {jv_s:5.2f} us   "
            f"trajectory_vjp_kernel + vjp_sum_kernel {vj:8.2f} +- {vj_s:5.2f} us   jvp + vjp (per block) {pair:8.2f} +- {pair_s:5.2f} us   "
            f"gnvp / (jvp + vjp) = {gn / pair:.2f}")
    say(f"  kernels gnvp 16: {names['gnvp 16']}")
    say("# (b) one CG iteration: gnvp_device(NULL) against jvp_device(NULL), the torch multiply, vjp_device(NULL)")
    for j in N_OBS:
        gn, gn_s = stats(t[f"gnvp {j}"])
        cg, cg_s = stats(t[f"cg {j}"])
        ydot_b = 16 * E * j * (N + 1)
        say(f"n_obs={j:<2d} fused {gn:8.2f} +- {gn_s:5.2f} us   composed {cg:8.2f} +- {cg_s:5.2f} us   fused / composed = {gn / cg:.2f}   "
            f"not allocated by the fused path: ydot {ydot_b / 1e6:.1f} MB + ybar {ydot_b / 1e6:.1f} MB "
            f"(+ {(E - 1) * 24 * j * (N + 1) / 1e6:.1f} MB where a caller would repeat the shared weights per member)")
    gnvp(4)
    torch.cuda.synchronize()
    G_f = Gd.cpu().numpy().T.copy()
    composed(4)
    torch.cuda.synchronize()
    G_c = Gd.cpu().numpy().T.copy()
    Gh = eng.observe_gnvp(w.x, xdot, O[:4], w=planes[:, :4], wf=wf)
    say(f"  n_obs = 4: reuse = host bit for bit {np.array_equal(G_f, Gh)}; |fused - composed|_inf / |fused|_inf = "
        f"{np.abs(G_f - G_c).max() / np.abs(G_f).max():.2e}")
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
