"""What several cotangent sets per trajectory call (grape_eval_vjp_multi_device) cost next to the single call's kernels, per
set -- the data behind the dispatch table vjp_multi_default (csrc/grape_kernels.hpp).

  (a) In ONE process and ONE context per (shape, flow), HIP events around blocks of back-to-back reuse calls (d_x = NULL: the
      pull-back alone, no sweep, no pulse map), in alternating blocks behind a warm-up block, for n_set = 1, 2, 4, 8, in the
      first-order mode (the exact mode runs the single call's kernels per set on either side):
        multi    GRAPE_VJP_MULTI=1: trajectory_vjp_multi_kernel in blocks of vjp_multi_block(n, m) sets + vjp_sum_kernel
        single   GRAPE_VJP_MULTI=0: n_set launches of trajectory_vjp_kernel (the staged instance where the device form
                 chooses it) + vjp_sum_kernel behind each other (the same bits)
      Per variant the median over the blocks of the block means +- half the 10 .. 90 % range between blocks, per call and per
      set, and the ratio.  Shapes: the headline config C3 (4 x 4, K = 4, N = 500, E = 1024) at 1 / 4 / 16 probes, and one
      further shape per n at 4 probes -- (n, m) = (2, 2), (3, 3), (4, 1), random Hermitian generators, K = 2, N = 500,
      E = 1024 -- each in the unitary flow and (FLAG_FORCE_GENERAL) in the general flow, which stores the states.
      A shape keeps the multi instance by default only if its per-set time at n_set = 4 lies below the single kernels' by more
      than the spread between blocks (the larger of the two spreads) at 4 probes, in both flows; a lone set (n_set = 1) goes
      to the multi kernel only under the same rule.
  (b) grape_eval of THIS build against another build of the library (the parent commit's libgrape_hip.so, --other): fresh
      child processes in turn (SweepParams grew).  "Did not move" holds only if the difference of the means lies inside the
      spread; F must be equal bit for bit.

Usage: python tools/vjp_multi_time.py [--blocks 15] [--calls 20] [--other PATH/libgrape_hip.so] [--out FILE]"""
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
from jvp_multi_time import headline, random_shape  # noqa: E402

N_SET = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
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

    def gpu_s(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e-3 * e0.elapsed_time(e1) / calls              # seconds per call (stats() reports us)

    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    say(f"# tools/vjp_multi_time.py: reuse calls (d_x = NULL), HIP events, {a.blocks} alternating blocks of {a.calls} calls behind "
        "a warm-up block; us: median of the block means +- half the 10..90 % range between blocks")
    verdict = {}
    for shape, probes in ((headline(), (1, 4, 16)), (random_shape(2, 2), (4,)), (random_shape(3, 3), (4,)), (random_shape(4, 1), (4,))):
        n, m, K, N, E = (shape[k] for k in ("n", "m", "K", "N", "E"))
        rng = np.random.default_rng(1)
        O = rng.standard_normal((16, n, m)) + 1j * rng.standard_normal((16, n, m))
        xd = dev(shape["x"].T)
        xb = dev(rng.standard_normal((8, E, m, n)) + 1j * rng.standard_normal((8, E, m, n)))
        for flow, flags in (("unitary", 0), ("general", qoc.engine.FLAG_FORCE_GENERAL)):
            eng = qoc.GrapeEngine("UnitaryGate", shape["A"], shape["B"], shape["Xi"], shape["Xt"], shape["wts"], shape["T"], N,
                                  device=0, flags=flags)
            info = eng.info
            say(f"## {shape['name']}, {flow} flow (unitary_flow={info['unitary_flow']}): n={n} m={m} K={K} N={N} E={E}, "
                f"slices_per_lane={info['slices_per_lane']} waves_per_member={info['waves_per_member']} "
                f"lane_pair={info['lane_pair']}; propagators {16 * n * n * N * E / 1e6:.0f} MB")
            for j in probes:
                Od = dev(qoc.engine._cm(O[:j]))
                yb = dev(rng.standard_normal((8, E, j, N + 1)) + 1j * rng.standard_normal((8, E, j, N + 1)))
                G = torch.empty((8, N, K), dtype=torch.float64, device="cuda")

                def call(ns, x=0):
                    eng._check(eng._lib.grape_eval_vjp_multi_device(eng._h, x, ns, j, 0, Od.data_ptr(), yb.data_ptr(), xb.data_ptr(),
                                                                    G.data_ptr(), 0))

                os.environ["GRAPE_VJP_MULTI"] = "1"
                call(8, xd.data_ptr())                         # the trajectory every reuse call below runs along
                torch.cuda.synchronize()
                ref = G.cpu().numpy().copy()
                t, names = {}, {}
                for blk in range(a.blocks + 1):
                    for ns in N_SET:
                        for key, env in (("multi", "1"), ("single", "0")):
                            os.environ["GRAPE_VJP_MULTI"] = env
                            rec = gpu_s(lambda: call(ns), a.calls)
                            names[key, ns] = eng.kernel_names()
                            if blk:
                                t.setdefault((key, ns), []).append(rec)
                os.environ["GRAPE_VJP_MULTI"] = "0"
                call(8)
                torch.cuda.synchronize()
                same = np.array_equal(G.cpu().numpy(), ref)
                for ns in N_SET:
                    mu, mu_s = stats(t["multi", ns])
                    si, si_s = stats(t["single", ns])
                    say(f"{shape['name']:11s} {flow:7s} n_obs={j:<2d} n_set={ns}: multi {mu:8.2f} +- {mu_s:5.2f} us "
                        f"({mu / ns:7.2f} per set)   single x {ns} {si:8.2f} +- {si_s:5.2f} us ({si / ns:7.2f} per set)   "
                        f"multi / single = {mu / si:.3f}")
                    if ns in (1, 4) and j == 4:
                        verdict[shape["name"], n, m, flow, ns] = (mu / ns, si / ns, max(mu_s, si_s) / ns,
                                                                  (si - mu) / ns > max(mu_s, si_s) / ns)
                say(f"  kernels at n_set = 8: multi {';'.join(names['multi', 8])} | single {';'.join(names['single', 8])}; "
                    f"multi = single bit for bit: {same}")
            eng.close()
    os.environ.pop("GRAPE_VJP_MULTI", None)
    say("# dispatch: per-set us at n_set = 4 and at a lone set, 4 probes; keep = the multi kernel is faster by more than the spread")
    for (name, n, m, flow, ns), (mu, si, sp, keep) in verdict.items():
        say(f"{name:11s} <{n},{m}> {flow:7s} n_set={ns}: multi {mu:7.2f}  single {si:7.2f}  spread {sp:5.2f}  -> "
            f"{'keep multi' if keep else 'single kernel'}")

    if a.other:
        say("# (b) grape_eval, fresh processes in turn, 21 blocks of 300 calls each: this build / the other build")
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
