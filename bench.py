#!/usr/bin/env python3
"""bench.py -- GRAPE gradient-evals/sec on the headline config (BASELINE.json):
2-qubit UnitaryGate, 4x4, 4 controls, 500 slices, 1024-member ensemble (SURVEY.md 8d "C3").

One step = one call of the reference's ensemble closure topt(F, G, x) (src/solve.jl:164-196) exactly
as the Julia glue makes it: grape_eval(ctx, x_host, &F, G_host) -- x in host memory -> all member
evaluations + the weighted reduction -> F, G back in host memory, blocking (SURVEY.md 8d,
BASELINE.md section 2).  An L-BFGS can run nothing faster than this, because x_{k+1} depends on G_k.
N > 1 GPUs: one process per GPU, the ensemble is sharded in contiguous member blocks and every
step ends in ONE all-reduce of K*N+1 doubles, issued inside libgrape_hip.so (RCCL, grape_comm_attach);
every rank makes the same host -> host call.

  python bench.py --gpus 1 --steps 300 --warmup 30
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
         --master-port 29500 bench.py --gpus 8 --steps 300 --warmup 30
  python bench.py --gpus 8         # no torchrun around it: spawns the 8 ranks itself (fresh children)

Timing: W warm-up steps, a >= 0.35 s clock ramp, a barrier + torch.cuda.synchronize() and 8 settling steps (all
untimed), then EXACTLY K timed steps (--steps), cut by the host clock into --blocks (default 3) blocks of near-equal
size, and a barrier after the last; per block the MAX over ranks; `ms_per_step` and `value` come from the MEDIAN
block's time per step (so one slow stretch does not set the figure); all block times are in the line.
--dump-outputs DIR writes F and G of the last timed step to DIR/F.npy and DIR/G.npy (float64); the inputs are
seeded, so two builds can be compared output for output.

Prints ONE JSON line on rank 0 (contract: see the task statement), including
  roofline      dominant kernel (sweep) against the 8 TB/s HBM peak with the ALGORITHMIC bytes of
                BASELINE.md's model S; duration from HIP events recorded around every sweep launch
                inside the timed region (on the launch stream; every 8th launch carries the event pair,
                GRAPE_FLAG_TIME_SAMPLED, because a pair costs ~5 us of the ~90 us call).  Also: the bytes/flops of the data
                flow actually run (`flow`), the FP64 fraction, and the end-to-end fraction
                (model S x value / peak, BASELINE.md section 2 formula).
A plain run stops there.  --full also measures what takes runs of its own:
  box           the clock the sweep kernel ran at (a stamped context right after the timed blocks);
  cpu_baseline  the C oracle (a port of the reference's serial algorithm) timed on this
                host on a bounded member sample, + `parity` of those members, rank 0 / N = 1 only;
  extra         the device-resident pipelined loop (grape_eval_device back to back, what round 1
                reported) for comparison, L-BFGS rates, shard overheads and the scaling forecast;
                N > 1: the weak-scaling and mailbox-exchange companions;
  extra_configs C2, C4 (E=1024), C5 (E=4096) host->host value + roofline on one GPU (N = 1 only).
"""
import argparse
import math
import json
import os
import statistics
import subprocess
import sys
import time

# the CPU baseline's OpenMP workers must not spin after their parallel region: the latency-bound lines that follow
# (L-BFGS iterations per second, single problems) poll a host flag and were seen 3x slower next to spinning threads
os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_PEAK_TFLOPS = 78.6    # MI355X FP64 vector = matrix spec; 72 measured (tools/ubench)


def cpu_baseline(workload, seconds, sample_members):
    """Time the oracle (kind 'port', 1 core) on `sample_members` members of the same workload
    and scale to whole-ensemble evaluations per second."""
    from oracle import grape_oracle

    w = workload.members(0, min(sample_members, workload.E))
    args = (w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.x, w.T)
    grape_oracle.ensemble_eval(*args)                      # warm (page in, build)
    n, t0 = 0, time.perf_counter()
    while True:
        F, G, foms, grads = grape_oracle.ensemble_eval(*args, per_member=True)
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds:
            break
    member_evals_per_s = n * w.E / el
    # B2 of BASELINE.md: the same port with OpenMP over members on every host core (bounded, ~1/3 of the time)
    try:
        cores = len(os.sched_getaffinity(0))          # cores this process may actually use
    except AttributeError:
        cores = os.cpu_count() or 1
    try:                                              # a cgroup CPU quota caps what affinity shows
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            cores = min(cores, max(1, int(-(-int(q) // int(per)))))
    except Exception:
        pass
    cores = max(1, min(cores, 64))
    wide = workload.members(0, min(max(sample_members, 16 * cores), workload.E))
    wargs = (wide.sys_type, wide.A, wide.B, wide.Xi, wide.Xt, wide.wts, wide.x, wide.T)
    grape_oracle.ensemble_eval(*wargs, n_threads=cores)
    n2, t1 = 0, time.perf_counter()
    while True:
        grape_oracle.ensemble_eval(*wargs, n_threads=cores)
        n2 += 1
        el2 = time.perf_counter() - t1
        if el2 >= seconds / 3:
            break
    return {
        "value": member_evals_per_s / workload.E, "unit": "gradient-evals/s", "cores": 1, "kind": "port",
        "sample": f"{n} x {w.E} of {workload.E} members, {el:.1f} s of oracle/grape_oracle.c (serial, like the "
                  f"reference's member loop); scaled by members",
        "member_evals_per_s": member_evals_per_s,
        "all_cores": {"value": n2 * wide.E / el2 / workload.E, "cores": cores,
                      "sample": f"{n2} x {wide.E} members, OpenMP over members"},
    }, (foms, grads)


def _stats_us(ms):
    import numpy as np
    a = np.asarray(ms, dtype=float) * 1e3
    if a.size == 0:
        return {"kernel_avg_us": 0.0, "kernel_min_us": 0.0, "kernel_median_us": 0.0, "kernel_max_us": 0.0, "kernel_launches": 0}
    return {"kernel_avg_us": float(a.mean()), "kernel_min_us": float(a.min()), "kernel_median_us": float(np.median(a)),
            "kernel_max_us": float(a.max()), "kernel_launches": int(a.size)}


_ACT_TOL = 3.7e-16
_ACT_THETA = [(_ACT_TOL * math.factorial(m + 1)) ** (1.0 / (m + 1)) for m in range(1, 25)]


def action_steps(local):
    """Horner steps (matrix-vector products per chain) action_thin_kernel takes over all members and slices: the degree
    table of csrc/action_thin.hip on  max(|A'_k|_1, |A'_k|_inf) + max over the step's two slices of the same bound of
    Gc_t  (one wave runs the forward slice i and the backward slice N-1-i together)."""
    import numpy as np
    dt = local.T / local.N

    def bound(M):
        a = np.abs(M.real) + np.abs(M.imag)
        return np.maximum(a.sum(-2).max(-1), a.sum(-1).max(-1))
    an = dt * bound(local.A)                                             # (E,)
    Gc = dt * np.einsum("ct,cij->tij", local.x, local.B[0])              # (N, n, n): the controls are member-invariant
    gn = bound(Gc)
    gn = np.maximum(gn, gn[::-1])
    th = an[:, None] + gn[None, :]
    pieces = np.where(th > 1.40513, np.ceil(th / 1.40513), 1.0)
    deg = 1 + np.searchsorted(np.asarray(_ACT_THETA), th / pieces, side="left")
    return float((np.minimum(deg, 24) * pieces).sum())


def _hermitian(M):
    import numpy as np
    M = np.asarray(M)
    return M.shape[-1] == M.shape[-2] and bool(np.allclose(M, np.conj(np.swapaxes(M, -1, -2)), rtol=0.0, atol=1e-13))


def tile_kernel_models(local, info, names=()):
    """Work of the two halves of a tile-family (n = 5..32) evaluation AS RUN: matrix-core flops
    = v_mfma_f64_16x16x4 instructions x 2048 (a complex tile product is 12 of them: three real products), HBM bytes =
    the padded D-layout dumps each kernel writes / reads.  Squarings (data dependent, none at the BASELINE configs with
    theta8 = 0.08) are not counted."""
    n, K, N, E = local.n, local.K, local.N, local.E
    NT = (n + 15) // 16                                    # (NT = 3, 4: sweep_grid.hip, n = 33..64)
    units = (E + 1) // 2 if n <= 8 else E                  # n <= 8: two members share a tile
    tsz = (16 * NT) ** 2 * 16                              # bytes of one matrix dump
    prod = 12 * NT ** 3 * 2048                             # flops of one complex tile-matrix product
    thin, fused, uni = bool(info.get("rank_one_chain")), bool(info.get("fused_forward")), bool(info.get("unitary_flow"))
    sand = local.sys_type != "UnitaryGate"
    if info.get("expm_action"):
        # rank-one states, shared controls: exp(G_t) applied to the two chains' vectors (csrc/action_thin.hip).  Vector FP64
        # flops = Horner steps x 256 complex multiply-adds x 8, the steps from the kernel's own rule (degree table on the
        # norm bound, replicated in action_steps); HBM bytes = the vector records written, then read by the forms kernel
        steps = action_steps(local)
        act = {"name": "vector chains (exp(G) v by Taylor series, both chains; vector FP64)",
               "flops": steps * 2 * 256 * 8, "bytes": 2 * units * (N + 1) * 256, "pipe": "valu_fp64",
               "taylor_steps_per_slice": steps / (units * N)}
        forms = {"name": "forms (bilinear forms w' B_c v, one lane per slice)",
                 "flops": units * N * K * (256 + 16) * 8, "bytes": 2 * units * (N + 1) * 256 + units * K * N * 8,
                 "pipe": "valu_fp64"}
        return act, forms
    expm = {"name": "expm (Taylor-8 on the matrix cores)",
            "flops": units * N * 3 * prod, "bytes": units * N * tsz + (units * (N + 1) * 256 if fused else 0)}
    if thin and info.get("prop_chain"):
        # csrc/action_thin.hip: P_t and P_t^T written by the expm kernel, each read once by its vector chain (one DPP
        # matrix-vector product per slice and chain), the records written and read back by the forms kernel; on a chunked
        # time axis (small ensembles) the chunk products read P_t once more and cost one matrix product per slice
        C = int(info.get("time_chunks") or 0)
        expm["bytes"] = 2 * units * N * tsz
        chain = {"name": "propagator chain" + (" on a chunked time axis" if C > 1 else "") + " + forms (vector FP64)",
                 "flops": units * N * (2 * 8 * 256 + K * 8 * (256 + 16)) + (units * N * prod if C > 1 else 0),
                 "bytes": units * N * tsz * (3 if C > 1 else 2) + 4 * units * (N + 1) * 256 + units * K * N * 8, "pipe": "valu_fp64"}
    elif thin:
        chain = {"name": "matrix-vector chain" + (", backward pass only" if fused else ", both passes"),
                 "flops": units * N * ((1 if fused else 2) * 8 * 256 + K * 14 * 256),
                 "bytes": units * N * tsz * (1 if fused else 2) + units * (N + 1) * 256 * (1 if fused else 2)}
    elif uni:
        chain = {"name": "unitary chain (M_t = P' M P, forward product P^T V)", "flops": units * N * 3 * prod,
                 "bytes": units * N * tsz * 2}
    else:
        # general flow.  Hermitian states + Hermitian control operators under the sandwich: Im tr(B [X, L]) = 2 Im tr(B X L),
        # five products per slice instead of six (every general-flow chain kernel); chain_tile_split_kernel (n <= 16) also
        # stores Hermitian states in 3/4 of their slot and, with member-invariant controls, forms the propagators itself --
        # no expm kernel: P_t written once, read once
        herm = sand and _hermitian(local.Xi) and _hermitian(local.Xt)
        q = (5 if herm and _hermitian(local.B) else 6) if sand else 3
        split = any(k.startswith("chain_tile_split_kernel") for k in names)
        state_b = 2 * (0.75 if (split and herm) else 1.0)
        chain = {"name": "dense chain (general flow: states stored)", "flops": units * N * q * prod,
                 "bytes": units * N * tsz * (2 + state_b)}
        if split and not any(k.startswith(("prop_", "grid_prop")) for k in names):
            chain = {"name": "two-wave chain forming its own propagators (general flow)",
                     "flops": units * N * (3 + q) * prod, "bytes": units * N * tsz * (2 + state_b)}
            return None, chain
    return expm, chain


def split_kernels(names):
    """The library's launch list (grape_get_kernel_names) cut where the middle HIP event sits: behind the expm kernel of the
    n = 5..32 family, or behind the vector chains of the propagator-free flow (the pre-pass launches in front of them
    belong to the first part, the reductions to the second)."""
    for prefixes in (("prop_", "grid_prop"), ("action_parts", "action_thin")):
        for i, k in enumerate(names):
            if k.startswith(prefixes):
                return names[:i + 1], names[i + 1:]
    return [], names


def roofline(local, info, samples, evals_per_s, n_gpus, traffic, profile=None, names=()):
    """The dominant kernel of one shard (`local` = the members this rank owns) against its roof.
    samples = (total_ms[], first_ms[]) of the evaluations inside the timed region (HIP events on the launch stream)."""
    import numpy as np
    tot_ms, first_ms = (np.asarray(a, dtype=float) for a in samples)
    st = _stats_us(tot_ms)
    sec = st["kernel_avg_us"] * 1e-6
    uni = bool(info.get("unitary_flow"))
    thin = bool(info.get("rank_one_chain"))
    alg_bytes, alg_flops = local.algorithmic_bytes, local.algorithmic_flops
    fused = bool(info.get("fused_forward"))
    chunks = int(info.get("time_chunks") or 0)
    if info.get("kernel_family") == 2 and local.n >= 17:
        # size-generic kernel on the matrix cores (sweep_any.hip, n > 64): products of 4 real MFMA products per complex one on
        # matrices padded to multiples of 16; per slice 3 (Taylor-8) + s squarings + 3 / 6 chain products, s from the kernel's
        # own rule on the 1-norm bound of G_t (replicated here on a sample of members)
        n, K, N, E = local.n, local.K, local.N, local.E
        nt = (n + 15) // 16
        prod = 4 * nt * nt * (4 * nt) * 2048
        dt = local.T / N
        sq = []
        for k in sorted(set(int(round(i * (E - 1) / 3)) for i in range(4))):
            H = local.A[k][None] + np.tensordot(local.x.T, local.B[k], 1)           # (N, n, n)
            nb = dt * (np.abs(H.real) + np.abs(H.imag)).sum(axis=1).max(axis=1)
            sq.append(np.where(nb > 0.08, np.ceil(np.log2(np.maximum(nb, 1e-300) / 0.08)), 0.0).mean())
        s_mean = float(np.mean(sq))
        q = 3 if local.sys_type == "UnitaryGate" else 6
        t_first = float(first_ms.mean()) * 1e-3 if first_ms.size else 0.0
        parts = []
        for nm, fl, t in (("propagators (any_prop_kernel)", E * N * (3 + s_mean) * prod, t_first),
                          ("chain (chunk products, boundary scan, windowed any_sweep_kernel)", E * N * q * prod, max(sec - t_first, 0.0))):
            if t <= 0:
                continue
            tf = fl / t / 1e12
            parts.append({"kernel": nm, "what": nm, "avg_us": 1e6 * t, "mfma_flops_per_launch": fl, "hbm_bytes_per_launch": 0.0,
                          "achieved_TFLOPs": tf, "achieved_GBs": 0.0, "frac_mfma": tf / FP64_PEAK_TFLOPS, "frac_hbm": 0.0, "bound": "mfma"})
        fl_all = E * N * (3 + s_mean + q) * prod
        tf_all = fl_all / sec / 1e12 if sec > 0 else 0.0
        roof = {"bound": "mfma", "achieved": tf_all, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf_all / FP64_PEAK_TFLOPS,
                "traffic": traffic, "kernel": ";".join(names), "kernels": parts, "squarings_per_slice": s_mean,
                "model_s_equivalent": {"flops_per_launch": alg_flops, "TFLOPs": alg_flops / sec / 1e12 if sec > 0 else 0.0,
                                       "frac_fp64": alg_flops / sec / 1e12 / FP64_PEAK_TFLOPS if sec > 0 else 0.0,
                                       "end_to_end_frac": alg_flops * evals_per_s / 1e12 / FP64_PEAK_TFLOPS},
                "note": "matrix-core flops ISSUED (four real products per complex one, padded tiles) / HIP-event time / 78.6 TF; the "
                        "chain runs on E compute units only (one workgroup per member, sequential in time)"}
    elif info.get("kernel_family") == 1:            # n > 4: FP64 matrix-core kernels
        # priced PER KERNEL on the flow actually run (the rank-one / unitary / chunked flows do less work than model S,
        # so model-S flops over their run time can exceed the peak: kept below as model_s_equivalent only)
        expm, chain = tile_kernel_models(local, info, names)
        t_first = float(first_ms.mean()) * 1e-3 if first_ms.size else 0.0
        parts = []
        k_first, k_rest = split_kernels(list(names))
        for part, t, launched in ((expm, t_first, k_first), (chain, max(sec - t_first, 0.0), k_rest)):
            if part is None:                                   # (the chain forms the propagators: one part, the whole launch list)
                continue
            tf = part["flops"] / t / 1e12 if t > 0 else 0.0
            gb = part["bytes"] / t / 1e9 if t > 0 else 0.0
            fm, fh = tf / FP64_PEAK_TFLOPS, gb / HBM_PEAK_GBS
            pipe = part.get("pipe", "mfma")                   # "valu_fp64": vector FP64 (same 78.6 TFLOP/s peak as the matrix pipe)
            d = {"kernel": ";".join(launched) or part["name"], "what": part["name"], "avg_us": 1e6 * t,
                 pipe + "_flops_per_launch": part["flops"],
                 "hbm_bytes_per_launch": part["bytes"], "achieved_TFLOPs": tf, "achieved_GBs": gb,
                 "frac_" + pipe: fm, "frac_hbm": fh, "bound": pipe if fm >= fh else "hbm"}
            if "taylor_steps_per_slice" in part:
                d["taylor_steps_per_slice"] = part["taylor_steps_per_slice"]
            parts.append(d)
        dom = max(parts, key=lambda d: d["avg_us"])
        mf = dom["bound"] != "hbm"
        roof = {"bound": dom["bound"], "achieved": dom["achieved_TFLOPs"] if mf else dom["achieved_GBs"],
                "peak": FP64_PEAK_TFLOPS if mf else HBM_PEAK_GBS, "unit": "TFLOP/s" if mf else "GB/s",
                "frac": dom.get("frac_mfma", dom.get("frac_valu_fp64")) if mf else dom["frac_hbm"], "traffic": traffic,
                "kernel": dom["kernel"], "kernels": parts,
                "model_s_equivalent": {"flops_per_launch": alg_flops, "TFLOPs": alg_flops / sec / 1e12 if sec > 0 else 0.0,
                                       "frac_fp64": alg_flops / sec / 1e12 / FP64_PEAK_TFLOPS if sec > 0 else 0.0,
                                       "end_to_end_frac": alg_flops * evals_per_s / 1e12 / FP64_PEAK_TFLOPS,
                                       "note": "SURVEY.md 8d model-S flops (dense four-product flow) over the measured run time: "
                                               "exceeds 1 where the flow run does less work than model S"},
                "note": "frac = work of the flow ACTUALLY RUN by the dominant (longer) kernel / its HIP-event time / peak: "
                        "matrix-core flops = MFMA instructions x 2048, HBM bytes = dumps written + read; `kernels` prices both halves"}
        if profile and not info.get("expm_action"):
            roof["mfma_utilisation_from_profile"] = profile
    else:
        gbs = alg_bytes / sec / 1e9 if sec > 0 else 0.0
        flow_bytes, flow_flops = local.flow_bytes(uni, thin, fused), local.flow_flops(uni, thin, chunked=chunks > 1)
        flow = {"name": (f"unitary (P_t only), time axis in {chunks} parallel chunks" if chunks > 1 else "unitary (P_t only)")
                        if uni else "general (model S)",
                "bytes_per_launch": flow_bytes,
                "achieved_GBs": flow_bytes / sec / 1e9 if sec > 0 else 0.0,
                "frac_hbm": flow_bytes / sec / 1e9 / HBM_PEAK_GBS if sec > 0 else 0.0,
                "flops_per_launch": flow_flops,
                "achieved_TFLOPs": flow_flops / sec / 1e12 if sec > 0 else 0.0,
                "frac_fp64": flow_flops / sec / 1e12 / FP64_PEAK_TFLOPS if sec > 0 else 0.0}
        # priced on the flow ACTUALLY RUN (as the tile-family lines are): the unitary flow stores P_t only and recomputes the
        # states, so SURVEY.md 8d's algorithmic bytes (model S: P_t and X_t written, then read) over its run time exceed the
        # HBM peak once the kernel is faster than 69.9 us (round 3: 67.4 .. 72 us by box) -- kept as model_s_equivalent
        fb, ff = flow["frac_hbm"], flow["frac_fp64"]
        roof = {"bound": "hbm" if fb >= ff else "valu_fp64",
                "achieved": flow["achieved_GBs"] if fb >= ff else flow["achieved_TFLOPs"],
                "peak": HBM_PEAK_GBS if fb >= ff else FP64_PEAK_TFLOPS, "unit": "GB/s" if fb >= ff else "TFLOP/s",
                "frac": max(fb, ff), "traffic": traffic,
                "kernel": ";".join(names) or ("sweep_pair_kernel" if info.get("lane_pair") else "sweep_small_kernel"),
                "bytes_per_launch": flow_bytes, "flow": flow,
                "model_s_equivalent": {"algorithmic_bytes_per_launch": alg_bytes, "GBs": gbs, "frac_hbm": gbs / HBM_PEAK_GBS,
                                       "end_to_end_frac": alg_bytes * evals_per_s / 1e9 / HBM_PEAK_GBS,
                                       "note": "SURVEY.md 8d algorithmic bytes (model S: every P_t and X_t written once, read "
                                               "once) over the measured kernel time -- the `frac` of rounds 1-2 (0.83 / 0.97); "
                                               "exceeds 1 where the flow run moves fewer bytes than model S"},
                "note": "frac = bytes (or FP64 flops, whichever fraction is larger) of the data flow ACTUALLY RUN by the sweep "
                        "kernel / its HIP-event time / peak; `traffic` = HBM bytes from the committed PMC passes; the kernel "
                        "itself is vector-FP64 issue bound (DESIGN.md section 4.1)"}
    roof.update(st)
    ms_eq = roof["model_s_equivalent"]
    roof["frac_model_s"] = ms_eq.get("frac_hbm", ms_eq.get("frac_fp64"))     # SURVEY.md 8d numerator over the same time
    # ... where it means something: a flow that does less than half of model S's work (the vector flow of C4 does ~1/12 of
    # its flops) makes that ratio a multiple of the peak -- printed as null, the flow's own fraction is `frac`
    if info.get("kernel_family") in (1, 2) and "kernels" in roof:
        done = sum(k.get("mfma_flops_per_launch", k.get("valu_fp64_flops_per_launch", 0.0)) for k in roof.get("kernels", []))
        if done < 0.5 * alg_flops:
            roof["frac_model_s"] = None
    elif "kernels" not in roof and roof.get("bytes_per_launch", alg_bytes) < 0.5 * alg_bytes:
        roof["frac_model_s"] = None
    if info.get("kernel_family") != 1 and info.get("lane_pair") and uni:
        ph = committed_phases(local, st["kernel_avg_us"])
        if ph:
            roof["phases_from_profile"] = ph
    if traffic is not None:
        roof["traffic_source"] = ("HBM bytes of the timed kernels per evaluation = (2*FETCH_SIZE + WRITE_SIZE) KiB from the rocprofv3 "
                                  "--pmc passes of this command committed under profiles/ (profiles/traffic.json names the file); "
                                  "NOT re-measured in this run")
    return roof


def committed_traffic(key):
    """HBM bytes per evaluation from the committed PMC profile of this config (profiles/traffic.json), or None."""
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        v = json.load(open(tpath)).get(key)
        return float(v) if v is not None else None
    except Exception:                          # noqa: BLE001
        return None


def committed_mfma(key):
    """{kernel: matrix-core pipe utilisation} from the committed PMC profile of this config ("from profile"), or None."""
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        t = json.load(open(tpath))
        v = t.get("mfma_utilisation", {}).get(key)
        return dict(v, source=t.get("_sources", {}).get(key, "profiles/")) if v else None
    except Exception:                          # noqa: BLE001
        return None


def committed_phases(local, kernel_us):
    """The lane-pair sweep kernel's phases from the committed phase-stamp profile of this config ("from profile": the
    stamps cost a few percent, so the bench run itself does not carry them): share of the wave's cycles per phase, scaled
    to this run's kernel time, and the rate at which the HBM-bound backward phase reads the stored propagators."""
    path = next((q for q in (os.path.join(ROOT, "profiles", f"r{r:02d}_C3_phase_stamps.json") for r in range(9, 0, -1))
                 if os.path.exists(q)), "")
    try:
        d = json.load(open(path))
        if local.n != 4 or d.get("E") != local.E or local.N != 500:
            return None
        out = {"source": f"profiles/{os.path.basename(path)} (tools/phase_profile.py), shares of a wave's cycles x this run's kernel time"}
        for name, ph in d["phases"].items():
            out[name] = {"share": ph["share"], "us": ph["share"] * kernel_us}
        p_bytes = local.E * local.N * local.n * local.n * 16
        t_d = out["D backward+grad"]["us"] * 1e-6
        out["D backward+grad"].update({"bound": "hbm", "propagator_bytes_read": p_bytes, "GBs": p_bytes / t_d / 1e9,
                                        "frac_hbm": p_bytes / t_d / 1e9 / HBM_PEAK_GBS})
        out["A propagators"]["bound"] = "vector FP64 issue (DESIGN.md section 4.1: ~0.8 of the 4-cycle issue limit)"
        return out
    except Exception:                          # noqa: BLE001
        return None


def box_record(qoc, w, dev_index, kernel_us, evals=40):
    """Which box, at which clock: the record a reader needs to tell a slower kernel from a slower machine.
    Right behind the timed blocks the same workload runs `evals` times on a context built with GRAPE_FLAG_PHASE_STAMPS: every
    wave of the sweep kernel stamps the shader-cycle counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) at
    its start and end, so  clock = cycles / real time  is the clock the SWEEP KERNEL ITSELF ran at (a one-wave probe kernel
    would see the idle boost clock instead).  kernel_cycles = kernel_us x clock is the box-independent figure
    tests/test_gpu_perf_gate.py holds the kernel to."""
    import numpy as np
    import torch
    prop = torch.cuda.get_device_properties(dev_index)
    rec = {"arch": getattr(prop, "gcnArchName", ""), "name": prop.name, "cus": int(prop.multi_processor_count),
           "hbm_gib": round(prop.total_memory / 2 ** 30, 1)}
    if w.n > 4:
        return rec                                     # the stamps live in the lane / lane-pair kernels
    try:
        with qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=dev_index,
                             flags=qoc.engine.FLAG_PHASE_STAMPS) as eng:
            clocks, cyc = [], []
            for i in range(evals):
                eng.eval(w.x)
                if i >= evals // 2 and i % 4 == 0:
                    st = eng.phase_stamps().astype(np.int64)
                    real_ns = (st[:, 6] - st[:, 5]) * 10.0
                    tot = st[:, 4] - st[:, 0]
                    ok = real_ns > 0
                    clocks.append(float(np.median(tot[ok] / real_ns[ok])))
                    cyc.append(float(np.median(tot[ok])))
        rec["clock_ghz"] = float(np.median(clocks))
        rec["clock_ghz_min_max"] = [float(min(clocks)), float(max(clocks))]
        rec["wave_cycles_median"] = float(np.median(cyc))          # one wave's start-to-end cycle count (stamped build)
        rec["kernel_cycles"] = {k: kernel_us[k] * 1e3 * rec["clock_ghz"] for k in ("min", "median", "max") if kernel_us.get(k)}
        rec["how"] = "clock = s_memtime cycles / s_memrealtime (100 MHz) over every wave of the sweep kernel, stamped build, right after the timed blocks; kernel_cycles = kernel_us x clock"
    except Exception as exc:                           # noqa: BLE001 -- a record must not kill the headline
        rec["clock_error"] = repr(exc)[:200]
    return rec


def clock_ramp(step, seconds=0.35, reduce_max=None):
    """Untimed evaluations for at least `seconds` before the first timed block, whatever --warmup says: a 20-step run
    of 0.1 ms calls used to be measured on a GPU still raising its clock (round 2: 83.7 us kernels in the driver's
    run against 72 us in every longer one).
    Several ranks (reduce_max given): a step holds a collective, so every rank must make the SAME number of calls -- a
    loop on each rank's own clock left one rank a call ahead of the other about once in ten runs (a mismatched
    all-reduce).  The ranks time a probe of 8 steps, agree on the slowest rank's figure and all run the count that follows."""
    if reduce_max is None:
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < seconds:
            step()
            n += 1
        return n
    probe = 8
    t0 = time.perf_counter()
    for _ in range(probe):
        step()
    per_step = reduce_max((time.perf_counter() - t0) / probe)      # identical on every rank (all-reduce MAX)
    n = max(0, min(20000, int(seconds / max(per_step, 1e-6)) - probe))
    for _ in range(n):
        step()
    return probe + n


def split_steps(steps, blocks):
    """`steps` timed steps cut into min(blocks, steps) blocks of near-equal size: --steps is the number of steps timed."""
    blocks = max(1, min(blocks, steps))
    return [steps // blocks + (i < steps % blocks) for i in range(blocks)]


def time_blocks(step, sizes, barrier, reduce_max, settle=0):
    """Consecutive timed blocks of sizes[i] steps between a barrier before the first and one after the last; per block
    the MAX over ranks.  Blocks are cut by the host clock alone: a step returns with its results in host memory, and a
    barrier between blocks would drain the device work a step leaves behind (which the next step overlaps in a caller's
    loop) and charge it, with the cold start that follows, to a short block.  `settle` untimed steps follow the first
    barrier for the same reason (C3 on an MI355X: the first ~7 steps after it take 20-30 us more in all).  Also returns
    what the last step returned."""
    last = None
    barrier()
    for _ in range(settle):
        step()
    marks = [time.perf_counter()]
    for i, n in enumerate(sizes):
        for _ in range(n):
            last = step()
        if i == len(sizes) - 1:
            barrier()
        marks.append(time.perf_counter())
    return [reduce_max(b - a) for a, b in zip(marks, marks[1:])], last


def dump_outputs(path, F, G):
    """What a caller of the timed step receives, from its last call: F as a (1,) array, G as (K, N), float64."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "F.npy"), np.array([F], dtype=np.float64))
    np.save(os.path.join(path, "G.npy"), np.ascontiguousarray(G, dtype=np.float64))


def run_extra_config(qoc, name, dev_index, steps, warmup):
    """One more BASELINE config on this GPU, host -> host, with its own roofline (N = 1 only).
    "C4dense": C4 through the dense MFMA chain (GRAPE_FLAG_FORCE_GENERAL) instead of the rank-one vector chain its
    vec(rho) vec(rho)' states allow.  "C5x1": ONE 32 x 32 problem of C5's shape -- the single-`Problem` closure
    (src/solve.jl:63-143), latency-bound: the time axis is evaluated in parallel chunks."""
    dense = name.endswith("dense")
    expm = name.endswith("expm")                           # "C4expm": GRAPE_ACTION=0, the MFMA expm + vector chain flow
    pm = name.endswith("pm")                               # "C4pm": the members' OWN control operators, B_k = (1 + eps_k) B --
    cfg_name = name[:-5] if dense else name[:-4] if expm else name[:-2] if pm else name     # what EnsembleProblem.B_g is for
    members = 0
    if "x" in cfg_name:                                    # "C5x1": the config's shape with that many members
        cfg_name, members = cfg_name.split("x")[0], int(cfg_name.split("x")[1])
    w = qoc.workloads.config(cfg_name, E=members) if members else qoc.workloads.config(cfg_name)
    if pm:                                                 # amplitude inhomogeneity (src/problems.jl:33-41, test/setup_tests.jl:31-32)
        import numpy as np
        w.B = np.ascontiguousarray(w.B * (1.0 + 0.05 * (np.arange(w.E) / w.E - 0.5))[:, None, None, None])
        w.name = name
    # latency-bound lines (hundreds of ~0.1 ms steps): HIP events around one evaluation in eight, as in the headline run -- a
    # pair of events costs ~5 us of such a call
    sampled = qoc.engine.FLAG_TIME_SAMPLED if steps >= 100 else 0
    if expm:
        os.environ["GRAPE_ACTION"] = "0"                   # (read by grape_set_operators)
    try:
        return _run_extra(qoc, name, cfg_name, w, dense, expm, sampled, dev_index, steps, warmup)
    finally:
        if expm:
            os.environ.pop("GRAPE_ACTION", None)


def _run_extra(qoc, name, cfg_name, w, dense, expm, sampled, dev_index, steps, warmup):
    with qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=dev_index,
                         flags=qoc.engine.FLAG_TIME_KERNELS | sampled | (qoc.engine.FLAG_FORCE_GENERAL if dense else 0)) as eng:
        import numpy as np
        xf = np.ascontiguousarray(w.x.T)
        call = eng.bind_eval(xf, np.empty_like(xf))           # the same copy-free host->host call as the headline step
        for _ in range(warmup):
            call()
        clock_ramp(call)
        eng.kernel_time(reset=True)
        t0 = time.perf_counter()
        for _ in range(steps):
            F = call()
        el = time.perf_counter() - t0
        samples = eng.kernel_samples()
        info = eng.info
        names = eng.kernel_names()
        rows = None
        try:                                                  # tile / grid families keep the members' rows anyway
            rows = eng.member_results()
        except Exception:                                     # noqa: BLE001 -- small family without the flag: a second context below
            rows = None
    evals = steps / el
    parity = spot_parity(qoc, w, rows, dense, dev_index)
    return {"id": name, "parity": parity,
            "workload": f"{name}: {w.sys_type} {w.n}x{w.n}, K={w.K}, N={w.N}, E={w.E}, host->host grape_eval"
                        + (" (dense chain forced)" if dense else " (GRAPE_ACTION=0: expm + vector chain)" if expm else ""),
            "value": evals, "unit": "gradient-evals/s", "ms_per_step": 1e3 * el / steps, "steps": steps,
            "member_evals_per_s": evals * w.E, "F": F,
            "roofline": roofline(w, info, samples, evals, 1, None if (dense or expm) else committed_traffic(f"{cfg_name}_E{w.E}"),
                                 committed_mfma(f"{name}_E{w.E}"), names)}


def spot_parity(qoc, w, rows, dense, dev_index, spots=4):
    """The in-line parity leg of an extra config: `spots` members spread over the ensemble (first, last and
    between), this run's per-member rows against the C oracle, at the 1e-10 bar of tests/conftest.py.  The oracle runs the
    spot members on separate threads (OpenMP over members): a 64 x 64 member takes it tens of seconds."""
    import numpy as np
    from oracle import grape_oracle
    try:
        if rows is None:                                       # small family: rows only with GRAPE_FLAG_MEMBER_RESULTS
            with qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=dev_index, member_results=True,
                                 flags=qoc.engine.FLAG_FORCE_GENERAL if dense else 0) as chk:
                chk.eval(w.x)
                rows = chk.member_results()
        foms, grads = rows
        ks = sorted(set(int(round(i * (w.E - 1) / max(spots - 1, 1))) for i in range(min(spots, w.E))))
        sel = np.array(ks)
        t0 = time.perf_counter()
        _, _, foms_ref, grads_ref = grape_oracle.ensemble_eval(w.sys_type, w.A[sel], w.B[sel], w.Xi[sel], w.Xt[sel], w.wts[sel],
                                                               w.x, w.T, per_member=True, n_threads=len(ks))
        gerr = max(float(np.abs(grads[k] - grads_ref[i]).max() / np.abs(grads_ref[i]).max()) for i, k in enumerate(ks))
        ferr = max(float(abs(foms[k] - foms_ref[i]) / (1e-10 * max(abs(foms_ref[i]), 1e-3 * w.n * w.n))) for i, k in enumerate(ks))
        return {"members": ks, "max_rel_G": gerr, "max_F_err_over_tol": ferr, "tol": 1e-10,
                "ok": bool(gerr <= 1e-10 and ferr <= 1.0), "oracle_s": time.perf_counter() - t0}
    except Exception as exc:                                   # noqa: BLE001 -- a check must not kill the line; it says so instead
        return {"error": repr(exc)[:120]}


def scaling_forecast(shards, allreduce_us=15.0):
    """What the driver's N = 2 / 4 / 8 runs should show (strong scaling: every GPU a contiguous 1/N of the members, one
    all-reduce of K N + 1 doubles per step), predicted from the shard steps timed on THIS GPU: evals/s = 1 / (shard step +
    allowance).  allreduce_us is an allowance, not a measurement: a 16-96 KB all-reduce over xGMI is latency-bound (an 8-rank
    ring is 14 hops); nobody has timed it on this pool (SCALE has been skipped every round)."""
    out = {"allreduce_allowance_us": allreduce_us}
    for cfg, sh in shards.items():
        if not isinstance(sh, dict) or "error" in sh:
            continue
        row = {}
        for n_gpus, key in zip((2, 4, 8), sorted(sh.keys(), key=lambda s: -int(s[1:]))):
            row[str(n_gpus)] = 1.0 / (1e-3 * sh[key]["ms_per_step"] + 1e-6 * allreduce_us)
        out[cfg] = row
    return out


def shard_overheads(qoc, cfg_name, dev_index, sizes=(512, 256, 128), steps=300):
    """What a GPU of an N-GPU strong-scaling run does per step, timed on this one: the config's ensemble cut to the shard
    sizes of 2 / 4 / 8 GPUs, host -> host grape_eval, next to the shard's sweep-kernel time.  fixed_overhead_us = the part
    that does not shrink with the shard (x upload, launches, the reduce, publication, host turnaround): an N-GPU step
    costs at least the largest shard's ms_per_step plus the all-reduce, whatever the kernels do."""
    import numpy as np
    out = {}
    for E in sizes:
        w = qoc.workloads.config(cfg_name, E=E)
        with qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=dev_index,
                             flags=qoc.engine.FLAG_TIME_KERNELS | (qoc.engine.FLAG_TIME_SAMPLED if steps >= 32 else 0)) as eng:   # (an event pair costs ~5 us: every 8th call, as the headline; short runs time every call)
            xf = np.ascontiguousarray(w.x.T)
            call = eng.bind_eval(xf, np.empty_like(xf))
            for _ in range(min(20, steps)):
                call()
            clock_ramp(call, 0.15)
            eng.kernel_time(reset=True)
            t0 = time.perf_counter()
            for _ in range(steps):
                call()
            el = time.perf_counter() - t0
            tot_ms, _ = eng.kernel_samples()
        k_us = float(np.mean(tot_ms) * 1e3)                  # HIP events around the sweep kernel(s) of an evaluation
        out[f"E{E}"] = {"ms_per_step": 1e3 * el / steps, "sweep_kernel_us": k_us,
                        "fixed_overhead_us": 1e6 * el / steps - k_us}
    return out


def lbfgs_rates(qoc, dev_index):
    """The library's device-resident L-BFGS (grape_lbfgs, Hager-Zhang line search as Optim's LBFGS()) next to the
    host-driven loop (SciPy L-BFGS-B calling grape_eval, the stand-in for Optim.jl on the host) on two shapes: the
    reference's own n_ens = 5 StateTransfer testset, and the headline-shaped ensemble.  Reported per driver: minimum,
    iterations, evaluations, seconds for the same iteration budget -- and, in BOTH directions, the evaluations and
    seconds each driver needs to reach the OTHER's final minimum (iterations per second alone say nothing when the
    progress per iteration differs)."""
    import numpy as np
    from scipy.optimize import minimize
    out = []
    for label, w, iters in (("reference testset: StateTransfer 2x2, n_ens=5, N=25 (state_transfer_tests.jl:42)",
                             qoc.workloads.reference_ensemble("StateTransfer", 5, 25, 5.0), 40),
                            ("C3-shaped StateTransfer ensemble (4x4, K=4, N=500, E=1024), 30 iterations", "st4", 30)):
        if w == "st4":                              # the headline operators with density-matrix states: here the
            w = qoc.workloads.config("C3")          # reference gradient is a consistent descent direction
            rho0 = np.zeros((4, 4), complex); rho0[0, 0] = 1
            psi = np.array([1, 1j, -1, 0.5]) / np.linalg.norm([1, 1j, -1, 0.5])
            w.sys_type = "StateTransfer"
            w.Xi = np.broadcast_to(rho0, (w.E, 4, 4)).copy()
            w.Xt = np.broadcast_to(np.outer(psi, psi.conj()), (w.E, 4, 4)).copy()
        ug = w.sys_type == "UnitaryGate"
        with qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, device=dev_index,
                             variant=1 if ug else 0) as eng:
            eng.lbfgs(w.x, iterations=3)                                   # warm
            # (the median of three identical runs: one run of a few milliseconds is at the mercy of the host's scheduler)
            info = sorted((eng.lbfgs(w.x, iterations=iters)[1] for _ in range(3)), key=lambda r: r["seconds"])[1]
            strict = sorted((eng.lbfgs(w.x, iterations=iters, line_search="optim")[1] for _ in range(3)),
                            key=lambda r: r["seconds"])[1]

            # host-driven: every evaluation stamped, so that "reached F at evaluation n after t seconds" can be read off
            trace = []
            t0 = time.perf_counter()

            def fun(xf):
                F, G = eng.eval(xf.reshape(w.K, w.N))
                trace.append((len(trace) + 1, time.perf_counter() - t0, F))
                return F, G.reshape(-1)
            res = minimize(fun, w.x.reshape(-1), jac=True, method="L-BFGS-B",
                           options={"maxiter": iters, "gtol": 1e-8, "ftol": 1e-15, "maxls": 40})
            host_s = time.perf_counter() - t0
            host_min, host_nfev, host_nit = float(res.fun), int(res.nfev), int(res.nit)
            # host -> the device loop's minimum: continue the host loop with a larger budget if it has not got there
            def host_reach(target):
                tr, t1 = [], time.perf_counter()

                def f2(xf):
                    F, G = eng.eval(xf.reshape(w.K, w.N))
                    tr.append((len(tr) + 1, time.perf_counter() - t1, F))
                    return F, G.reshape(-1)
                minimize(f2, w.x.reshape(-1), jac=True, method="L-BFGS-B",
                         options={"maxiter": 10 * iters, "gtol": 1e-8, "ftol": 1e-15, "maxls": 40})
                hit = next(((n, t) for n, t, F in tr if F <= target), None)
                return {"evaluations": hit[0], "seconds": hit[1]} if hit else {"evaluations": None, "seconds": None,
                                                                               "note": f"not reached in {len(tr)} evaluations"}
            # device -> the host loop's minimum: smallest iteration budget whose result is at or below it
            def device_reach(target):
                for it in range(1, 10 * iters + 1):
                    _, r = eng.lbfgs(w.x, iterations=it)
                    if r["minimum"] <= target or r["status"] != 2:
                        ok = r["minimum"] <= target
                        return {"iterations": r["iterations"], "evaluations": r["evaluations"] if ok else None,
                                "seconds": r["seconds"] if ok else None}
                return {"evaluations": None, "seconds": None}
            tol = 1e-9 * max(1.0, abs(host_min))
            out.append({"problem": label,
                        "device_lbfgs": {"line_search": "Hager-Zhang (initial step accepted when Wolfe holds)",
                                         "iterations": info["iterations"], "evaluations": info["evaluations"],
                                         "seconds": info["seconds"], "minimum": info["minimum"], "status": info["message"],
                                         "ladder_fallbacks": info["ladder_fallbacks"]},
                        "device_lbfgs_optim_strict": {"line_search": "Hager-Zhang as Optim runs it behind InitialStatic",
                                                      "iterations": strict["iterations"], "evaluations": strict["evaluations"],
                                                      "seconds": strict["seconds"], "minimum": strict["minimum"]},
                        "host_driven_scipy": {"iterations": host_nit, "evaluations": host_nfev, "seconds": host_s,
                                              "minimum": host_min},
                        "to_reach_the_host_loops_minimum": {"device_lbfgs": device_reach(host_min + tol),
                                                            "host_driven_scipy": {"evaluations": host_nfev, "seconds": host_s}},
                        "to_reach_the_device_loops_minimum": {"device_lbfgs": {"evaluations": info["evaluations"],
                                                                               "seconds": info["seconds"]},
                                                              "host_driven_scipy": host_reach(info["minimum"] + tol)}})
    return out


def _r(v, digits=4):
    """Numbers of the printed line: 4-5 significant digits are what the measurement has."""
    if isinstance(v, float):
        return float(f"{v:.{digits}g}")
    return v


def compact_roofline(r):
    """bound / achieved / peak / unit / frac / traffic as the contract asks, plus frac_model_s (SURVEY.md 8d numerator over the
    same kernel time; `frac` prices the flow actually run), the kernel names the library reported and the event times."""
    out = {k: _r(r[k], 5) for k in ("bound", "achieved", "peak", "unit", "frac", "frac_model_s", "traffic") if k in r}
    out["kernel"] = r.get("kernel")
    out["kernel_us"] = {"avg": _r(r.get("kernel_avg_us")), "min": _r(r.get("kernel_min_us")), "median": _r(r.get("kernel_median_us")),
                        "max": _r(r.get("kernel_max_us")), "launches": r.get("kernel_launches")}
    if "bytes_per_launch" in r:
        out["bytes_per_launch"] = r["bytes_per_launch"]
        out["model_s_bytes_per_launch"] = r["model_s_equivalent"]["algorithmic_bytes_per_launch"]
    if "kernels" in r:                          # tile family: both timed parts, priced on the flow run
        out["parts"] = [{"kernel": k["kernel"], "us": _r(k["avg_us"]), "bound": k["bound"],
                         "frac": _r(k.get("frac_mfma", k.get("frac_valu_fp64", 0.0)) if k["bound"] != "hbm" else k["frac_hbm"]),
                         "frac_hbm": _r(k["frac_hbm"])} for k in r["kernels"]]
    m = r.get("mfma_utilisation_from_profile")
    if m:
        out["mfma_util_from_profile"] = {k: _r(v) for k, v in m.items() if k != "source"}
    return out


def compact(out):
    """The ONE printed JSON line, <= 7.5 KB: the driver keeps an 8 KB tail of stdout (round 3's 17.8 KB line lost C2, C4 and
    the L-BFGS figures there).  Prose lives in DESIGN.md section 5; `--details FILE` / `--verbose` give the complete record."""
    c = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                             "vs_baseline", "dtype", "data") if k in out}
    c["value"], c["ms_per_step"] = _r(out["value"], 6), _r(out["ms_per_step"], 5)
    cfg = out["config"]
    c["config"] = {"workload": cfg["workload"].split("; step =")[0] + "; step = host->host grape_eval", "parallelism": cfg["parallelism"]}
    if cfg.get("collective"):
        c["config"]["collective"] = cfg["collective"]
    c["blocks_s"] = [_r(t) for t in out["blocks"]["seconds"]]
    c["roofline"] = compact_roofline(out["roofline"])
    if "box" in out:
        c["box"] = {k: (_r(v, 5) if not isinstance(v, (dict, list)) else ({kk: _r(vv, 6) for kk, vv in v.items()} if isinstance(v, dict) else [_r(x, 5) for x in v]))
                    for k, v in out["box"].items() if k != "how"}
    cb = out.get("cpu_baseline")
    if cb:
        c["cpu_baseline"] = {"value": _r(cb["value"]), "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"],
                             "sample": cb["sample"].split(" of oracle")[0] + " of the C oracle",
                             "all_cores": {"value": _r(cb["all_cores"]["value"]), "cores": cb["all_cores"]["cores"]}}
    if "parity" in out:
        c["parity"] = {k: _r(v, 3) for k, v in out["parity"].items()}
    ex = out.get("extra") or {}
    cx = {}
    if "device_resident_pipelined" in ex:
        cx["device_resident_pipelined"] = _r(ex["device_resident_pipelined"]["value"], 5)
    if "weak_scaling" in ex:
        cx["weak_scaling"] = {k: _r(v, 5) for k, v in ex["weak_scaling"].items()
                              if k in ("value", "ms_per_step", "ensemble_total", "scaling", "error")}
    if "ipc_exchange" in ex:
        cx["ipc_exchange"] = {k: (_r(v, 5) if k != "error" else str(v)[:100]) for k, v in ex["ipc_exchange"].items() if k in ("value", "ms_per_step", "error")}
    if isinstance(ex.get("lbfgs"), list):
        cx["lbfgs"] = [{"problem": "reference n_ens=5 testset" if e["problem"].startswith("reference") else "C3-shaped StateTransfer E=1024",
                        "device": [e["device_lbfgs"]["iterations"], e["device_lbfgs"]["evaluations"], _r(1e3 * e["device_lbfgs"]["seconds"]),
                                   _r(e["device_lbfgs"]["minimum"], 7)],
                        "host_scipy": [e["host_driven_scipy"]["iterations"], e["host_driven_scipy"]["evaluations"],
                                       _r(1e3 * e["host_driven_scipy"]["seconds"]), _r(e["host_driven_scipy"]["minimum"], 7)]}
                       for e in ex["lbfgs"]]
        cx["lbfgs_columns"] = "iterations, evaluations, ms, minimum"
    elif "lbfgs" in ex:
        cx["lbfgs"] = ex["lbfgs"]
    if isinstance(ex.get("shard_fixed_overhead"), dict):
        cx["shard_ms_kernel_us"] = {k: ([_r(v["ms_per_step"]), _r(v["sweep_kernel_us"])] if "ms_per_step" in v else v)
                                    for k, v in ex["shard_fixed_overhead"].items()}
    if isinstance(ex.get("scaling_forecast"), dict):
        cx["scaling_forecast"] = {k: ({kk: _r(vv, 4) for kk, vv in v.items()} if isinstance(v, dict) else v)
                                  for k, v in ex["scaling_forecast"].items()}
    if cx:
        c["extra"] = cx
    if "extra_configs" in out:
        c["extra_configs"] = []
        c["extra_parity_columns"] = "spot members, max rel G err, max F err/tol, ok (C oracle, 1e-10)"
        for e in out["extra_configs"]:
            if "error" in e:
                c["extra_configs"].append({"id": e.get("workload"), "error": e["error"][:120]})
                continue
            par = e.get("parity") or {}
            cpar = ([len(par["members"]), _r(par["max_rel_G"], 2), _r(par["max_F_err_over_tol"], 2), par["ok"]]
                    if "members" in par else {"error": par.get("error", "none")})
            if "x" in e["id"] or e["id"] == "L1d":      # single problems (the `Problem` closure) and the 4 x 1 Liouvillian ensemble: rate, time, kernels
                c["extra_configs"].append({"id": e["id"], "value": _r(e["value"], 5), "ms_per_step": _r(e["ms_per_step"], 5),
                                           "kernel": e["roofline"].get("kernel"), "parity": cpar})
                continue
            if e["id"].endswith("pm"):                  # per-member controls: the rate, its ratio to the shared-controls line, kernels
                base = next((b for b in out["extra_configs"] if b.get("id") == e["id"][:-2]), None)
                base_v = base["value"] if base else (out["value"] if e["id"][:-2] == out["config"]["workload"].split(":")[0] else None)
                c["extra_configs"].append({"id": e["id"], "value": _r(e["value"], 5), "ms_per_step": _r(e["ms_per_step"], 5),
                                           "vs_shared_controls": _r(e["value"] / base_v, 3) if base_v else None,
                                           "kernel": e["roofline"].get("kernel"), "parity": cpar})
                continue
            cr = compact_roofline(e["roofline"])
            for k in ("bytes_per_launch", "model_s_bytes_per_launch"):      # (the headline's roofline keeps them; the line has 8 KB)
                cr.pop(k, None)
            c["extra_configs"].append({"id": e["id"], "value": _r(e["value"], 5), "ms_per_step": _r(e["ms_per_step"], 5),
                                       "roofline": cr, "parity": cpar})
    for k in ("ranks_seen", "rank_kernel_us"):
        if k in out:
            c[k] = out[k] if k == "ranks_seen" else {kk: _r(vv) for kk, vv in out[k].items()}
    c["F"] = out.get("F")
    return c


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks as fresh child
    processes (nothing in THIS process has touched the GPU yet), relay their output, exit with
    their code.  Never re-exec a process that initialised HIP."""
    import torch                                   # device_count() does not initialise the GPU on this image

    have = torch.cuda.device_count()
    if have < args.gpus and not os.environ.get("GRAPE_BENCH_SHARE_GPU"):      # (sharing: plumbing tests only)
        raise SystemExit(f"bench.py: --gpus {args.gpus} but only {have} HIP device(s) are visible; refusing to "
                         f"report a {args.gpus}-GPU number from fewer GPUs")
    port = 29500 + os.getpid() % 400
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300, help="timed steps")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=3, help="the timed steps are cut into this many blocks; value = median block")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: box clock, CPU baseline + parity, device-resident loop, "
                         "L-BFGS, shard overheads, extra configs (N > 1: the weak-scaling and mailbox companions)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write F and G of the last timed step to DIR/F.npy and DIR/G.npy (float64, G as (K, N))")
    ap.add_argument("--config", default="C3", help="workload: C2, C3 (headline), C4, C5")
    ap.add_argument("--ensemble", type=int, default=0, help="override E (default: the config's)")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="strong: the config's ensemble is split over the GPUs (north star); "
                         "weak: every GPU gets a full-size ensemble shard")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--cpu-sample", type=int, default=32)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the device-resident loop and the extra configs")
    ap.add_argument("--extra-configs", default="C4,C5,C4dense,C4expm,C6,C7,C2,C5x1,C4x1,C6x1,C7x1,L1d,C3pm,C4pm,C5pm")
    ap.add_argument("--details", default="", help="also write the complete record (every note, per-kernel model, L-BFGS traces) "
                                                  "to this file; the printed line stays compact")
    ap.add_argument("--verbose", action="store_true", help="print the complete record instead of the compact line")
    ap.add_argument("--backend", default="",
                    help="torch.distributed backend; default: gloo as the control plane when the data-path collective "
                         "is RCCL inside the library (--collective lib), cpu:gloo,cuda:nccl for --collective torch")
    ap.add_argument("--collective", choices=["lib", "ipc", "torch"], default="lib",
                    help="lib: ncclAllReduce inside libgrape_hip.so (grape_comm_attach, the north star's exchange); ipc: the "
                         "library's mailbox exchange over HIP IPC handles (grape_ipc_attach, no RCCL); torch: torch.distributed.all_reduce")
    ap.add_argument("--force-dist", action="store_true",
                    help="run the collective even with one rank (a 1-rank RCCL communicator)")
    ap.add_argument("--force-general", action="store_true",
                    help="use the general data flow (forward states stored) even for Hermitian generators")
    ap.add_argument("--slices-per-lane", type=int, default=0)
    ap.add_argument("--waves-per-member", type=int, default=0)
    args = ap.parse_args()

    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    extras = args.full and not args.no_extra
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)                          # does not return
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; refusing to mislabel the run")

    import numpy as np
    import torch
    import torch.distributed as dist

    import quoptimalcontrol_jl_amd as qoc
    from quoptimalcontrol_jl_amd.distributed import sharded_engine

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    if world > torch.cuda.device_count() and not os.environ.get("GRAPE_BENCH_SHARE_GPU"):
        raise SystemExit(f"bench.py: {world} ranks but {torch.cuda.device_count()} GPU(s): one rank per GPU is the contract")
    dev_index = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group(args.backend or ("gloo" if args.collective in ("lib", "ipc") else "cpu:gloo,cuda:nccl"))

    base = qoc.workloads.config(args.config)
    E_cfg = args.ensemble or base.E
    E_total = E_cfg * (world if args.scaling == "weak" else 1)
    w = qoc.workloads.config(args.config, E=E_total) if E_total != base.E else base

    sg = sharded_engine(w, device, force_collective=args.force_dist, collective=args.collective,
                        flags=qoc.engine.FLAG_TIME_KERNELS | qoc.engine.FLAG_TIME_SAMPLED |
                        (qoc.engine.FLAG_FORCE_GENERAL if args.force_general else 0),
                        slices_per_lane=args.slices_per_lane, waves_per_member=args.waves_per_member)
    x_host = np.ascontiguousarray(w.x)

    def barrier():
        if world > 1:
            dist.all_reduce(torch.zeros(1))        # CPU tensor: the gloo half of the control plane
        torch.cuda.synchronize(device)

    def reduce_max(seconds):
        if world > 1:
            t = torch.tensor([seconds], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return seconds

    # the step, as a compiled caller makes it: buffers in the library's (K,N) column-major layout, allocated once
    xf = np.ascontiguousarray(w.x.T)
    Gf = np.empty_like(xf)
    direct = sg.local is not None and (sg.collective in ("lib", "ipc") or (world == 1 and not args.force_dist))

    bound = sg.local.bind_eval(xf, Gf) if direct else None

    def step():
        if direct:
            return bound(), Gf                     # grape_eval: host -> GPUs -> host, all-reduce inside the library
        return sg.eval(x_host)

    for _ in range(args.warmup):
        step()
    # >= 0.35 s of untimed calls: the timed blocks see a warm clock (N > 1: the same number of calls on every rank)
    ramp_steps = clock_ramp(step, reduce_max=reduce_max if world > 1 else None)
    barrier()
    if sg.local is not None:
        sg.local.kernel_time(reset=True)
    sizes = split_steps(args.steps, args.blocks)
    block_s, (F_last, G_last) = time_blocks(step, sizes, barrier, reduce_max, settle=8)
    G_last = np.array(G_last.T if direct else G_last)          # (K, N), as grape_eval's caller reads it
    samples = sg.local.kernel_samples() if sg.local is not None else ([], [])
    info = sg.local.info if sg.local is not None else {}
    names = sg.local.kernel_names() if sg.local is not None and hasattr(sg.local, "kernel_names") else []
    step_s = statistics.median([t / n for t, n in zip(block_s, sizes)])
    rank_kernel = None
    if world > 1:                                  # every rank's own sweep-kernel time (median of its HIP-event samples): min / max over ranks
        mine = float(np.median(samples[0]) * 1e3) if len(samples[0]) else float("nan")
        t = torch.tensor([mine, -mine], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        rank_kernel = {"min": float(t[0].item()), "max": float(-t[1].item())}

    # ---- the device-resident pipelined loop round 1 reported (x and [G,F] stay in HBM, one sync at the end)
    extra = None
    if extras:
        x_dev = torch.as_tensor(np.ascontiguousarray(w.x.T), device=device)
        for _ in range(min(args.warmup, 10)):
            sg.eval_device(x_dev)
        dev_s = time_blocks(lambda: sg.eval_device(x_dev), [args.steps], barrier, reduce_max)[0][0]
        extra = {"device_resident_pipelined": {
            "value": args.steps / dev_s * (E_total / E_cfg), "ms_per_step": 1e3 * dev_s / args.steps,
            "what": "grape_eval_device back to back, x and [G,F] resident in HBM, one sync after all steps: "
                    "kernel throughput, not a rate a sequential optimiser can reach"}}

    # ---- N > 1: the companion weak-scaling figure (every GPU a full-size ensemble shard, same step, same all-reduce):
    # the headline stays the north star's strong-scaling number; this one shows what the exchange costs when the
    # per-GPU work does not shrink
    if world > 1 and args.scaling == "strong" and extras:
        try:
            w_weak = qoc.workloads.config(args.config, E=E_cfg * world)
            sg_w = sharded_engine(w_weak, device, force_collective=args.force_dist, collective=args.collective,
                                  flags=qoc.engine.FLAG_FORCE_GENERAL if args.force_general else 0)
            xw = np.ascontiguousarray(w_weak.x.T)
            Gw = np.empty_like(xw)
            direct_w = sg_w.local is not None and sg_w.collective == "lib"
            bound_w = sg_w.local.bind_eval(xw, Gw) if direct_w else None
            step_w = (lambda: bound_w()) if direct_w else (lambda: sg_w.eval(np.ascontiguousarray(w_weak.x)))
            for _ in range(min(args.warmup, 10)):
                step_w()
            weak_s = statistics.median(time_blocks(step_w, [args.steps] * args.blocks, barrier, reduce_max)[0])
            sg_w.close()
            extra = dict(extra or {})
            extra["weak_scaling"] = {
                "value": args.steps / weak_s * world, "unit": "gradient-evals/s", "ms_per_step": 1e3 * weak_s / args.steps,
                "ensemble_total": E_cfg * world, "scaling": "weak",
                "what": f"every GPU evaluates a full E={E_cfg} shard of a {E_cfg * world}-member ensemble per step, one "
                        f"all-reduce; value = steps/s x {world} in units of the config's {E_cfg}-member evaluation"}
        except Exception as exc:                   # noqa: BLE001 -- an extra must not kill the headline
            extra = dict(extra or {})
            extra["weak_scaling"] = {"error": repr(exc)}

    # ---- N > 1 with the RCCL exchange: the same strong-scaling step through the library's mailbox exchange (no RCCL), so that
    # a multi-GPU run shows both side by side.  It runs in a watched thread: the headline above is already measured, and
    # a companion that gets stuck on hardware nobody has tried it on must not take the line with it (after 90 s the ranks
    # print what they have and leave through os._exit).
    companion_stuck = False
    if world > 1 and args.scaling == "strong" and extras and args.collective == "lib" \
            and os.environ.get("GRAPE_BENCH_IPC_COMPANION", "1") != "0":
        import threading
        box = {}

        def _companion():
            try:
                sg_i = sharded_engine(w, device, collective="ipc", flags=qoc.engine.FLAG_FORCE_GENERAL if args.force_general else 0)
                if sg_i.collective == "ipc":
                    Gi = np.empty_like(xf)
                    bound_i = sg_i.local.bind_eval(xf, Gi)
                    for _ in range(min(args.warmup, 10)):
                        bound_i()
                    ipc_s = statistics.median(time_blocks(bound_i, [args.steps] * args.blocks, barrier, reduce_max)[0])
                    box["res"] = {"value": args.steps / ipc_s, "unit": "gradient-evals/s", "ms_per_step": 1e3 * ipc_s / args.steps,
                                  "what": "the same step with collective='ipc' (ipc_allreduce_kernel instead of ncclAllReduce + copy)"}
                else:
                    box["res"] = {"error": getattr(sg_i, "attach_error", "not attached")}
                sg_i.close()
            except Exception as exc:               # noqa: BLE001 -- an extra must not kill the headline
                box["res"] = {"error": repr(exc)}
        th = threading.Thread(target=_companion, daemon=True)
        th.start()
        th.join(90.0)
        companion_stuck = th.is_alive()
        extra = dict(extra or {})
        extra["ipc_exchange"] = {"error": "did not finish within 90 s"} if companion_stuck else box.get("res", {"error": "no result"})

    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, F_last, G_last)
        evals_per_s = 1.0 / step_s
        # units: with weak scaling the job evaluates world x the config's ensemble per step;
        # report in the metric's unit (evaluations of the CONFIG's E-member ensemble).
        value = evals_per_s * (E_total / E_cfg)
        local = w.members(sg.lo, sg.hi)
        traffic = committed_traffic(f"{args.config}_E{local.E}")
        roof = roofline(local, info, samples, evals_per_s, world, traffic, committed_mfma(f"{args.config}_E{local.E}"), names)
        n_joined = sg.comm_size if (world > 1 or args.force_dist) else 1
        out = {
            "metric": "GRAPE gradient-evals/sec", "value": value, "unit": "gradient-evals/s",
            "n_gpus": n_joined, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * step_s, "higher_is_better": True,
            "scaling": args.scaling, "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{args.config}: {w.sys_type} {w.n}x{w.n}, K={w.K}, N={w.N} slices, "
                                   f"ensemble E={E_total} ({'sharded' if world > 1 else 'one GPU'}, "
                                   f"{local.E} members/GPU), T={w.T}; step = host->host grape_eval "
                                   f"(x in host memory -> F, G in host memory, blocking)",
                       "parallelism": (f"ensemble-shard x{world}, one all-reduce of {w.K * w.N + 1} f64 per step "
                                       f"({'ncclAllReduce inside libgrape_hip.so' if sg.collective == 'lib' else 'mailbox exchange inside libgrape_hip.so (HIP IPC)' if sg.collective == 'ipc' else 'torch.distributed'})")
                                      if world > 1 else "single GPU",
                       "collective": sg.collective if (world > 1 or args.force_dist) else None,
                       "slices_per_lane": info.get("slices_per_lane"),
                       "waves_per_member": info.get("waves_per_member")},
            "blocks": {"count": len(sizes), "steps_each": sizes, "seconds": block_s, "statistic": "median time per step",
                       "untimed_ramp_steps": ramp_steps},
            "member_evals_per_s": evals_per_s * E_total,
            "roofline": roof,
            "F": float(F_last),
        }
        if args.full:
            out["box"] = box_record(qoc, local, dev_index, {"min": roof["kernel_min_us"], "median": roof["kernel_median_us"],
                                                            "max": roof["kernel_max_us"]})
        if extra is not None:
            out["extra"] = extra
        if world > 1 or args.force_dist:
            out["ranks_seen"] = n_joined           # the communicator's own count (ncclCommCount / the mailbox group), not WORLD_SIZE
            if rank_kernel:
                out["rank_kernel_us"] = rank_kernel
        if world == 1 and args.full and not args.no_cpu_baseline:
            cb, (foms_ref, grads_ref) = cpu_baseline(w, args.cpu_seconds, args.cpu_sample)
            out["cpu_baseline"] = cb
            m = len(foms_ref)
            ws = w.members(0, m)                       # same members through the HIP path, rows kept
            with qoc.GrapeEngine(ws.sys_type, ws.A, ws.B, ws.Xi, ws.Xt, ws.wts, ws.T, ws.N, device=dev_index,
                                 member_results=True) as chk:
                chk.eval(ws.x)
                foms, grads = chk.member_results()
            gerr = float(np.abs(grads[:m] - grads_ref).max() / np.abs(grads_ref).max())
            ftol = 1e-10 * np.maximum(np.abs(foms_ref), 1e-3 * w.n * w.n)
            ferr = float((np.abs(foms[:m] - foms_ref) / ftol).max())
            out["parity"] = {"members_checked": m, "max_rel_G": gerr, "max_F_err_over_tol": ferr,
                             "tol": 1e-10, "ok": bool(gerr <= 1e-10 and ferr <= 1.0)}
    else:
        out = None

    sg.close()
    if rank == 0 and world == 1 and extras:
        try:
            out["extra"]["lbfgs"] = lbfgs_rates(qoc, dev_index)
        except Exception as exc:                   # noqa: BLE001 -- an extra must not kill the headline
            out["extra"]["lbfgs"] = {"error": repr(exc)}
        try:
            out["extra"]["shard_fixed_overhead"] = shard_overheads(qoc, args.config, dev_index)
        except Exception as exc:                   # noqa: BLE001
            out["extra"]["shard_fixed_overhead"] = {"error": repr(exc)}
        shards = {args.config: out["extra"]["shard_fixed_overhead"]}
        for cfg, sizes, st in (("C4", (512, 256, 128), 20), ("C5", (2048, 1024, 512), 3)):
            if cfg == args.config or cfg not in args.extra_configs.split(","):
                continue
            try:
                shards[cfg] = shard_overheads(qoc, cfg, dev_index, sizes, st)
            except Exception as exc:               # noqa: BLE001
                shards[cfg] = {"error": repr(exc)}
        out["extra"]["scaling_forecast"] = scaling_forecast(shards)
    if rank == 0 and world == 1 and extras and args.extra_configs:
        out["extra_configs"] = []
        for name in [s for s in args.extra_configs.split(",") if s and s != args.config]:
            heavy = name in ("C4", "C4dense", "C4expm", "C5", "C6", "C7", "C4pm", "C5pm", "C6x1", "C7x1")
            slow = name in ("C5", "C6", "C7", "C5pm")
            try:
                out["extra_configs"].append(run_extra_config(qoc, name, dev_index, 3 if slow else (20 if heavy else 200),
                                                             1 if slow else (3 if heavy else 20)))
            except Exception as exc:               # noqa: BLE001 -- an extra line must not kill the headline
                out["extra_configs"].append({"workload": name, "error": repr(exc)})
    # the JSON line must be the LAST thing on stdout: flush what native libraries (RCCL prints a version banner
    # through C stdio, block-buffered on a pipe) still hold, on every rank, before rank 0 prints
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:                          # noqa: BLE001
        pass
    sys.stdout.flush()
    if companion_stuck:                            # a thread of this process is wedged in a collective: no orderly teardown
        if out is not None:
            print(json.dumps(out if args.verbose else compact(out), separators=(",", ":")), flush=True)
        os._exit(0)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    if out is not None:
        if args.details:
            with open(args.details, "w") as fh:
                json.dump(out, fh, indent=1)
        print(json.dumps(out if args.verbose else compact(out), separators=(",", ":")), flush=True)
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:                      # noqa: BLE001
            pass


if __name__ == "__main__":
    main()
