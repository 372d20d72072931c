#!/usr/bin/env python3
"""Randomised soak of the trajectory calls (read-out, VJP, JVP, device forms and reuse, the exact modes, the risk) between the
settings that live on a context: the walks of tests/trajectory_sequences.py over a range of seeds, each check against the
references, the bitwise memo and the flag model.  The suite runs seeds 0:40 (test_gpu_trajectory_soak.py); this is the long run.
--family: the family walk of tests/trajectory_family_sequences.py instead (the multi, HVP, GNVP and mean forms among the older
calls; the suite runs its committed seeds in test_gpu_trajectory_family_soak.py).
usage: tools/soak_trajectory.py [--family] [--seeds A:B] [--contexts C]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quoptimalcontrol_jl_amd as qoc  # noqa: E402
import trajectory_sequences as ts  # noqa: E402
from oracle import grape_oracle as orc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", default="100:160", help="A:B, the seeds A .. B-1")
ap.add_argument("--contexts", type=int, default=ts.CONTEXTS_PER_SEED, help="contexts per seed")
ap.add_argument("--family", action="store_true", help="the family walk (tests/trajectory_family_sequences.py)")
args = ap.parse_args()
if args.family:
    import trajectory_family_sequences as ts  # noqa: E402,F811
first, last = (int(v) for v in args.seeds.split(":"))
orc.build()
fails = checks = contexts = 0
t0 = time.time()


def setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


for seed in range(first, last):
    for ci, (ctx, steps) in enumerate(ts.walk_seed(seed, args.contexts)):
        lines = []
        contexts += 1
        try:
            done = ts.run_context(qoc, orc, ctx, steps, setenv, (seed, ci), lines.append)
            assert done == ts.drawn_checks(steps), (done, ts.drawn_checks(steps))
            checks += done
        except Exception as exc:                      # noqa: BLE001
            fails += 1
            print(f"FAIL seed {seed} context {ci}\n  " + "\n  ".join(lines) + "\n  -> " + repr(exc)[:600], flush=True)
            if getattr(exc, "status", 0) == -4 or "HIP" in repr(exc):     # a device error: nothing more is started on the GPU
                print("device error: the soak ends here", flush=True)
                sys.exit(2)
print(f"trajectory {'family ' if args.family else ''}soak: seeds {first}:{last}, {contexts} contexts, {checks} checked operations, {fails} failures, "
      f"{time.time() - t0:.1f} s")
sys.exit(1 if fails else 0)
