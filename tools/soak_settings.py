#!/usr/bin/env python3
"""Randomised soak of the settings that live on a context (penalties, basis, running cost, fom) across operator re-uploads:
the walks of tests/settings_sequences.py, as many as asked for, each check against the composed reference.
usage: tools/soak_settings.py [contexts] [seed]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import quoptimalcontrol_jl_amd as qoc  # noqa: E402
import settings_sequences as ss  # noqa: E402
from oracle import grape_oracle as orc  # noqa: E402

contexts = int(sys.argv[1]) if len(sys.argv) > 1 else 60
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
orc.build()
rng = np.random.default_rng(seed)
fails = checks = 0
t0 = time.time()


def setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


for ci in range(contexts):
    ctx = ss.draw_context(rng)
    steps = ss.draw_steps(rng, ctx)
    lines = []
    try:
        checks += ss.run_context(qoc, orc, ctx, steps, setenv, None, lines.append)
    except Exception as exc:                          # noqa: BLE001
        fails += 1
        print(f"FAIL context {ci}\n  " + "\n  ".join(lines) + "\n  -> " + repr(exc)[:400], flush=True)
print(f"settings soak: {contexts} contexts, {checks} checked operations, {fails} failures, {time.time() - t0:.1f} s (seed {seed})")
sys.exit(1 if fails else 0)
