"""GPU: short random walks with grape_set_bounds among the settings that live on a context -- bounds, basis, penalties and a
running cost switched on, changed and off, operator re-uploads between (tests/bounds_sequences.py draws them,
test_bounds_host.py shows on the CPU that every pairing of the bounds with another setting occurs).  Every evaluation is held
to the NumPy reference (oracle + penalty_ref + running_cost_ref on the saturated pulse, slope and projection in NumPy) at the
project's 1e-10 bar.  In process: a failure prints the context and the steps walked so far."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_sequences as bs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", bs.SEEDS)
def test_bounds_survive_random_sequences(qoc, oracle, monkeypatch, seed):
    lines = []

    def setenv(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)

    rng = np.random.default_rng(7000 + seed)
    checks = 0
    try:
        for ci in range(bs.CONTEXTS_PER_SEED):
            ctx = bs.draw_context(rng)
            steps = bs.draw_steps(rng, ctx)
            checks += bs.run_context(qoc, oracle, ctx, steps, setenv, ("bounds", seed, ci), lines.append)
    except BaseException:
        start = max(i for i, line in enumerate(lines) if line.startswith("context"))
        print(f"seed {seed}:")
        print("\n".join(lines[start:]))
        raise
    assert checks >= bs.CONTEXTS_PER_SEED
