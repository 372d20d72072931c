"""GPU: random walks over the trajectory calls -- the read-out, its pull-back and push-forward, their device forms and the
d_x = NULL reuse, the two exact derivative modes and the risk -- between the settings of the older walks and across operator
re-uploads (tests/trajectory_sequences.py draws them, test_trajectory_sequences_host.py shows on the CPU what the committed
seeds cover and that no mix-up can hide).  Every result is held to the NumPy / oracle references at the project's 1e-10 bar and
to every earlier result with the same key bit for bit; a reuse call must answer what the header's flag rule says; where a call
cannot apply, the refusal -- status and reason word -- is the assertion.  In process: a failure prints the context and the
steps walked so far."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_sequences as ts  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", ts.SEEDS)
def test_trajectory_calls_survive_random_sequences(qoc, oracle, monkeypatch, seed):
    lines = []

    def setenv(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)

    try:
        contexts, checks, drawn = ts.run_seed(qoc, oracle, seed, setenv, lines.append)
    except Exception:
        starts = [i for i, line in enumerate(lines) if line.startswith("context")]
        if starts:                                            # (nothing logged yet: the error itself says where)
            print(f"seed {seed}, context {len(starts) - 1}:")
            print("\n".join(lines[starts[-1]:]))
        raise
    assert contexts == ts.CONTEXTS_PER_SEED and checks == drawn >= contexts
