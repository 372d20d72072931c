"""GPU: random walks over the settings that live on a context -- penalties, basis, running cost, the gradient-free figure of
merit -- across re-uploads of operators that flip the data flow (tests/settings_sequences.py draws them,
test_settings_sequences_host.py shows on the CPU what the 24 seeds cover).  Every evaluation, through every entry point, is
held to the composed reference (oracle + penalty_ref + the running cost's double sum, parameter mode in NumPy) at the project's
1e-10 bar; where a setting cannot apply, the refusal is the assertion.  In process: a failure prints the context and the steps
walked so far."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import settings_sequences as ss  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", ss.SEEDS)
def test_settings_survive_random_sequences(qoc, oracle, monkeypatch, seed):
    lines = []

    def setenv(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)

    try:
        contexts, checks = ss.run_seed(qoc, oracle, seed, setenv, lines.append)
    except BaseException:
        start = max(i for i, line in enumerate(lines) if line.startswith("context"))
        print(f"seed {seed}, context {sum(line.startswith('context') for line in lines) - 1}:")
        print("\n".join(lines[start:]))
        raise
    assert contexts == ss.CONTEXTS_PER_SEED and checks >= contexts
