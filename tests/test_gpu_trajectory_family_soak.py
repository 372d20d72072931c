"""GPU: the family walk -- random walks over the trajectory calls as they are today: grape_eval_vjp_multi, grape_eval_jvp_multi,
grape_eval_hvp, grape_eval_gnvp (host forms, device forms and the d_x = NULL reuse) and the ensemble-averaged host forms,
against each other, against the older trajectory calls and across the settings and operator re-uploads of the older walks
(tests/trajectory_family_sequences.py draws them on top of tests/trajectory_sequences.py; test_trajectory_family_host.py shows
on the CPU what the committed seeds cover and that no mix-up can hide).  Every result is held to the NumPy references at the
project's 1e-10 bar and to every earlier result with the same key bit for bit -- block r of a multi call under the single
call's key, so single, multi, host, device, reuse and forced GRAPE_*_MULTI = 0 / 1 meet in one key --; a reuse call must
answer what the header's flag rule says; where a call cannot apply, the refusal -- status and reason word -- is the assertion.
In process: a failure prints the context and the steps walked so far."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_family_sequences as tf  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", tf.SEEDS)
def test_the_trajectory_family_survives_random_sequences(qoc, oracle, monkeypatch, seed):
    lines = []

    def setenv(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)

    try:
        contexts, checks, drawn = tf.run_seed(qoc, oracle, seed, setenv, lines.append)
    except Exception:
        starts = [i for i, line in enumerate(lines) if line.startswith("context")]
        if starts:                                            # (nothing logged yet: the error itself says where)
            print(f"seed {seed}, context {len(starts) - 1}:")
            print("\n".join(lines[starts[-1]:]))
        raise
    assert contexts == tf.CONTEXTS_PER_SEED and checks == drawn >= contexts
