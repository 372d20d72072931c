"""grape_eval_observables without a GPU: the NumPy / SciPy reference of tests/observe_reference.py pinned to the 50-digit
golden fixtures (every fixture with n <= 4), and the interface (header, binding)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import observe_reference as obr  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_oracle_golden import GOLDEN, load_case  # noqa: E402

SMALL = [p for p in GOLDEN if load_case(p)[0]["n"] <= 4]


def test_every_small_fixture_is_used():
    assert len(SMALL) == 13


@pytest.mark.parametrize("path", SMALL, ids=[os.path.basename(p)[:-5] for p in SMALL])
def test_reference_matches_the_golden_fixtures(path):
    """States of member 0 (N + 1 of them), every member's F_k from y_{k,N} with O = Xt, and the weighted sum, at 1e-12.
    (Measured on the CPU over the 13 fixtures: <= 1.4e-14 in the states, <= 3.6e-15 in member_F.)"""
    c, A, B, Xi, Xt, wts, x, exp, traj = load_case(path)
    n, m = c["n"], Xi.shape[2]
    y, Xf = obr.observables_ref(c["sys_type"], A, B, Xi, x, c["T"], obr.matrix_units(n, m), variant=c["variant"])
    want = traj[1]                                            # member0_states (N + 1, n, m)
    assert want.shape == (c["N"] + 1, n, m)
    got = np.moveaxis(y[0], 0, -1).reshape(c["N"] + 1, n, m)
    dev_x = np.abs(got - want).max()
    assert dev_x <= 1e-12, dev_x
    assert np.abs(Xf[0] - want[-1]).max() <= 1e-12
    yt, _ = obr.observables_ref(c["sys_type"], A, B, Xi, x, c["T"], Xt[:, None], per_member=True, variant=c["variant"])
    Fk = obr.member_fom(c["sys_type"], yt[:, 0, -1], n)
    dev_f = np.abs(Fk - np.array(exp["member_F"])).max()
    print(f"{os.path.basename(path)}: states {dev_x:.2e} member_F {dev_f:.2e}")
    assert dev_f <= 1e-12, dev_f
    assert abs(float(wts @ Fk) - exp["F"]) <= 1e-12


def test_interface_is_declared_and_bound(qoc):
    assert "grape_eval_observables" in qoc.engine.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+grape_eval_observables\s*\(", hdr)
    assert callable(qoc.GrapeEngine.observe) and callable(qoc.test_pulse) and callable(qoc.expectation_values)
