"""The exact gradient of the running cost (grape_set_running_cost_derivative) on the host: the NumPy / SciPy reference of
tests/rc_exact_reference.py (expm_frechet per slice, the O(N^2) double sum) against central differences of the running cost
itself, the first-order reference of rc_reference.py missing the same differences by orders of magnitude, the agreement of
the two references in the limit of fine slices, and the plumbing of the setting (engine.py, api.py) on a stand-in engine.
No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rc_exact_reference as rxr  # noqa: E402
import rc_reference as rcr  # noqa: E402
from test_running_cost_host import _ket_problem, _smooth_pulse  # noqa: E402

# n, m, N, T, hermitian, variant, J: n = 2, 3, 4; m < n and m = n; N = 6 .. 12; both kinds of drift; one and three terms
CASES = [
    (2, 1, 6, 1.0, True, 0, 1), (2, 2, 7, 3.0, False, 1, 3), (2, 2, 12, 2.0, True, 1, 3), (2, 1, 9, 2.5, False, 0, 1),
    (3, 1, 8, 1.5, False, 0, 3), (3, 3, 6, 3.0, True, 1, 1), (3, 2, 11, 1.0, False, 1, 3), (3, 1, 12, 2.0, True, 0, 1),
    (4, 1, 7, 2.0, True, 1, 3), (4, 4, 6, 1.0, False, 0, 1), (4, 3, 10, 3.0, True, 0, 3), (4, 2, 12, 1.5, False, 1, 1),
]
E, K = 2, 2
_CACHE = {}


def problem(i):
    n, m, N, T, herm, variant, J = CASES[i]
    rng = np.random.default_rng(9700 + i)
    A, B, Xi, wts = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
    x = rng.standard_normal((K, N))
    R = rng.standard_normal((J, E, n, m)) + 1j * rng.standard_normal((J, E, n, m))
    rho = rng.uniform(0.5, 1.5, (J, N)) * rng.choice([-1.0, 1.0], (J, 1))
    return dict(A=A, B=B, Xi=Xi, wts=wts, x=x, R=R, rho=rho, T=T, variant=variant, K=K, N=N)


def central_differences(c, h=1e-5):
    """dJ/dx entry by entry (the whole gradient: a single direction can hide a wrong gradient behind a cancellation)"""
    fd = np.empty((c["K"], c["N"]))
    for cc in range(c["K"]):
        for t in range(c["N"]):
            d = np.zeros((c["K"], c["N"]))
            d[cc, t] = h
            fd[cc, t] = (rcr.running_cost_value(c["A"], c["B"], c["Xi"], c["wts"], c["x"] + d, c["T"], c["R"], c["rho"], c["variant"]) -
                         rcr.running_cost_value(c["A"], c["B"], c["Xi"], c["wts"], c["x"] - d, c["T"], c["R"], c["rho"], c["variant"])) / (2 * h)
    return fd


def case(i):
    if i not in _CACHE:
        c = problem(i)
        args = (c["A"], c["B"], c["Xi"], c["wts"], c["x"], c["T"], c["R"], c["rho"], c["variant"])
        c["fd"] = central_differences(c)
        c["J_exact"], c["G_exact"] = rxr.rc_exact_ref(*args)
        c["J_first"], c["G_first"] = rcr.running_cost_ref(*args)
        c["J_value"] = rcr.running_cost_value(*args)
        _CACHE[i] = c
    return _CACHE[i]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_exact_reference_agrees_with_central_differences(i):
    """G_J[c,t] against (J(x + h e_ct) - J(x - h e_ct)) / 2h, h = 1e-5: |G - G_fd|_inf <= 1e-6 |G_fd|_inf (the margin covers
    the cancellation error of the differences); J is the value the first-order reference and running_cost_value return"""
    c = case(i)
    dev = np.abs(c["G_exact"] - c["fd"]).max() / np.abs(c["fd"]).max()
    print(f"case {i} {CASES[i]}: exact gradient of J against central differences: relative deviation {dev:.2e}")
    assert dev <= 1e-6, dev
    assert c["J_exact"] == pytest.approx(c["J_value"], rel=1e-13) and c["J_first"] == pytest.approx(c["J_value"], rel=1e-13)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_first_order_reference_misses_the_same_differences(i):
    """the two rules differ, and the check tells which one is right: the first-order gradient deviates from the differences
    by at least 1e-2 of the gradient's norm on every one of these coarse cases"""
    c = case(i)
    dev = np.linalg.norm(c["G_first"] - c["fd"]) / np.linalg.norm(c["fd"])
    print(f"case {i} {CASES[i]}: first-order gradient of J against central differences: relative deviation {dev:.2e}")
    assert dev >= 1e-2, dev


@pytest.mark.parametrize("n,m,hermitian,variant", [(2, 2, True, 0), (3, 1, False, 1), (4, 2, True, 1)])
def test_the_two_references_agree_in_the_limit_of_fine_slices(n, m, hermitian, variant):
    """a smooth pulse and smooth weights at fixed T: per doubling of N the entries of the gradient halve (each slice is half as
    long) and so does the relative first-order error, so |G_first - G_exact|_inf falls by about 4 (within 3 .. 5.5)"""
    rng = np.random.default_rng(41)
    T = 1.5
    A, B, Xi, wts = rcr.random_problem(rng, n, m, K, E, hermitian=hermitian)
    R = rng.standard_normal((2, E, n, m)) + 1j * rng.standard_normal((2, E, n, m))
    diff = []
    for N in (16, 32, 64):
        x = _smooth_pulse(K, N, T)
        ts = (np.arange(N) + 1) * (T / N)
        rho = np.array([1.0 + 0.5 * np.sin(2.0 * ts), -0.8 * np.cos(1.1 * ts)]) * (T / N)
        _, G1 = rcr.running_cost_ref(A, B, Xi, wts, x, T, R, rho, variant)
        _, Gx = rxr.rc_exact_ref(A, B, Xi, wts, x, T, R, rho, variant)
        diff.append(np.abs(G1 - Gx).max())
    print(f"n={n} m={m}: |G_first - G_exact|_inf at N = 16, 32, 64: {diff[0]:.3e} {diff[1]:.3e} {diff[2]:.3e}")
    assert 3.0 <= diff[0] / diff[1] <= 5.5 and 3.0 <= diff[1] / diff[2] <= 5.5, diff


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
class RecordingEngine:
    """stands in for GrapeEngine inside api.make_engine: records the constructor's keywords and the order of the setters"""
    log = None

    def __init__(self, *args, **kw):
        type(self).log.append(("create", kw.get("gradient", 0), kw.get("objective", 0)))

    def set_running_cost_derivative(self, mode):
        type(self).log.append(("mode", mode))

    def set_running_cost(self, R, rho):
        type(self).log.append(("cost", np.asarray(R).shape))

    def close(self):
        type(self).log.append(("close",))


@pytest.fixture
def recorded(qoc, monkeypatch):
    RecordingEngine.log = []
    monkeypatch.setattr(qoc.api, "GrapeEngine", RecordingEngine)
    return RecordingEngine.log


def test_fields_and_defaults(qoc):
    costs = [qoc.EvolutionTime(2.0)]
    assert qoc.GRAPE(n_slices=6).running_cost_derivative == "first_order"
    assert qoc.GRAPE(n_slices=6, running_costs=costs, running_cost_derivative="exact").running_cost_derivative == "exact"
    assert qoc.ADGRAPE(n_slices=6).running_costs is None
    assert qoc.ADGRAPE(n_slices=6, running_costs=costs).running_costs is costs


def test_make_engine_sets_the_mode_before_the_cost(qoc, recorded):
    prob = _ket_problem(qoc)
    costs = [qoc.ForbiddenStates([[0, 0, 1.0]], 0.7), qoc.EvolutionTime(2.0)]
    eng = qoc.api.make_engine(prob, qoc.ADGRAPE(n_slices=6, running_costs=costs))
    assert recorded == [("create", "exact", "c1"), ("mode", "exact"), ("cost", (2, 1, 3, 1))] and eng.running_cost_constant == 2.0
    del recorded[:]
    qoc.api.make_engine(prob, qoc.GRAPE(n_slices=6, running_costs=costs, running_cost_derivative="exact"))
    assert recorded == [("create", 0, 0), ("mode", "exact"), ("cost", (2, 1, 3, 1))]
    del recorded[:]
    qoc.api.make_engine(prob, qoc.GRAPE(n_slices=6, running_costs=costs))     # the default: the setting is never called
    assert recorded == [("create", 0, 0), ("cost", (2, 1, 3, 1))]
    del recorded[:]
    eng = qoc.api.make_engine(prob, qoc.ADGRAPE(n_slices=6))                  # no cost: neither call
    assert recorded == [("create", "exact", "c1")] and eng.running_cost_constant == 0.0
    del recorded[:]
    eng = qoc.api.make_engine(prob, qoc.GRAPE(n_slices=6, running_cost_derivative="exact"))
    assert recorded == [("create", 0, 0)]                                     # a mode without a cost stays a field


def test_a_refused_mode_closes_the_engine(qoc, recorded, monkeypatch):
    def refuse(self, mode):
        raise ValueError("refused")
    monkeypatch.setattr(RecordingEngine, "set_running_cost_derivative", refuse)
    with pytest.raises(ValueError):
        qoc.api.make_engine(_ket_problem(qoc), qoc.ADGRAPE(n_slices=6, running_costs=[qoc.EvolutionTime(1.0)]))
    assert recorded[-1] == ("close",) and ("cost", (1, 1, 3, 1)) not in recorded


def test_fields_survive_save_and_load(qoc, tmp_path):
    prob = _ket_problem(qoc)
    path = os.path.join(tmp_path, "rcx.npz")
    costs = [qoc.ForbiddenStates([[0, 0, 1.0]], 0.7), qoc.EvolutionTime(2.0)]
    alg = qoc.GRAPE(n_slices=6, running_costs=costs, running_cost_derivative="exact")
    qoc.save(qoc.SolutionResult(None, 0.5, np.asarray(prob.guess), prob, alg), path)
    back = qoc.load(path).alg
    assert isinstance(back, qoc.GRAPE) and back.running_cost_derivative == "exact"
    assert [type(c).__name__ for c in back.running_costs] == ["ForbiddenStates", "EvolutionTime"]
    qoc.save(qoc.SolutionResult(None, 0.5, np.asarray(prob.guess), prob, qoc.GRAPE(n_slices=6, running_costs=costs)), path)
    assert qoc.load(path).alg.running_cost_derivative == "first_order"
    qoc.save(qoc.SolutionResult(None, 0.5, np.asarray(prob.guess), prob, qoc.ADGRAPE(n_slices=6, running_costs=costs)), path)
    back = qoc.load(path).alg
    assert isinstance(back, qoc.ADGRAPE) and back.running_costs[1].weight == 2.0 and back.running_costs[0].weight == 0.7
    qoc.save(qoc.SolutionResult(None, 0.5, np.asarray(prob.guess), prob, qoc.ADGRAPE(n_slices=6)), path)
    assert qoc.load(path).alg.running_costs is None


def test_engine_method_checks_the_mode_before_the_library(qoc):
    eng = object.__new__(qoc.GrapeEngine)
    eng._h = None
    eng._rc_derivative = "first_order"
    with pytest.raises(ValueError):
        qoc.GrapeEngine.set_running_cost_derivative(eng, "second_order")
    assert eng.running_cost_derivative == "first_order"


def test_the_symbol_refuses_a_null_context(qoc):
    lib = qoc.load_library()
    assert "grape_set_running_cost_derivative" in qoc.engine.EXPORTS
    assert lib.grape_set_running_cost_derivative(None, C.c_int32(1)) == -1
