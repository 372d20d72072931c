"""The control penalties C3 / C4 (src/cost_functions.jl:29-39, 66-69) without a GPU: the C entry point exists and refuses a
null context, the Python functionals give the reference's values, and the closed-form gradient the device adds
(include/grape_hip.h, grape_set_penalties) is the derivative of the penalty."""
import ctypes as C

import numpy as np
import pytest


def penalty_ref(x, amp, var):
    """F_p = sum_c a_c sum_t x^2 + sum_c v_c sum_{t<N-1} (x[c,t+1]-x[c,t])^2 and its closed-form gradient."""
    x = np.asarray(x, dtype=np.float64)
    a = np.zeros(x.shape[0]) if amp is None else np.asarray(amp, dtype=np.float64)
    v = np.zeros(x.shape[0]) if var is None else np.asarray(var, dtype=np.float64)
    d = np.diff(x, axis=1)
    F = float(np.sum(a[:, None] * x ** 2) + np.sum(v[:, None] * d ** 2))
    G = 2 * a[:, None] * x
    G[:, 1:] += 2 * v[:, None] * d          # [t > 0] (x[c,t] - x[c,t-1])
    G[:, :-1] -= 2 * v[:, None] * d         # [t < N-1] (x[c,t+1] - x[c,t])
    return F, G


def test_set_penalties_refuses_a_null_context(qoc):
    lib = qoc.load_library()
    assert lib.grape_set_penalties(None, None, None) == -1
    w = (C.c_double * 2)(1.0, 2.0)
    assert lib.grape_set_penalties(None, w, w) == -1


def test_c3_c4_values_by_hand(qoc):
    u = np.array([[1.0, -2.0, 0.5], [0.0, 3.0, 3.0]])
    assert qoc.C3(u) == 1 + 4 + 0.25 + 9 + 9
    assert qoc.C4(u) == 9 + 6.25 + 9 + 0
    assert qoc.C4(np.array([[1.0, 2.0, 4.0]])) == 1 + 4
    assert qoc.C4(np.array([[7.0]])) == 0.0
    pf = qoc.PenaltyFunctionals([0.5, [1.0, 2.0]], [qoc.C3, qoc.C4])
    assert pf(u) == pytest.approx(0.5 * qoc.C3(u) + 1.0 * (9 + 6.25) + 2.0 * 9)
    amp, var = pf.device_weights(2)
    assert np.array_equal(amp, [0.5, 0.5]) and np.array_equal(var, [1.0, 2.0])
    assert pf(u) == pytest.approx(penalty_ref(u, amp, var)[0])
    assert qoc.PenaltyFunctionals([1.0], [qoc.C4]).device_weights(3)[0] is None
    for bad in (([1.0], [qoc.C1]), ([1.0, 2.0], [qoc.C3, qoc.C3]), ([1.0], [qoc.C3, qoc.C4])):
        with pytest.raises(ValueError):
            qoc.PenaltyFunctionals(*bad)
    with pytest.raises(ValueError):
        qoc.PenaltyFunctionals([[1.0, 2.0, 3.0]], [qoc.C3]).device_weights(2)
    back = qoc.api.PenaltyFunctionals.from_json(pf.to_json())
    assert back(u) == pf(u)


@pytest.mark.parametrize("K,N", [(1, 1), (2, 1), (1, 2), (3, 2), (2, 7)])
def test_closed_form_gradient_matches_finite_differences(K, N):
    rng = np.random.default_rng(K * 10 + N)
    x = rng.standard_normal((K, N))
    amp = rng.uniform(0, 2, K)
    var = rng.uniform(0, 2, K)
    amp[0] = 0.0
    F, G = penalty_ref(x, amp, var)
    h = 1e-6
    G_fd = np.zeros_like(x)
    for c in range(K):
        for t in range(N):
            e = np.zeros_like(x)
            e[c, t] = h
            G_fd[c, t] = (penalty_ref(x + e, amp, var)[0] - penalty_ref(x - e, amp, var)[0]) / (2 * h)
    assert np.abs(G - G_fd).max() <= 1e-7 * max(1.0, np.abs(G).max())
    # the formulas as written in the header, term by term
    F_direct = sum(amp[c] * x[c, t] ** 2 for c in range(K) for t in range(N)) + \
        sum(var[c] * (x[c, t + 1] - x[c, t]) ** 2 for c in range(K) for t in range(N - 1))
    assert F == pytest.approx(F_direct, rel=1e-14, abs=1e-300)


def test_engine_weights_are_checked_before_the_library(qoc):
    """GrapeEngine.set_penalties shapes scalars / vectors; a wrong length is a ValueError (no library call)."""
    eng = object.__new__(qoc.GrapeEngine)
    eng.K = 3
    eng._h = None
    with pytest.raises(ValueError):
        qoc.GrapeEngine.set_penalties(eng, [1.0, 2.0])


def test_grape_and_adgrape_take_penalties(qoc):
    pf = qoc.PenaltyFunctionals([1.0], [qoc.C3])
    assert qoc.GRAPE(n_slices=4, penalties=pf).penalties is pf
    assert qoc.ADGRAPE(n_slices=4, penalties=pf).penalties is pf
    assert qoc.GRAPE(n_slices=4).penalties is None
