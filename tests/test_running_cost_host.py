"""Running costs on the intermediate states (grape_set_running_cost; C5 / C6 / C7 of src/cost_functions.jl:44-61) without a
GPU: the NumPy reference the GPU tests compare against is pinned to finite differences of its own J, the host functionals
to literal transcriptions of the Julia one-liners, the descriptors to the (R, rho, constant) the header documents, and the
argument rules of GrapeEngine.set_running_cost are checked before any library call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rc_reference as rcr  # noqa: E402


def _smooth_pulse(K, N, T):
    t = (np.arange(N) + 0.5) * (T / N)
    return np.array([0.7 * np.sin(1.3 * t + c) + 0.4 * np.cos(0.6 * t * (c + 1)) for c in range(K)])


def _fd_error(n, m, N, hermitian, variant, seed):
    """relative error of the reference's first-order gradient against central differences of its own J"""
    rng = np.random.default_rng(seed)
    K, E, T = 2, 2, 1.5
    A, B, Xi, wts = rcr.random_problem(rng, n, m, K, E, hermitian=hermitian)
    R = rng.standard_normal((2, E, n, m)) + 1j * rng.standard_normal((2, E, n, m))
    x = _smooth_pulse(K, N, T)
    # weights as smooth functions of time scaled by dt: J approximates the same time integral at every N
    ts = (np.arange(N) + 1) * (T / N)
    rho = np.array([1.0 + 0.5 * np.sin(2.0 * ts), -0.8 * np.cos(1.1 * ts)]) * (T / N)
    J, G = rcr.running_cost_ref(A, B, Xi, wts, x, T, R, rho, variant)
    assert J == pytest.approx(rcr.running_cost_value(A, B, Xi, wts, x, T, R, rho, variant), rel=1e-13)
    h = 1e-6
    G_fd = np.zeros_like(x)
    for c in range(K):
        for t in range(N):
            e = np.zeros_like(x)
            e[c, t] = h
            G_fd[c, t] = (rcr.running_cost_value(A, B, Xi, wts, x + e, T, R, rho, variant) -
                          rcr.running_cost_value(A, B, Xi, wts, x - e, T, R, rho, variant)) / (2 * h)
    return np.abs(G - G_fd).max() / np.abs(G_fd).max()


@pytest.mark.parametrize("n,m,hermitian,variant", [(2, 2, True, 0), (3, 1, False, 1), (4, 2, True, 1)])
def test_reference_gradient_converges_to_finite_differences_at_first_order(n, m, hermitian, variant):
    """The formula and its indexing (rho[s-1] <-> state after s slices, Lam_{t+1} with X_{t+1}): the error of the first-order
    gradient against the finite difference of J falls like dt -- a factor 4 between N and 4N at fixed T, within 2x."""
    e1 = _fd_error(n, m, 12, hermitian, variant, seed=5)
    e4 = _fd_error(n, m, 48, hermitian, variant, seed=5)
    print(f"n={n} m={m}: rel err N=12 {e1:.3e}, N=48 {e4:.3e}, ratio {e1 / e4:.2f}")
    assert e4 > 1e-6                 # what is measured is the O(dt) term, far above the ~1e-9 noise of the central difference
    assert 2.0 <= e1 / e4 <= 8.0


def test_single_weight_pins_the_index_convention():
    """rho with ONE non-zero entry [s-1]: J is that weight times |tr(R' X_s)|^2 with X_s the state after s slices, and the
    gradient vanishes for the slices t >= s."""
    rng = np.random.default_rng(3)
    n, m, K, E, N, T = 3, 3, 2, 1, 5, 1.0
    A, B, Xi, wts = rcr.random_problem(rng, n, m, K, E)
    x = rng.standard_normal((K, N))
    R = rng.standard_normal((1, E, n, m)) + 1j * rng.standard_normal((1, E, n, m))
    X = rcr.states(rcr.propagators(A, B, x, T), Xi)
    for s in (1, 3, 5):
        rho = np.zeros((1, N))
        rho[0, s - 1] = 2.5
        J, G = rcr.running_cost_ref(A, B, Xi, wts, x, T, R, rho)
        assert J == pytest.approx(wts[0] * 2.5 * abs(np.trace(R[0, 0].conj().T @ X[s, 0])) ** 2, rel=1e-13)
        assert np.all(G[:, s:] == 0.0) and np.abs(G[:, :s]).min() > 0.0


def test_c5_c6_c7_match_the_julia_one_liners(qoc):
    rng = np.random.default_rng(11)
    n, N = 3, 4
    psiF = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    psij = [rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(N)]
    # sum(abs2(psiF' * psi) for psi in psij)
    assert qoc.C5(psiF, psij) == pytest.approx(sum(abs(psiF.conj() @ psi) ** 2 for psi in psij), rel=1e-14)
    KT = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    KJ = [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(N)]
    # 1 - 1 / N * sum(abs2(tr(KT' * Kj) / D) for Kj in KJ)
    assert qoc.C6(KT, KJ, N, n) == pytest.approx(1 - 1 / N * sum(abs(np.trace(KT.conj().T @ Kj) / n) ** 2 for Kj in KJ), rel=1e-14)
    # 1 - 1 / N * sum(abs2(tr(psiT * psij)) for psij in psiJ)
    assert qoc.C7(KT, KJ, N) == pytest.approx(1 - 1 / N * sum(abs(np.trace(KT @ Kj)) ** 2 for Kj in KJ), rel=1e-14)
    # pure states: tr(rhoT rho) = |psiT' psi|^2 -- the overlap the device form sums (the one-liner squares it once more)
    a, b = psiF / np.linalg.norm(psiF), psij[0] / np.linalg.norm(psij[0])
    assert np.trace(np.outer(a, a.conj()) @ np.outer(b, b.conj())) == pytest.approx(abs(a.conj() @ b) ** 2, rel=1e-13)
    assert qoc.C7(np.outer(a, a.conj()), [np.outer(b, b.conj())], 1) == pytest.approx(1 - abs(a.conj() @ b) ** 4, rel=1e-13)


def _ket_problem(qoc, n=3, N=6):
    rng = np.random.default_rng(2)
    A, B, Xi, _ = rcr.random_problem(rng, n, 1, 2, 1)
    Xt = np.zeros((n, 1), complex)
    Xt[1, 0] = 1.0
    return qoc.Problem(B=list(B[0]), A=A[0], Xi=Xi[0], Xt=Xt, T=1.0, n_controls=2, guess=rng.standard_normal((2, N)),
                       sys_type=qoc.UnitaryGate())


def test_descriptors_give_the_documented_terms(qoc):
    from quoptimalcontrol_jl_amd.api import running_cost_terms
    prob = _ket_problem(qoc)
    N = 6
    e2 = np.array([0, 0, 1.0])
    R, rho, const = running_cost_terms([prob], [qoc.ForbiddenStates([e2], 0.7)], N)
    assert R.shape == (1, 1, 3, 1) and np.array_equal(R[0, 0, :, 0], e2) and np.array_equal(rho, np.full((1, N), 0.7)) and const == 0.0
    # C7 on kets: R = psiT, rho = -lambda / N, constant lambda
    R, rho, const = running_cost_terms([prob], [qoc.EvolutionTime(2.0)], N)
    assert np.array_equal(R[0, 0], prob.Xt) and np.allclose(rho, -2.0 / N) and const == 2.0
    # C6 on a gate: R = Xt, rho = -lambda / (N D^2); members' own targets; the constant carries the ensemble weights
    gate = qoc.Problem(B=prob.B, A=prob.A, Xi=np.eye(3), Xt=np.diag([1, 1j, -1]), T=1.0, n_controls=2, guess=prob.guess,
                       sys_type=qoc.UnitaryGate())
    ens = qoc.EnsembleProblem(gate, 2, lambda k: gate.A * k, lambda k: gate.B, lambda k: gate.Xi, lambda k: gate.Xt * k, [0.25, 0.5])
    R, rho, const = running_cost_terms(qoc.init_ensemble(ens), [qoc.EvolutionTime(3.0)], N, ens.wts)
    assert R.shape == (1, 2, 3, 3) and np.array_equal(R[0, 1], 2 * gate.Xt) and np.allclose(rho, -3.0 / (N * 9)) and const == pytest.approx(2.25)
    # mixed list: terms are stacked, at most four in all
    R, rho, const = running_cost_terms([prob], [qoc.ForbiddenStates([e2, [1, 0, 0]], 1.0), qoc.EvolutionTime(1.0)], N)
    assert R.shape == (3, 1, 3, 1) and rho.shape == (3, N) and const == 1.0
    with pytest.raises(ValueError):
        running_cost_terms([prob], [qoc.ForbiddenStates(np.eye(3), 1.0), qoc.ForbiddenStates(np.eye(3)[:2], 1.0)], N)
    with pytest.raises(ValueError):
        running_cost_terms([gate], [qoc.ForbiddenStates([e2], 1.0)], N)          # forbidden kets need n x 1 states
    # the value the device form stands for: weight * C5 / C7 of the trajectory
    x = np.asarray(prob.guess)
    A, B, Xi = prob.A[None], np.array(prob.B)[None], np.asarray(prob.Xi)[None]
    X = rcr.states(rcr.propagators(A, B, x, prob.T), Xi)[1:, 0]
    R, rho, const = running_cost_terms([prob], [qoc.ForbiddenStates([e2], 0.7), qoc.EvolutionTime(2.0)], N)
    J = rcr.running_cost_value(A, B, Xi, [1.0], x, prob.T, R, rho) + const
    rhoT = prob.Xt @ prob.Xt.conj().T
    want = 0.7 * qoc.C5(e2, X) + 2.0 * (1 - sum(np.trace(rhoT @ (v @ v.conj().T)).real for v in X) / N)
    assert J == pytest.approx(want, rel=1e-12)


def test_descriptors_survive_save_and_load(qoc, tmp_path):
    prob = _ket_problem(qoc)
    alg = qoc.GRAPE(n_slices=6, running_costs=[qoc.ForbiddenStates([[0, 0, 1.0], [0, 1j, 0]], 0.7), qoc.EvolutionTime(2.0)])
    assert qoc.GRAPE(n_slices=6).running_costs is None
    res = qoc.SolutionResult(None, 0.5, np.asarray(prob.guess), prob, alg)
    path = os.path.join(tmp_path, "rc.npz")
    qoc.save(res, path)
    back = qoc.load(path).alg.running_costs
    assert [type(c).__name__ for c in back] == ["ForbiddenStates", "EvolutionTime"]
    assert np.array_equal(back[0].states, alg.running_costs[0].states) and back[0].weight == 0.7 and back[1].weight == 2.0
    qoc.save(qoc.SolutionResult(None, 0.5, np.asarray(prob.guess), prob, qoc.GRAPE(n_slices=6)), path)
    assert qoc.load(path).alg.running_costs is None


def test_penalty_functionals_still_take_only_c3_and_c4(qoc):
    for f in (qoc.C5, qoc.C6, qoc.C7):
        with pytest.raises(ValueError):
            qoc.PenaltyFunctionals([1.0], [f])


def test_set_running_cost_refuses_a_null_context(qoc):
    lib = qoc.load_library()
    assert "grape_set_running_cost" in qoc.engine.EXPORTS
    assert lib.grape_set_running_cost(None, 0, None, None) == -1
    buf = (C.c_double * 8)(*([1.0] * 8))
    assert lib.grape_set_running_cost(None, 1, buf, buf) == -1


def test_engine_shapes_are_checked_before_the_library(qoc):
    """GrapeEngine.set_running_cost on a handle-less engine: wrong shapes are ValueErrors, no library call."""
    eng = object.__new__(qoc.GrapeEngine)
    eng.E, eng.n, eng.m, eng.N, eng.K = 3, 4, 2, 5, 2
    eng._h = None
    ok_R, ok_rho = np.ones((4, 2)), np.ones(5)
    for R, rho in ((ok_R, None),                                   # R without rho
                   (np.ones((4, 3)), ok_rho),                      # wrong m
                   (np.ones((2, 4, 2)), ok_rho),                   # (E', n, m) with E' != E
                   (np.ones((5, 1, 4, 2)), np.ones((5, 5))),       # five terms
                   (ok_R, np.ones(4)),                             # wrong N
                   (ok_R, np.ones((2, 3, 5))),                     # rho with three axes
                   (np.ones(4), ok_rho)):                          # a vector is not an n x m block
        with pytest.raises(ValueError):
            qoc.GrapeEngine.set_running_cost(eng, R, rho)
