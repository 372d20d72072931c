"""grape_set_risk without a GPU: both entry points are declared and exported under the unchanged ABI version 8 and refuse a null
context; the NumPy reference of risk_reference.py has the properties the header states -- the mean as beta -> 0, the bounds
sum_k w_k F_k <= F_beta <= W max_k F_k, sum_k p_k = W, invariance under splitting a member -- and, with the exact gradient of
the C1 functional, G_beta = sum_k p_k g_k is the derivative of F_beta (central differences)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import risk_reference as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_risk_entry_points_under_abi_8(qoc):
    hdr = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    assert re.search(r"int grape_set_risk\(grape_ctx \*ctx, double beta\);", hdr)
    assert re.search(r"int grape_get_risk_weights\(grape_ctx \*ctx, double \*p\);", hdr)
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", hdr).group(1)) == 8 == qoc.engine.ABI_VERSION
    assert "grape_set_risk" in qoc.engine.EXPORTS and "grape_get_risk_weights" in qoc.engine.EXPORTS
    assert "chain rule applied to the gradient convention" in hdr
    lib = qoc.load_library()
    assert hasattr(lib, "grape_set_risk") and hasattr(lib, "grape_get_risk_weights")
    jl = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    assert ":grape_set_risk" in jl and ":grape_get_risk_weights" in jl


def test_null_context_is_refused(qoc):
    lib = qoc.load_library()
    p = np.zeros(4)
    assert lib.grape_set_risk(None, 1.0) == -1
    assert b"grape_set_risk" in lib.grape_last_error(None)
    assert lib.grape_set_risk(None, 0.0) == -1
    assert lib.grape_get_risk_weights(None, p.ctypes.data) == -1
    assert lib.grape_get_risk_weights(None, None) == -1


def test_grape_takes_a_risk_and_saves_it(qoc, tmp_path):
    api = qoc.api
    assert api.GRAPE(n_slices=10).risk == 0.0
    alg = api.GRAPE(n_slices=10, risk=4.0)
    w = qoc.workloads.reference_ensemble("StateTransfer", 5, 10, 5.0)
    base = api.Problem(B=list(w.B[0]), A=w.A[0], Xi=w.Xi[0], Xt=w.Xt[0], T=w.T, n_controls=w.K, guess=w.x,
                       sys_type=api.StateTransfer())
    res = api.SolutionResult(None, 0.25, w.x, base, alg)
    path = os.path.join(tmp_path, "risk.npz")
    api.save(res, path)
    back = api.load(path)
    assert back.alg.risk == 4.0 and isinstance(back.alg, api.GRAPE)
    api.save(api.SolutionResult(None, 0.25, w.x, base, api.GRAPE(n_slices=10)), path)
    assert api.load(path).alg.risk == 0.0


@pytest.fixture(scope="module")
def members(oracle):
    """(workload, F_k, g_k) of one small ensemble: computed once, read-only"""
    w = rr.problem(2, 2, 6, 5, "StateTransfer", seed=11)
    foms, grads = rr.members(oracle, w, w.x)
    foms.setflags(write=False)
    grads.setflags(write=False)
    return w, foms, grads


@pytest.mark.parametrize("beta", [1e-9, -1e-9])
def test_small_beta_is_the_weighted_mean(members, beta):
    w, foms, grads = members
    F, G, p = rr.combine(foms, grads, w.wts, beta)
    F0, G0, p0 = rr.combine(foms, grads, w.wts, 0.0)
    assert F0 == float(w.wts @ foms) and np.array_equal(p0, w.wts)
    assert abs(F - F0) <= 1e-7 * abs(F0)
    assert np.abs(G - G0).max() <= 1e-7 * np.abs(G0).max()
    assert np.abs(p - w.wts).max() <= 1e-7 * w.wts.sum()


@pytest.mark.parametrize("beta", [0.5, 6.0, 300.0, -0.5, -3.0, -300.0])
def test_bounds_and_normalisation(members, beta):
    w, foms, grads = members
    on, W = w.wts > 0, w.wts.sum()
    assert (~on).sum() == 1                                   # one member of weight 0: it takes no part
    F, _, p = rr.combine(foms, grads, w.wts, beta)
    mean, eps = float(w.wts @ foms), 1e-14 * W
    if beta > 0:
        assert mean - eps <= F <= W * foms[on].max() + eps
    else:
        assert W * foms[on].min() - eps <= F <= mean + eps
    assert abs(p.sum() - W) <= 1e-14 * W and np.all(p >= 0) and p[~on] == 0.0
    assert np.isfinite(F)


def test_limits_are_the_extreme_members(members):
    w, foms, grads = members
    on, W = w.wts > 0, w.wts.sum()
    for beta, pick in ((1e6, np.argmax), (-1e6, np.argmin)):
        k = np.flatnonzero(on)[pick(foms[on])]
        F, G, p = rr.combine(foms, grads, w.wts, beta)
        assert abs(F - (W * foms[k] + (W / beta) * np.log(w.wts[k] / W))) <= 1e-12 * W
        assert np.count_nonzero(p) == 1 and p[k] == W
        assert np.array_equal(G, W * grads[k])


@pytest.mark.parametrize("beta", [0.5, 6.0, -3.0])
def test_splitting_a_member_changes_nothing(members, beta):
    w, foms, grads = members
    k = int(np.argmax(w.wts))
    f2, g2 = np.append(foms, foms[k]), np.concatenate([grads, grads[k:k + 1]])
    w2 = np.append(w.wts, w.wts[k] / 2)
    w2[k] /= 2
    F, G, p = rr.combine(foms, grads, w.wts, beta)
    F2, G2, p2 = rr.combine(f2, g2, w2, beta)
    assert abs(F2 - F) <= 1e-14 * max(1.0, abs(F))
    assert np.abs(G2 - G).max() <= 1e-14 * max(1.0, np.abs(G).max())
    assert abs(p2[k] + p2[-1] - p[k]) <= 1e-14 * w.wts.sum()


@pytest.mark.parametrize("beta", [4.0, -3.0])
def test_exact_gradient_is_the_derivative_of_the_soft_maximum(oracle, beta):
    """gradient = exact, objective = c1 on the reference (2 x 2 StateTransfer, E = 5, N = 6, K = 2): G_beta against central
    differences of F_beta, step 1e-6, to 1e-6 relative"""
    w = rr.problem(2, 2, 6, 5, "StateTransfer", seed=12)
    F, G, _, _ = rr.risk_reference(oracle, w, w.x, beta, variant=1, exact=True, objective=1)
    h, fd = 1e-6, np.zeros_like(G)
    for c in range(w.K):
        for t in range(w.N):
            xp, xm = w.x.copy(), w.x.copy()
            xp[c, t] += h
            xm[c, t] -= h
            fd[c, t] = (rr.risk_reference(oracle, w, xp, beta, variant=1, exact=True, objective=1)[0] -
                        rr.risk_reference(oracle, w, xm, beta, variant=1, exact=True, objective=1)[0]) / (2 * h)
    err = np.abs(G - fd).max() / np.abs(fd).max()
    print(f"beta = {beta}: F_beta = {F!r}, max |G - fd| / max |fd| = {err:.3e}")
    assert err <= 1e-6
