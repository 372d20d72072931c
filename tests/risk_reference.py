"""grape_set_risk: the NumPy reference the risk tests are held to.  Shared by test_risk_host.py (the functional's properties,
on the CPU) and test_gpu_risk.py (the device against it).  No test functions here, and no device result enters anything.

  soft_max        (F_beta, p) of per-member values F_k and weights w_k, straight from the header's formulas with a
                  max-shifted log-sum-exp:  W = sum w,  M = max_{w_k > 0} beta F_k,  S = sum_k w_k exp(beta F_k - M),
                  F_beta = (W / beta)(M + log(S / W)),  p_k = W w_k exp(beta F_k - M) / S
  risk_reference  per-member (F_k, g_k) from oracle.ensemble_eval / ensemble_exact (per_member=True) -> soft_max ->
                  G_beta = sum_k p_k g_k -> + settings_sequences.penalty_ref
  composed        the same between a basis / bounds in NumPy, as bounds_sequences.bounded_reference lays them around the
                  evaluation: expand -> saturate -> risk_reference -> slope -> project
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_sequences as bs  # noqa: E402
import settings_sequences as ss  # noqa: E402


def soft_max(foms, wts, beta):
    """(F_beta, p); beta = 0: the weighted mean and p = w"""
    foms, wts = np.asarray(foms, dtype=np.float64), np.asarray(wts, dtype=np.float64)
    W = wts.sum()
    if beta == 0.0:
        return float(wts @ foms), wts.copy()
    on = wts > 0
    M = np.max(beta * foms[on])
    e = np.zeros_like(foms)
    e[on] = wts[on] * np.exp(beta * foms[on] - M)
    S = e.sum()
    return float((W / beta) * (M + np.log(S / W))), W * e / S


def members(oracle, w, x, variant=0, exact=False, objective=0):
    """the oracle's unweighted (F_k (E,), g_k (E, K, N)) of a workload-like object at the pulse x"""
    if exact:
        _, _, foms, grads = oracle.ensemble_exact(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, x, w.T, variant=variant,
                                                  objective=objective, per_member=True)
    else:
        _, _, foms, grads = oracle.ensemble_eval(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, x, w.T, variant=variant,
                                                 per_member=True)
    return np.asarray(foms), np.asarray(grads)


def combine(foms, grads, wts, beta, x=None, penalties=None):
    """(F, G, p) of per-member results: the risk-weighted sum, then the penalties of the pulse x"""
    F, p = soft_max(foms, wts, beta)
    G = np.tensordot(p, grads, axes=1)
    if penalties is not None:
        Fp, Gp = ss.penalty_ref(x, *penalties)
        F, G = F + Fp, G + Gp
    return F, G, p


def risk_reference(oracle, w, x, beta, variant=0, exact=False, objective=0, penalties=None):
    """(F, G, p, F_k) at the physical pulse x (K, N); penalties: (amp, var) or None"""
    foms, grads = members(oracle, w, x, variant, exact, objective)
    F, G, p = combine(foms, grads, w.wts, beta, x, penalties)
    return F, G, p, foms


def composed(oracle, w, theta, beta, variant=0, penalties=None, phi=None, x0=None, bounds=None):
    """(F, G in the space of theta, p, x) with a basis phi (N, M) [+ offset x0] and bounds (lo, hi) around the evaluation"""
    a = np.asarray(theta, dtype=np.float64)
    if phi is not None:
        a = a @ phi.T
        if x0 is not None:
            a = x0 + a
    x, s = bs.sat(a, *bounds) if bounds is not None else (a, np.ones_like(a))
    F, G, p, _ = risk_reference(oracle, w, x, beta, variant, penalties=penalties)
    G = G * s
    if phi is not None:
        G = G @ phi
    return F, G, p, x


def problem(n, K, N, E, sys_type, seed, hermitian=True, T=1.3, zero_weight=True):
    """a small random ensemble (the operators of test_gpu_fom.random_problem): unequal weights, one of them 0 when E > 1"""
    from types import SimpleNamespace
    rng = np.random.default_rng(seed)

    def gen(scale):
        M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        H = (M + M.conj().T) / 2
        if not hermitian:                                     # a damping part: the generators are no longer Hermitian
            D = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
            H = H - 0.15j * (D @ D.conj().T) / n
        return H * scale * min(1.0, 2.0 / n)
    A = np.array([gen(1.0) for _ in range(E)])
    B = np.array([[gen(0.5) for _ in range(K)] for _ in range(E)])
    if sys_type == "UnitaryGate":
        Xi = np.array([np.eye(n, dtype=complex)] * E)
        Xt = np.array([np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0] for _ in range(E)])
    else:
        def rho():
            v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
            v /= np.linalg.norm(v)
            return np.outer(v, v.conj())
        Xi = np.array([rho() for _ in range(E)])
        Xt = np.array([rho() for _ in range(E)])
    wts = rng.uniform(0.2, 1.7, E)
    if zero_weight and E > 1:
        wts[int(rng.integers(0, E))] = 0.0
    return SimpleNamespace(name="risk", sys_type=sys_type, n=n, K=K, N=N, E=E, T=T, A=A, B=B, Xi=Xi, Xt=Xt, wts=wts,
                           x=rng.uniform(-1, 1, (K, N)))
