"""Plain NumPy / SciPy reference of grape_eval_hvp (include/grape_hip.h), shared by test_hvp_host.py and the GPU tests.
Deliberately NOT the algorithm of hvp.hip: propagators from scipy.linalg.expm (tests/rc_reference.py) and forward-mode
differentiation of vjp_reference.vjp_recurrence -- the same plain loop over the slices on (value, tangent) pairs of matrices
under the rule of the first-order pair, Pdot_s = V_s P_s.  No chunks, no scans.

  xdot (K, N) is a direction in the coordinates of the PHYSICAL pulse;  V_ks = sum_c xdot[c,s] (-i dt B_kc)
  (ybar_dot, xbar_dot) is the tangent of the cotangents (None: zero)
  Gdot[c,t] = sum_k Re tr(Lamd_{k,t+1}' B'_kc X_{k,t+1}) + Re tr(Lam_{k,t+1}' B'_kc Xd_{k,t+1}) ,  returned as its two terms
No ensemble weight enters.
"""
import numpy as np
from scipy.linalg import expm

from rc_reference import propagators
from vjp_reference import probes_per_member


def dagger(M):
    return np.conj(np.swapaxes(M, -1, -2))


def directions(B, xdot, dt):
    """V[s, k] = sum_c xdot[c, s] (-i dt B_kc)"""
    return (-1j * dt) * np.einsum("cs,kcab->skab", np.asarray(xdot, float), np.asarray(B, complex))


def vjp_of_propagators(P, B, Xi, dt, Ok, ybar, xbar):
    """vjp_reference.vjp_recurrence on given propagators P (N, E, n, n): what the difference quotients perturb"""
    N, K = P.shape[0], B.shape[1]
    X = [np.asarray(Xi, complex)]
    for s in range(N):
        X.append(P[s] @ X[-1])
    G = np.zeros((K, N))
    Lam = np.zeros_like(X[0])
    for s in range(N, 0, -1):
        if s < N:
            Lam = dagger(P[s]) @ Lam
        if s == N and xbar is not None:
            Lam = Lam + xbar
        if ybar is not None:
            Lam = Lam + np.einsum("kj,kjam->kam", ybar[:, :, s], Ok)
        G[:, s - 1] = np.real(np.einsum("kam,kcab,kbm->c", Lam.conj(), (-1j * dt) * B, X[s]))
    return G


def _prepare(A, B, Xi, x, T, O, ybar, xbar, ybar_dot, xbar_dot, per_member, variant, P=None):
    A, B, Xi = (np.asarray(v, complex) for v in (A, B, Xi))
    x = np.asarray(x, float)
    cplx = lambda v: None if v is None else np.asarray(v, complex)
    ybar, xbar, ybar_dot, xbar_dot = cplx(ybar), cplx(xbar), cplx(ybar_dot), cplx(xbar_dot)
    Ok = probes_per_member(O, A.shape[0], per_member) if (ybar is not None or ybar_dot is not None) else None
    P = propagators(A, B, x, T, variant) if P is None else P
    return A, B, Xi, x, T / x.shape[1], P, Ok, ybar, xbar, ybar_dot, xbar_dot


def hvp_ref(A, B, Xi, x, xdot, T, O=None, ybar=None, xbar=None, ybar_dot=None, xbar_dot=None, per_member=False, variant=0,
            P=None):
    """(term of Lamd, term of Xd), each (K, N); their sum is Gdot.  A (E,n,n), B (E,K,n,n), Xi (E,n,m), x and xdot (K,N);
    O, ybar (E, n_obs, N+1), xbar (E, n, m) as vjp_recurrence takes them; ybar_dot / xbar_dot likewise, None: zero.
    P: rc_reference.propagators of (A, B, x, T, variant) where the caller has them already."""
    A, B, Xi, x, dt, P, Ok, ybar, xbar, ybd, xbd = _prepare(A, B, Xi, x, T, O, ybar, xbar, ybar_dot, xbar_dot, per_member, variant,
                                                            P)
    K, N = x.shape
    V = directions(B, xdot, dt)
    Pd = V @ P                                                    # the pair's rule: Pdot_s = V_s P_s
    X, Xd = [Xi], [np.zeros_like(Xi)]
    for s in range(N):                                            # (X, Xd) <- (P X, Pdot X + P Xd)
        X.append(P[s] @ X[s])
        Xd.append(Pd[s] @ X[s] + P[s] @ Xd[s])
    t_lam, t_x = np.zeros((K, N)), np.zeros((K, N))
    Lam, Lamd = np.zeros_like(Xi), np.zeros_like(Xi)
    Bp = (-1j * dt) * B
    for s in range(N, 0, -1):
        if s < N:                                                 # (Lam, Lamd) <- (P' Lam, Pdot' Lam + P' Lamd)
            Lam, Lamd = dagger(P[s]) @ Lam, dagger(Pd[s]) @ Lam + dagger(P[s]) @ Lamd
        if s == N and xbar is not None:
            Lam = Lam + xbar
        if s == N and xbd is not None:
            Lamd = Lamd + xbd
        if ybar is not None:
            Lam = Lam + np.einsum("kj,kjam->kam", ybar[:, :, s], Ok)
        if ybd is not None:
            Lamd = Lamd + np.einsum("kj,kjam->kam", ybd[:, :, s], Ok)
        t_lam[:, s - 1] = np.real(np.einsum("kam,kcab,kbm->c", Lamd.conj(), Bp, X[s]))
        t_x[:, s - 1] = np.real(np.einsum("kam,kcab,kbm->c", Lam.conj(), Bp, Xd[s]))
    return t_lam, t_x


def hvp_model_fd(A, B, Xi, x, xdot, T, eps, O=None, ybar=None, xbar=None, ybar_dot=None, xbar_dot=None, per_member=False,
                 variant=0):
    """Gdot by central differences of step eps of the VJP recurrence over P_s(eps) = expm(eps V_s) P_s and the cotangents
    (ybar + eps ybar_dot, xbar + eps xbar_dot): the model grape_eval_hvp differentiates, with the quotient's O(eps^2) error"""
    A, B, Xi, x, dt, P, Ok, ybar, xbar, ybd, xbd = _prepare(A, B, Xi, x, T, O, ybar, xbar, ybar_dot, xbar_dot, per_member, variant)
    V = directions(B, xdot, dt)

    def side(e):
        Pe = np.array([[expm(e * V[s, k]) @ P[s, k] for k in range(P.shape[1])] for s in range(P.shape[0])])
        yb = ybar if ybd is None else (0 if ybar is None else ybar) + e * ybd
        xb = xbar if xbd is None else (0 if xbar is None else xbar) + e * xbd
        return vjp_of_propagators(Pe, B, Xi, dt, Ok, yb, xb)

    return (side(eps) - side(-eps)) / (2.0 * eps)


def hvp_true_fd(A, B, Xi, x, xdot, T, h, O=None, ybar=None, xbar=None, ybar_dot=None, xbar_dot=None, per_member=False, variant=0):
    """Central differences of step h of the VJP recurrence with the pulse perturbed INSIDE expm: the true directional
    derivative of G, which the first-order rule approaches as dt -> 0"""
    A, B, Xi, x, dt, _, Ok, ybar, xbar, ybd, xbd = _prepare(A, B, Xi, x, T, O, ybar, xbar, ybar_dot, xbar_dot, per_member, variant)
    xdot = np.asarray(xdot, float)

    def side(e):
        yb = ybar if ybd is None else (0 if ybar is None else ybar) + e * ybd
        xb = xbar if xbd is None else (0 if xbar is None else xbar) + e * xbd
        return vjp_of_propagators(propagators(A, B, x + e * xdot, T, variant), B, Xi, dt, Ok, yb, xb)

    return (side(h) - side(-h)) / (2.0 * h)
