"""Plain NumPy / SciPy reference of the EXACT derivative mode of the trajectory pull-back / push-forward
(grape_set_trajectory_derivative, GRAPE_TRAJ_EXACT; include/grape_hip.h), shared by test_traj_exact_host.py and
test_gpu_traj_exact.py.  Deliberately NOT the algorithm of the kernels: per slice scipy.linalg.expm_frechet (Pade with its
own scaling, the derivative by Al-Mohy / Higham's block recurrences) in the K directions B'_c -- the kernels differentiate a
Taylor polynomial once, in the direction W_t --, states by a plain loop, the pull-back straight from the O(N^2) double sum over
(t, s > t) without a costate, the push-forward by the plain recurrence.

  G_t = -i dt H_t ,  P_t = exp(G_t) ,  L_t[E] = d/de exp(G_t + e E) at e = 0 ,  B'_kc = -i dt B_kc
  pull-back     G[c,t]  = sum_k sum_{s>t} Re( sum_j conj(ybar_kjs) tr(O_kj' Z_s) + [s = N] tr(Xbar_k' Z_N) ) ,
                Z_s     = P_{s-1} .. P_{t+1} L_t[B'_kc] X_{k,t}                      (X_t: the state BEFORE slice t)
  push-forward  D_0 = 0 ,  D_{t+1} = P_t D_t + L_t[V_t] X_t ,  V_t = sum_c xdot[c,t] B'_kc
No ensemble weight enters.
"""
import numpy as np
from scipy.linalg import expm_frechet

from rc_reference import states
from vjp_reference import probes_per_member


def generators(A, B, x, T, variant=0):
    """G[t, k] = -i dt H, H summed in the order of rc_reference.propagators"""
    E, K, n = B.shape[0], B.shape[1], B.shape[2]
    N = x.shape[1]
    dt = T / N
    G = np.empty((N, E, n, n), complex)
    for t in range(N):
        for k in range(E):
            if variant == 0:
                H = np.zeros((n, n), complex)
                for c in range(K):
                    H = H + B[k, c] * x[c, t]
                H = H + A[k]
            else:
                H = A[k].astype(complex)
                for c in range(K):
                    H = H + B[k, c] * x[c, t]
            G[t, k] = -1j * dt * H
    return G


FRECHET_CALLS_MAX = 2500         # expm_frechet takes ~1 ms per call: up to here the per-slice loop stays within seconds


def slice_derivatives_eig(A, B, x, T, variant=0):
    """The same (P, L) for the shapes with tens of thousands of (slice, member, control) triples, where the expm_frechet loop
    takes a quarter of a minute: all slices at once from the eigendecomposition G = V diag(lam) V^-1 (Daleckii-Krein),
        L[E] = V ((V^-1 E V) o Phi) V^-1 ,  Phi_ij = (e^lam_i - e^lam_j) / (lam_i - lam_j) ,  Phi_ii = e^lam_i .
    No polynomial, no scaling and squaring: not the kernels' algorithm either.  test_traj_exact_host.py pins it to
    slice_derivatives (expm_frechet) at 1e-12 on generic generators, which is what the random test problems are."""
    A, B = np.asarray(A, complex), np.asarray(B, complex)
    x = np.asarray(x, float)
    dt = T / x.shape[1]
    G = generators(A, B, x, T, variant)                               # (N, E, n, n)
    lam, V = np.linalg.eig(G)
    Vi = np.linalg.inv(V)
    el = np.exp(lam)
    d = lam[..., :, None] - lam[..., None, :]
    small = np.abs(d) < 1e-9
    Phi = np.where(small, 0.5 * (el[..., :, None] + el[..., None, :]),
                   (el[..., :, None] - el[..., None, :]) / np.where(small, 1.0, d))
    P = (V * el[..., None, :]) @ Vi
    Ed = Vi[:, :, None] @ (-1j * dt * B)[None] @ V[:, :, None]        # (N, E, K, n, n)
    L = V[:, :, None] @ (Ed * Phi[:, :, None]) @ Vi[:, :, None]
    return P, L


def slice_derivatives(A, B, x, T, variant=0):
    """(P (N, E, n, n), L (N, E, K, n, n)): the propagators and their Frechet derivatives in the K control directions"""
    A, B = np.asarray(A, complex), np.asarray(B, complex)
    x = np.asarray(x, float)
    E, K, n = B.shape[0], B.shape[1], B.shape[2]
    N = x.shape[1]
    dt = T / N
    if N * E * K > FRECHET_CALLS_MAX:
        return slice_derivatives_eig(A, B, x, T, variant)
    G = generators(A, B, x, T, variant)
    P = np.empty((N, E, n, n), complex)
    L = np.empty((N, E, K, n, n), complex)
    for t in range(N):
        for k in range(E):
            for c in range(K):
                P[t, k], L[t, k, c] = expm_frechet(G[t, k], -1j * dt * B[k, c])
    return P, L


def exact_vjp_ref_many(A, B, Xi, x, T, O, ybars=None, xbars=None, variant=0, PL=None):
    """One pass of the double sum for R cotangent sets at once (G is linear in them): O (E, J, n, m) per member,
    ybars (R, E, J, N+1) and xbars (R, E, n, m), either None.  Returns G (R, K, N).  PL: slice_derivatives' result, if the
    caller has it."""
    Xi = np.asarray(Xi, complex)
    x = np.asarray(x, float)
    K, N = x.shape
    P, L = PL if PL is not None else slice_derivatives(A, B, x, T, variant)
    X = states(P, Xi)
    yb = None if ybars is None else np.asarray(ybars, complex)
    xb = None if xbars is None else np.asarray(xbars, complex)
    Oc = None if yb is None else np.asarray(O, complex).conj()
    G = np.zeros(((yb if yb is not None else xb).shape[0], K, N))
    for t in range(N):
        Z = np.einsum("kcab,kbm->kcam", L[t], X[t])                   # L_t[B'_c] X_t
        for s in range(t + 1, N + 1):
            if s > t + 1:
                Z = P[s - 1][:, None] @ Z                             # P_{s-1} .. P_{t+1} L_t[B'_c] X_t
            if yb is not None:
                tr = np.einsum("kjam,kcam->kjc", Oc, Z)
                G[:, :, t] += np.real(np.einsum("rkj,kjc->rc", yb[:, :, :, s].conj(), tr))
            if xb is not None and s == N:
                G[:, :, t] += np.real(np.einsum("rkam,kcam->rc", xb.conj(), Z))
    return G


def exact_vjp_ref(A, B, Xi, x, T, O=None, ybar=None, xbar=None, per_member=False, variant=0, PL=None):
    """G (K, N); the arguments of vjp_reference.vjp_ref"""
    Ok = probes_per_member(O, np.asarray(A).shape[0], per_member) if ybar is not None else None
    return exact_vjp_ref_many(A, B, Xi, x, T, Ok, None if ybar is None else np.asarray(ybar)[None],
                              None if xbar is None else np.asarray(xbar)[None], variant, PL)[0]


def exact_tangent_states(A, B, Xi, x, xdot, T, variant=0, PL=None):
    """D (N+1, E, n, m) from the recurrence; L_t[V_t] by linearity from the K derivatives"""
    Xi = np.asarray(Xi, complex)
    x, xdot = np.asarray(x, float), np.asarray(xdot, float)
    N = x.shape[1]
    P, L = PL if PL is not None else slice_derivatives(A, B, x, T, variant)
    X = states(P, Xi)
    D = [np.zeros_like(X[0])]
    for t in range(N):
        Et = np.einsum("c,kcab->kab", xdot[:, t], L[t])
        D.append(P[t] @ D[-1] + Et @ X[t])
    return np.array(D)


def exact_jvp_ref(A, B, Xi, x, xdot, T, O, per_member=False, variant=0, PL=None):
    """(ydot (E, n_obs, N+1), Xdot_final (E, n, m)); the arguments of jvp_reference.jvp_ref"""
    D = exact_tangent_states(A, B, Xi, x, xdot, T, variant, PL)
    Ok = probes_per_member(O, D.shape[1], per_member)
    return np.einsum("kjab,skab->kjs", Ok.conj(), D), D[-1]


def smooth_loss(y, XN):
    """l = sum_j 0.1 cos(Re y + j) + 0.01 |y|^4 over (y, X_N) flattened together: smooth, pole-free, non-quadratic.
    Returns (l, ybar, Xbar) with the cotangents dl/dRe + i dl/dIm."""
    def part(z):
        j = np.arange(z.size).reshape(z.shape) % 7
        val = np.sum(0.1 * np.cos(z.real + j) + 0.01 * np.abs(z) ** 4)
        bar = -0.1 * np.sin(z.real + j) + 0.04 * np.abs(z) ** 2 * z
        return float(val), bar
    ly, ybar = part(np.asarray(y))
    lx, xbar = part(np.asarray(XN))
    return ly + lx, ybar, xbar
