"""Plain NumPy / SciPy reference of grape_eval_vjp (include/grape_hip.h), shared by test_vjp_host.py and test_gpu_vjp.py.
Deliberately NOT the algorithm of vjp.hip: propagators from scipy.linalg.expm (tests/rc_reference.py), states by a plain
loop, and the first-order gradient straight from the O(N^2) double sum over (t, s > t) -- no costate recursion, no chunk
products, no scans.

  l is a real function of y_kjs = tr(O_kj' X_ks) (s = 0..N) and of X_kN;  ybar = dl/dRe y + i dl/dIm y, Xbar likewise
  G[c,t] = sum_k sum_{s>t} Re( sum_j conj(ybar_kjs) tr(O_kj' Z_s) + [s = N] tr(Xbar_k' Z_N) ) ,
           Z_s = P_{s-1} .. P_{t+1} (-i dt B_kc) X_{k,t+1}
No ensemble weight enters: the caller's loss carries its own.
"""
import numpy as np

from rc_reference import propagators, states


def probes_per_member(O, E, per_member):
    """O (n_obs, n, m) shared, one (n, m) matrix, or (E, n_obs, n, m) -> (E, n_obs, n, m)"""
    O = np.asarray(O, complex)
    if per_member:
        return O
    if O.ndim == 2:
        O = O[None]
    return np.broadcast_to(O, (E,) + O.shape)


def vjp_ref_many(A, B, Xi, x, T, O, ybars=None, xbars=None, variant=0):
    """One pass of the double sum for R cotangent sets at once (G is linear in them): O (E, J, n, m) per member,
    ybars (R, E, J, N+1) and xbars (R, E, n, m), either None.  Returns G (R, K, N)."""
    A, B, Xi = (np.asarray(v, complex) for v in (A, B, Xi))
    x = np.asarray(x, float)
    K, N = x.shape
    dt = T / N
    P = propagators(A, B, x, T, variant)
    X = states(P, Xi)
    yb = None if ybars is None else np.asarray(ybars, complex)
    xb = None if xbars is None else np.asarray(xbars, complex)
    Oc = None if yb is None else np.asarray(O, complex).conj()
    G = np.zeros(((yb if yb is not None else xb).shape[0], K, N))
    for t in range(N):
        Z = (-1j * dt) * np.einsum("kcab,kbm->kcam", B, X[t + 1])     # (-i dt B_c) X_{t+1}
        for s in range(t + 1, N + 1):
            if s > t + 1:
                Z = P[s - 1][:, None] @ Z                             # P_{s-1} .. P_{t+1} (-i dt B_c) X_{t+1}
            if yb is not None:
                tr = np.einsum("kjam,kcam->kjc", Oc, Z)
                G[:, :, t] += np.real(np.einsum("rkj,kjc->rc", yb[:, :, :, s].conj(), tr))
            if xb is not None and s == N:
                G[:, :, t] += np.real(np.einsum("rkam,kcam->rc", xb.conj(), Z))
    return G


def vjp_ref(A, B, Xi, x, T, O=None, ybar=None, xbar=None, per_member=False, variant=0):
    """G (K, N).  A (E,n,n), B (E,K,n,n), Xi (E,n,m), x (K,N); O as observables_ref takes it; ybar (E, n_obs, N+1) and
    xbar (E, n, m) complex, either None."""
    Ok = probes_per_member(O, np.asarray(A).shape[0], per_member) if ybar is not None else None
    return vjp_ref_many(A, B, Xi, x, T, Ok, None if ybar is None else np.asarray(ybar)[None],
                        None if xbar is None else np.asarray(xbar)[None], variant)[0]


def vjp_recurrence(A, B, Xi, x, T, O=None, ybar=None, xbar=None, per_member=False, variant=0):
    """The same G from the costate recurrence of the header (what the kernel evaluates, chunked and scanned):
    Lam_N = Xbar + sum_j ybar[N] O_j,  Lam_s = P_s' Lam_{s+1} + sum_j ybar[s] O_j,  G[c,t] = sum_k Re tr(Lam_{t+1}' (-i dt B_c) X_{t+1})."""
    A, B, Xi = (np.asarray(v, complex) for v in (A, B, Xi))
    x = np.asarray(x, float)
    E, (K, N) = A.shape[0], x.shape
    dt = T / N
    P = propagators(A, B, x, T, variant)
    X = states(P, Xi)
    Ok = probes_per_member(O, E, per_member) if ybar is not None else None
    G = np.zeros((K, N))
    Lam = np.zeros_like(X[0])
    for s in range(N, 0, -1):
        if s < N:
            Lam = np.conj(np.swapaxes(P[s], -1, -2)) @ Lam
        if s == N and xbar is not None:
            Lam = Lam + np.asarray(xbar, complex)
        if ybar is not None:
            Lam = Lam + np.einsum("kj,kjam->kam", np.asarray(ybar, complex)[:, :, s], Ok)
        G[:, s - 1] = np.real(np.einsum("kam,kcab,kbm->c", Lam.conj(), (-1j * dt) * B, X[s]))
    return G


def observe(A, B, Xi, x, T, O, per_member=False, variant=0):
    """(y (E, n_obs, N+1), X_N (E, n, m)) under left multiplication -- the forward the VJP belongs to"""
    A, B, Xi = (np.asarray(v, complex) for v in (A, B, Xi))
    X = states(propagators(A, B, np.asarray(x, float), T, variant), Xi)
    Ok = probes_per_member(O, A.shape[0], per_member)
    return np.einsum("kjab,skab->kjs", Ok.conj(), X), X[-1]
