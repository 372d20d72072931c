"""Plain NumPy / SciPy reference of grape_eval_observables (include/grape_hip.h), shared by test_observe_host.py and
test_gpu_observe.py.  Deliberately NOT the algorithm of observe.hip: propagators from scipy.linalg.expm with H built in the
variant's association (as tests/rc_reference.py), states by a plain loop over the slices -- P X for UnitaryGate, P X P' for
the sandwich types -- and the traces by einsum.  No chunk products, no prefix scan, and no device result enters it.

  y[k, j, s] = tr(O_kj' X_ks) ,  s = 0..N ,  X_k0 = Xi_k
"""
import numpy as np

from rc_reference import propagators


def is_sandwich(sys_type):
    return str(sys_type) != "UnitaryGate"


def states(P, Xi, sandwich):
    """X[s, k]: the state of member k after s slices, s = 0..N.  P (N, E, n, n), Xi (E, n, m)."""
    X = [np.asarray(Xi, complex)]
    for t in range(P.shape[0]):
        Y = P[t] @ X[-1]
        if sandwich:
            Y = Y @ np.conj(np.swapaxes(P[t], -1, -2))
        X.append(Y)
    return np.array(X)


def observables_ref(sys_type, A, B, Xi, x, T, O, per_member=False, variant=0):
    """(y (E, n_obs, N+1), X_final (E, n, m)).  A (E,n,n), B (E,K,n,n), Xi (E,n,m), x (K,N); O (n_obs,n,m) shared by the
    members or, per_member, (E,n_obs,n,m)."""
    A, B, Xi = (np.asarray(v, complex) for v in (A, B, Xi))
    x = np.asarray(x, float)
    X = states(propagators(A, B, x, T, variant), Xi, is_sandwich(sys_type))
    O = np.asarray(O, complex)
    if O.ndim == 2:
        O = O[None]
    if per_member:
        y = np.einsum("kjab,skab->kjs", O.conj(), X)
    else:
        y = np.einsum("jab,skab->kjs", O.conj(), X)
    return y, X[-1]


def member_fom(sys_type, y_N, n):
    """fom_func of the reference from z = tr(Xt' X_N): Re z^2 (UnitaryGate), 1 - |z / n|^2 (the sandwich types)."""
    y_N = np.asarray(y_N, complex)
    if is_sandwich(sys_type):
        return 1.0 - np.abs(y_N / n) ** 2
    return np.real(y_N * y_N)


def matrix_units(n, m):
    """the n m probes E_ab: tr(E_ab' X) = X[a, b], in the order of X.reshape(-1)"""
    O = np.zeros((n * m, n, m), complex)
    for a in range(n):
        for b in range(m):
            O[a * m + b, a, b] = 1.0
    return O
