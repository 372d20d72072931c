"""Plain NumPy / SciPy reference of the running cost of grape_set_running_cost (include/grape_hip.h), shared by
test_running_cost_host.py and test_gpu_running_cost.py.  Deliberately NOT the algorithm of running_cost.hip: propagators
from scipy.linalg.expm, states by a plain loop, and the first-order gradient straight from the O(N^2) double sum over
(t, s > t) -- no costate recursion.

  J          = sum_k w_k sum_j sum_{s=1..N} rho[j, s-1] |y_kjs|^2 ,   y_kjs = tr(R_kj' X_ks)
  dJ/dx[c,t] ~ sum_k w_k sum_j sum_{s>t} rho[j, s-1] 2 Re( conj(y_kjs) tr(R_kj' P_{s-1} .. P_{t+1} (-i dt B_kc) X_{k,t+1}) )
"""
import numpy as np
from scipy.linalg import expm


def propagators(A, B, x, T, variant=0):
    """P[t, k] = exp(-i dt H), H = (sum_c B_kc x[c,t]) + A_k (variant 0) or A_k + sum_c B_kc x[c,t] (variant 1)."""
    E, K, n = B.shape[0], B.shape[1], B.shape[2]
    N = x.shape[1]
    dt = T / N
    P = np.empty((N, E, n, n), complex)
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
            P[t, k] = expm(-1j * dt * H)
    return P


def states(P, Xi):
    """X[s, k] = state of member k after s slices, s = 0..N."""
    X = [np.asarray(Xi, complex)]
    for t in range(P.shape[0]):
        X.append(P[t] @ X[-1])
    return np.array(X)


def running_cost_value(A, B, Xi, wts, x, T, R, rho, variant=0):
    X = states(propagators(A, B, x, T, variant), Xi)
    y = np.einsum("jkab,skab->jsk", R.conj(), X[1:])
    return float(np.einsum("js,jsk,k->", rho, np.abs(y) ** 2, np.asarray(wts, float)))


def running_cost_ref(A, B, Xi, wts, x, T, R, rho, variant=0):
    """(J, G_J (K, N)).  A (E,n,n), B (E,K,n,n), Xi (E,n,m), R (J,E,n,m), rho (J,N), x (K,N)."""
    A, B, Xi, R = (np.asarray(v, complex) for v in (A, B, Xi, R))
    rho, wts, x = np.asarray(rho, float), np.asarray(wts, float), np.asarray(x, float)
    K, N = x.shape
    dt = T / N
    P = propagators(A, B, x, T, variant)
    X = states(P, Xi)
    y = np.einsum("jkab,skab->jsk", R.conj(), X[1:])                  # y[j, s-1, k]
    J = float(np.einsum("js,jsk,k->", rho, np.abs(y) ** 2, wts))
    G = np.zeros((K, N))
    for t in range(N):
        Z = (-1j * dt) * np.einsum("kcab,kbm->kcam", B, X[t + 1])     # (-i dt B_c) X_{t+1}
        for s in range(t + 1, N + 1):
            if s > t + 1:
                Z = P[s - 1][:, None] @ Z                             # P_{s-1} .. P_{t+1} (-i dt B_c) X_{t+1}
            tr = np.einsum("jkam,kcam->jkc", R.conj(), Z)
            G[:, t] += 2.0 * np.real(np.einsum("j,jk,jkc,k->c", rho[:, s - 1], y[:, s - 1].conj(), tr, wts))
    return J, G


def random_problem(rng, n, m, K, E, hermitian=True, scale=1.0):
    """Random drift / controls (Hermitian, or with an anti-Hermitian damping part: the general flow), Xi = m columns of a
    random unitary, weights of order 1 / E."""
    def herm():
        M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        return scale * (M + M.conj().T) / 2
    A = np.array([herm() for _ in range(E)])
    B = np.array([[herm() for _ in range(K)] for _ in range(E)])
    if not hermitian:
        for k in range(E):
            D = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
            A[k] = A[k] - 0.05j * scale * (D @ D.conj().T)
    Q = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0]
    Xi = np.array([Q[:, :m] for _ in range(E)])
    wts = rng.uniform(0.5, 1.5, E) / E
    return A, B, Xi, wts


def perturbed_target(A, B, Xi, x, T, rng, variant=0):
    """Xt_k = the propagation of Xi_k under a perturbed pulse: a target a finite distance away from every state of x."""
    xp = x + 0.3 * rng.standard_normal(x.shape)
    return states(propagators(A, B, xp, T, variant), Xi)[-1]
