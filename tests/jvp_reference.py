"""Plain NumPy / SciPy reference of grape_eval_jvp (include/grape_hip.h), shared by test_jvp_host.py and the GPU tests.
Deliberately NOT the algorithm of jvp.hip: propagators from scipy.linalg.expm (tests/rc_reference.py), states by a plain
loop, and the first-order tangent straight from the O(N^2) double sum over (t, s > t) -- no tangent recursion, no chunk
products, no scans.

  xdot (K, N) is a direction in the coordinates of the PHYSICAL pulse;  V_kt = sum_c xdot[c,t] (-i dt B_kc)
  Xdot_ks = sum_{t<s} P_{s-1} .. P_{t+1} V_kt X_{k,t+1} ,   ydot_kjs = tr(O_kj' Xdot_ks) ,   Xdot_final_k = Xdot_kN
No ensemble weight enters.
"""
import numpy as np

from rc_reference import propagators, states
from vjp_reference import probes_per_member


def tangent_states_ref(A, B, Xi, x, xdot, T, variant=0):
    """Xdot (N+1, E, n, m) from the double sum"""
    A, B, Xi = (np.asarray(v, complex) for v in (A, B, Xi))
    x, xdot = np.asarray(x, float), np.asarray(xdot, float)
    N = x.shape[1]
    dt = T / N
    P = propagators(A, B, x, T, variant)
    X = states(P, Xi)
    D = np.zeros_like(X)
    for t in range(N):
        V = (-1j * dt) * np.einsum("c,kcab->kab", xdot[:, t], B)
        Z = V @ X[t + 1]                                          # V_t X_{t+1}
        for s in range(t + 1, N + 1):
            if s > t + 1:
                Z = P[s - 1] @ Z                                  # P_{s-1} .. P_{t+1} V_t X_{t+1}
            D[s] += Z
    return D


def tangent_states_recurrence(A, B, Xi, x, xdot, T, variant=0):
    """The same Xdot from the recurrence of the header (what the kernel evaluates, chunked and scanned):
    Xdot_0 = 0,  Xdot_{s+1} = P_s Xdot_s + V_s X_{s+1}."""
    A, B, Xi = (np.asarray(v, complex) for v in (A, B, Xi))
    x, xdot = np.asarray(x, float), np.asarray(xdot, float)
    N = x.shape[1]
    dt = T / N
    P = propagators(A, B, x, T, variant)
    X = states(P, Xi)
    D = [np.zeros_like(X[0])]
    for s in range(N):
        V = (-1j * dt) * np.einsum("c,kcab->kab", xdot[:, s], B)
        D.append(P[s] @ D[-1] + V @ X[s + 1])
    return np.array(D)


def read_out(D, O, per_member=False):
    """(ydot (E, n_obs, N+1), Xdot_final (E, n, m)) of the tangent states D (N+1, E, n, m); O as observe takes it"""
    Ok = probes_per_member(O, D.shape[1], per_member)
    return np.einsum("kjab,skab->kjs", Ok.conj(), D), D[-1]


def jvp_ref(A, B, Xi, x, xdot, T, O, per_member=False, variant=0):
    """(ydot, Xdot_final) from the double sum.  A (E,n,n), B (E,K,n,n), Xi (E,n,m), x and xdot (K,N)."""
    return read_out(tangent_states_ref(A, B, Xi, x, xdot, T, variant), O, per_member)


def jvp_recurrence(A, B, Xi, x, xdot, T, O, per_member=False, variant=0):
    return read_out(tangent_states_recurrence(A, B, Xi, x, xdot, T, variant), O, per_member)


def pairing(ybar, ydot, xbar, xdot_final):
    """(<(ybar, Xbar), (ydot, Xdot_final)>, the sum of the absolute values of its terms): the real pairing the cotangent
    convention of grape_eval_vjp belongs to; either pair may be None"""
    val = mag = 0.0
    for a, b in ((ybar, ydot), (xbar, xdot_final)):
        if a is not None:
            val += float(np.sum(np.real(np.conj(a) * b)))
            mag += float(np.sum(np.abs(a) * np.abs(b)))
    return val, mag
