"""Plain NumPy / SciPy reference of grape_eval_gnvp (include/grape_hip.h), shared by test_gnvp_host.py and the GPU tests.
Deliberately NOT the algorithm of gnvp.hip: the composition of the repository's own references,
  jvp_reference.jvp_recurrence  ->  the weight blocks  ->  hvp_reference.vjp_of_propagators,
on propagators from scipy.linalg.expm (tests/rc_reference.py).  No chunks, no scans, no stored sources.

  w   the weights of y's entries: (n_obs, N+1) shared or (E, n_obs, N+1) per member (scalar), or behind a leading axis of 3 the
      planes rr, ri, ii of a real symmetric 2x2 block per entry acting on (Re ydot, Im ydot); None: zero
  wf  (E,) the weights of the final states; None: zero
  Gn = J' W J xdot,  (K, N), in the coordinates of the PHYSICAL pulse.  No ensemble weight enters.
gn_dense builds the same operator as a matrix from unit directions through jvp_reference.jvp_ref (the O(N^2) double sum).
"""
import numpy as np

import jvp_reference as jr
from hvp_reference import vjp_of_propagators
from rc_reference import propagators
from vjp_reference import probes_per_member


def weight_planes(w, y_shape, blocks=None):
    """(rr, ri, ii), each broadcastable to y's shape (E, n_obs, N+1), of a weight array in any of the four accepted shapes
    (an array of y's own shape is scalar weights per member, as in GrapeEngine.observe_gnvp)"""
    w = np.asarray(w, float)
    shared, member = tuple(y_shape[1:]), tuple(y_shape)
    if blocks is not True and w.shape in (shared, member):        # scalar weights: rr = ii = w, ri = 0
        return w, np.zeros_like(w), w
    if blocks is not False and w.shape in ((3,) + shared, (3,) + member):
        return w[0], w[1], w[2]
    raise ValueError(f"weights of shape {w.shape} for y of shape {member}")


def apply_weights(w, ydot, blocks=None):
    """c = (w_rr Re ydot + w_ri Im ydot) + i (w_ri Re ydot + w_ii Im ydot): the cotangent of the weighted tangent"""
    rr, ri, ii = weight_planes(w, ydot.shape, blocks)
    return (rr * ydot.real + ri * ydot.imag) + 1j * (ri * ydot.real + ii * ydot.imag)


def gnvp_ref(A, B, Xi, x, xdot, T, O=None, w=None, wf=None, per_member=False, variant=0, P=None, blocks=None):
    """Gn (K, N).  A (E,n,n), B (E,K,n,n), Xi (E,n,m), x and xdot (K,N); O as observe takes it.
    P: rc_reference.propagators of (A, B, x, T, variant) where the caller has them already (the pull-back's)."""
    A, B, Xi = (np.asarray(v, complex) for v in (A, B, Xi))
    x = np.asarray(x, float)
    E, N = A.shape[0], x.shape[1]
    if w is not None:
        ydot, Xd = jr.jvp_recurrence(A, B, Xi, x, xdot, T, O, per_member, variant)
        ybar = apply_weights(w, ydot, blocks)
        Ok = probes_per_member(O, E, per_member)
    else:
        Xd = jr.tangent_states_recurrence(A, B, Xi, x, xdot, T, variant)[-1]
        ybar, Ok = None, None
    xbar = None if wf is None else np.asarray(wf, float)[:, None, None] * Xd
    P = propagators(A, B, x, T, variant) if P is None else P
    return vjp_of_propagators(P, B, Xi, T / N, Ok, ybar, xbar)


def gn_dense(A, B, Xi, x, T, O=None, w=None, wf=None, per_member=False, variant=0, blocks=None):
    """J' W J as a (K N, K N) matrix, index c N + t: J from unit directions through the double sum (jvp_reference.jvp_ref), the
    weight blocks applied to its real and imaginary rows, contracted in the real pairing of grape_eval_vjp's convention"""
    A, B, Xi = (np.asarray(v, complex) for v in (A, B, Xi))
    x = np.asarray(x, float)
    K, N = x.shape
    E = A.shape[0]
    cols_y, cols_x = [], []
    for c in range(K):
        for t in range(N):
            e = np.zeros((K, N))
            e[c, t] = 1.0
            D = jr.tangent_states_ref(A, B, Xi, x, e, T, variant)
            cols_x.append(D[-1])
            cols_y.append(jr.read_out(D, O, per_member)[0] if w is not None else None)
    Q = K * N
    M = np.zeros((Q, Q))
    if w is not None:
        Jy = np.array(cols_y)                                     # (Q, E, n_obs, N+1)
        WJ = np.array([apply_weights(w, col, blocks) for col in Jy])
        M += np.real(np.einsum("pkjs,qkjs->pq", Jy.conj(), WJ))
    if wf is not None:
        Jx = np.array(cols_x)                                     # (Q, E, n, m)
        M += np.real(np.einsum("pkab,k,qkab->pq", Jx.conj(), np.asarray(wf, float), Jx))
    return M
