"""Plain NumPy / SciPy reference of the EXACT gradient of the running cost (grape_set_running_cost_derivative,
GRAPE_TRAJ_EXACT; include/grape_hip.h), shared by test_rc_exact_host.py and test_gpu_rc_exact.py.  Deliberately NOT the
algorithm of running_cost.hip: the states from rc_reference.states, the per-slice derivatives from scipy.linalg.expm_frechet
(traj_exact_reference.slice_derivatives) and the pull-back from traj_exact_reference.exact_vjp_ref_many -- the O(N^2) double
sum over (t, s > t), no costate -- with the probes R and the cotangents of J,

  J = sum_k w_k sum_j sum_{s=1..N} rho[j, s-1] |y_kjs|^2 ,  y_kjs = tr(R_kj' X_ks)
  ybar_kjs = 2 rho[j, s-1] y_kjs ,  ybar_kj0 = 0 ,

one cotangent set per member (the pull-back carries no weight) and the ensemble weights applied outside.
"""
import numpy as np

import traj_exact_reference as xr
from rc_reference import states


def rc_exact_ref(A, B, Xi, wts, x, T, R, rho, variant=0, PL=None):
    """(J, G_J (K, N)).  A (E,n,n), B (E,K,n,n), Xi (E,n,m), R (J,E,n,m), rho (J,N), x (K,N); PL: slice_derivatives' result,
    if the caller has it."""
    A, B, Xi, R = (np.asarray(v, complex) for v in (A, B, Xi, R))
    rho, wts, x = np.asarray(rho, float), np.asarray(wts, float), np.asarray(x, float)
    E = A.shape[0]
    nJ, N = rho.shape
    if PL is None:
        PL = xr.slice_derivatives(A, B, x, T, variant)
    X = states(PL[0], Xi)
    y = np.einsum("jkab,skab->kjs", R.conj(), X[1:])                  # y[k, j, s-1]
    J = float(np.einsum("js,kjs,k->", rho, np.abs(y) ** 2, wts))
    ybars = np.zeros((E, E, nJ, N + 1), complex)                      # set r: member r's cotangents, nothing for the others
    for k in range(E):
        ybars[k, k, :, 1:] = 2.0 * rho * y[k]
    G_members = xr.exact_vjp_ref_many(A, B, Xi, x, T, R.transpose(1, 0, 2, 3), ybars, None, variant, PL)
    return J, np.einsum("k,kct->ct", wts, G_members)
