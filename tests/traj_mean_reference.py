"""Plain NumPy statement of the ensemble-averaged trajectory calls (include/grape_hip.h: grape_eval_observables_mean,
grape_eval_vjp_mean, grape_eval_jvp_mean), shared by test_traj_mean_host.py and test_gpu_traj_mean.py.  Built on the
references of the calls they sit on (observe_reference.py, vjp_reference.py, jvp_reference.py): the per-member result first,
then the sum over the members -- not the device's segmented tree, and no device result enters.

  y_mean[j, s] = sum_k v_k y[k, j, s] ,   X_mean = sum_k v_k X_final[k]
  G            = vjp(ybar[k] = v_k ybar_mean, xbar[k] = v_k xbar_mean)
  ydot_mean    = sum_k v_k ydot[k] ,      Xdot_mean = sum_k v_k Xdot_final[k]
"""
import math

import numpy as np

import jvp_reference as jr
import observe_reference as obr
import vjp_reference as vr


def member_sum(v, a):
    """sum_k v[k] a[k] over the leading axis, plain NumPy"""
    v = np.asarray(v, float)
    return np.tensordot(v, np.asarray(a, complex), axes=(0, 0))


def fsum_mean(v, a):
    """(sum_k v[k] a[k] with math.fsum per real component -- the correctly rounded sum of the E rounded products --, and
    sum_k |v[k]| |component of a[k]| per component, what the a-priori error bound of any summation order scales with).
    a (E, ...) complex.  Returns two arrays of a[0]'s shape, the second complex with the two components' magnitudes."""
    v = np.asarray(v, float)
    a = np.asarray(a, complex)
    E = a.shape[0]
    flat = a.reshape(E, -1)
    out = np.empty(flat.shape[1], complex)
    for part in ("real", "imag"):
        prod = v[:, None] * getattr(flat, part)                # E rounded products per component
        getattr(out, part)[:] = [math.fsum(col) for col in prod.T]
    mag = np.abs(v) @ np.abs(flat.real) + 1j * (np.abs(v) @ np.abs(flat.imag))
    return out.reshape(a.shape[1:]), mag.reshape(a.shape[1:])


def fsum_tolerance(E, mag):
    """E 2^-52 sum_k |v_k| |component_k| per component: twice the a-priori first-order bound E u sum |terms| (u = 2^-53) of E
    rounded products and E - 1 rounded additions in ANY order -- derived, not measured"""
    return E * 2.0 ** -52 * mag


def within(got, want, tol):
    """every real component of got - want within its own tolerance (tol complex: the two components' bounds)"""
    d = np.asarray(got) - np.asarray(want)
    return bool(np.all(np.abs(d.real) <= tol.real) and np.all(np.abs(d.imag) <= tol.imag))


def broadcast_cotangent(v, cot):
    """cot (…) -> (E, …) with .real = v_k Re cot, .imag = v_k Im cot: one rounded product per component"""
    if cot is None:
        return None
    v = np.asarray(v, float)
    cot = np.asarray(cot, complex)
    shape = (len(v),) + (1,) * cot.ndim
    out = np.empty((len(v),) + cot.shape, complex)
    out.real = v.reshape(shape) * cot.real
    out.imag = v.reshape(shape) * cot.imag
    return out


def observables_mean_ref(sys_type, A, B, Xi, x, T, O, v, per_member=False, variant=0):
    y, Xf = obr.observables_ref(sys_type, A, B, Xi, x, T, O, per_member, variant)
    return member_sum(v, y), member_sum(v, Xf)


def vjp_mean_ref(A, B, Xi, x, T, O, v, ybar_mean=None, xbar_mean=None, per_member=False, variant=0):
    return vr.vjp_ref(A, B, Xi, x, T, O, broadcast_cotangent(v, ybar_mean), broadcast_cotangent(v, xbar_mean), per_member, variant)


def jvp_mean_ref(A, B, Xi, x, xdot, T, O, v, per_member=False, variant=0):
    yd, Xd = jr.jvp_ref(A, B, Xi, x, xdot, T, O, per_member, variant)
    return member_sum(v, yd), member_sum(v, Xd)
