"""The ensemble-averaged trajectory calls without a GPU: the header and the ctypes prototypes, the NumPy statement of
tests/traj_mean_reference.py against itself (the mean form = the mean of the per-member results, adjointness, the fsum
reference and its bound), the null-context answers of the built library and the default of api.expectation_values."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import observe_reference as obr  # noqa: E402
import rc_reference as rcr  # noqa: E402
import traj_mean_reference as tm  # noqa: E402
import vjp_reference as vr  # noqa: E402
from conftest import ROOT  # noqa: E402

NAMES = ("grape_eval_observables_mean", "grape_eval_vjp_mean", "grape_eval_jvp_mean")


def header():
    hdr = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def prototype(name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header(), flags=re.S)
    assert m, f"{name} is not declared in include/grape_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_three_entry_points():
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", header()).group(1)) == 8       # additive: the version stays
    assert prototype(NAMES[0]) == ["grape_ctx *ctx", "const double *x", "int32_t n_obs", "int32_t per_member", "const double *O",
                                   "const double *v", "double *y_mean", "double *X_mean", "double *F"]
    assert prototype(NAMES[1]) == ["grape_ctx *ctx", "const double *x", "int32_t n_obs", "int32_t per_member", "const double *O",
                                   "const double *v", "const double *ybar_mean", "const double *Xbar_mean", "double *G"]
    assert prototype(NAMES[2]) == ["grape_ctx *ctx", "const double *x", "const double *xdot", "int32_t n_obs", "int32_t per_member",
                                   "const double *O", "const double *v", "double *ydot_mean", "double *Xdot_mean"]
    # host forms only, and the header says so
    for name in NAMES:
        assert not re.search(r"\b%s_device\b" % name, header())
    assert "Host forms ONLY" in open(os.path.join(ROOT, "include", "grape_hip.h")).read()


def test_ctypes_prototypes_mirror_the_header(qoc):
    lib = qoc.load_library()
    for name in NAMES:
        assert name in qoc.engine.EXPORTS
        fn = getattr(lib, name)
        want = [C.c_int32 if a.startswith("int32_t") else C.c_void_p for a in prototype(name)]
        got = [C.c_void_p if t is C.POINTER(C.c_double) else t for t in fn.argtypes]
        assert got == want, name
        assert fn.restype == C.c_int


def test_every_symbol_answers_invalid_arg_to_a_null_context(qoc):
    lib = qoc.load_library()
    assert lib.grape_eval_observables_mean(None, None, 0, 0, None, None, None, None, None) == -1
    assert b"grape_eval_observables_mean" in lib.grape_last_error(None)
    assert lib.grape_eval_vjp_mean(None, None, 0, 0, None, None, None, None, None) == -1
    assert b"grape_eval_vjp_mean" in lib.grape_last_error(None)
    assert lib.grape_eval_jvp_mean(None, None, None, 0, 0, None, None, None, None) == -1
    assert b"grape_eval_jvp_mean" in lib.grape_last_error(None)


def test_expectation_values_keeps_its_default(qoc):
    sig = inspect.signature(qoc.api.expectation_values)
    assert list(sig.parameters)[:3] == ["prob", "pulse", "ops"]
    assert sig.parameters["mean"].default is False
    assert sig.parameters["engine"].default is None
    for name in ("observe_mean", "observe_vjp_mean", "observe_jvp_mean"):
        assert callable(getattr(qoc.GrapeEngine, name))


def problem(per_member, hermitian=False):
    rng = np.random.default_rng(9301 + per_member)
    n, m, K, E, N, T = 3, 2, 2, 5, 9, 1.5
    A, B, Xi, wts = rcr.random_problem(rng, n, m, K, E, hermitian=hermitian)
    x, xdot = rng.standard_normal((K, N)), rng.standard_normal((K, N))
    cplx = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    O = cplx(E, 3, n, m) if per_member else cplx(3, n, m)
    v = rng.standard_normal(E)
    v[1] = 0.0                                                # zero and negative weights are weights
    return dict(A=A, B=B, Xi=Xi, wts=wts, x=x, xdot=xdot, O=O, v=v, T=T, ybar=cplx(3, N + 1), xbar=cplx(n, m))


@pytest.mark.parametrize("per_member", [False, True])
def test_the_mean_form_is_the_mean_of_the_per_member_results(per_member):
    p = problem(per_member)
    y, Xf = obr.observables_ref("UnitaryGate", p["A"], p["B"], p["Xi"], p["x"], p["T"], p["O"], per_member)
    ym, Xm = tm.observables_mean_ref("UnitaryGate", p["A"], p["B"], p["Xi"], p["x"], p["T"], p["O"], p["v"], per_member)
    assert ym.shape == y.shape[1:] and Xm.shape == Xf.shape[1:]
    want = sum(p["v"][k] * y[k] for k in range(len(p["v"])))
    assert np.abs(ym - want).max() <= 1e-14 * np.abs(y).max()
    # the fsum reference and its bound: any order of the E products lies within it
    ref, mag = tm.fsum_mean(p["v"], y)
    tol = tm.fsum_tolerance(len(p["v"]), mag)
    assert tm.within(ym, ref, tol) and tm.within(want, ref, tol)
    back = sum(p["v"][k] * y[k] for k in reversed(range(len(p["v"]))))
    assert tm.within(back, ref, tol)
    assert not tm.within(ref + 4.0 * (tol.real.max() + 1j * tol.imag.max()), ref, tol)         # (the bound binds)
    # one member with weight 1: the member itself
    one, _ = tm.fsum_mean([1.0], y[:1])
    assert np.array_equal(one, y[0])
    # the push-forward: the same sum of the per-member tangents
    yd, Xd = jr.jvp_ref(p["A"], p["B"], p["Xi"], p["x"], p["xdot"], p["T"], p["O"], per_member)
    ydm, Xdm = tm.jvp_mean_ref(p["A"], p["B"], p["Xi"], p["x"], p["xdot"], p["T"], p["O"], p["v"], per_member)
    assert np.abs(ydm - np.tensordot(p["v"], yd, 1)).max() <= 1e-14 * np.abs(yd).max()
    assert np.abs(Xdm - np.tensordot(p["v"], Xd, 1)).max() <= 1e-14 * np.abs(Xd).max()


def test_the_broadcast_cotangent_is_one_rounded_product_per_component():
    p = problem(False)
    yb = tm.broadcast_cotangent(p["v"], p["ybar"])
    assert yb.shape == (5,) + p["ybar"].shape
    for k in range(5):
        assert np.array_equal(yb[k].real, p["v"][k] * p["ybar"].real) and np.array_equal(yb[k].imag, p["v"][k] * p["ybar"].imag)
    assert not yb[1].any() and tm.broadcast_cotangent(p["v"], None) is None


@pytest.mark.parametrize("per_member", [False, True])
def test_adjointness_of_the_mean_pair(per_member):
    """<(ybar, Xbar), J_mean xdot> = <J_mean' (ybar, Xbar), xdot>, both sides from the double-sum references"""
    p = problem(per_member)
    ydm, Xdm = tm.jvp_mean_ref(p["A"], p["B"], p["Xi"], p["x"], p["xdot"], p["T"], p["O"], p["v"], per_member)
    G = tm.vjp_mean_ref(p["A"], p["B"], p["Xi"], p["x"], p["T"], p["O"], p["v"], p["ybar"], p["xbar"], per_member)
    lhs, mag = jr.pairing(p["ybar"], ydm, p["xbar"], Xdm)
    rhs = float(np.sum(G * p["xdot"]))
    assert abs(lhs) > 0 and abs(lhs - rhs) <= 1e-12 * (mag + float(np.sum(np.abs(G * p["xdot"]))))
    # and the pull-back of the mean is the per-member pull-back of the broadcast cotangents, by the recurrence as well
    G2 = vr.vjp_recurrence(p["A"], p["B"], p["Xi"], p["x"], p["T"], p["O"], tm.broadcast_cotangent(p["v"], p["ybar"]),
                           tm.broadcast_cotangent(p["v"], p["xbar"]), per_member)
    assert np.abs(G - G2).max() <= 1e-12 * np.abs(G).max()
