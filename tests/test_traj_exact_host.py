"""The exact derivative mode of the trajectory pull-back / push-forward on the host: the NumPy / SciPy reference of
tests/traj_exact_reference.py (expm_frechet per slice) against central differences of a smooth non-quadratic loss, the
first-order reference failing the same check by orders of magnitude, the transpose pairing of the two exact references, and
the plumbing of the setting (engine.py, autograd.py) on the stand-in engine of test_vjp_host.py.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import rc_reference as rcr  # noqa: E402
import traj_exact_reference as xr  # noqa: E402
import vjp_reference as vr  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_vjp_host import StandInEngine, cplx  # noqa: E402

# n, m, N, T, hermitian, variant: n = 2, 3, 4; m = 1 and n; N = 6 .. 12; T = 1 .. 3; both kinds of drift
CASES = [
    (2, 1, 6, 1.0, True, 0), (2, 2, 7, 3.0, False, 1), (2, 2, 12, 2.0, True, 1), (2, 1, 9, 2.5, False, 0),
    (3, 1, 8, 1.5, False, 0), (3, 3, 6, 3.0, True, 1), (3, 3, 11, 1.0, False, 1), (3, 1, 12, 2.0, True, 0),
    (4, 1, 7, 2.0, True, 1), (4, 4, 6, 1.0, False, 0), (4, 4, 10, 3.0, True, 0), (4, 1, 12, 1.5, False, 1),
]
E, K, J = 2, 2, 3
_CACHE = {}


def case(i):
    """problem, loss cotangents, both pull-backs and the gradient by central differences, entry by entry (the whole gradient:
    a single direction can hide a wrong gradient behind a cancellation in <G, v>) -- once per case"""
    if i not in _CACHE:
        n, m, N, T, herm, variant = CASES[i]
        rng = np.random.default_rng(9100 + i)
        A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
        x, v = rng.standard_normal((K, N)), rng.standard_normal((K, N))
        O = cplx(rng, J, n, m)

        def loss_at(xx):
            y, XN = vr.observe(A, B, Xi, xx, T, O, False, variant)
            return xr.smooth_loss(y, XN)

        _, ybar, xbar = loss_at(x)
        h = 1e-5
        fd = np.empty((K, N))
        for cc in range(K):
            for t in range(N):
                d = np.zeros((K, N))
                d[cc, t] = h
                fd[cc, t] = (loss_at(x + d)[0] - loss_at(x - d)[0]) / (2 * h)
        G_exact = xr.exact_vjp_ref(A, B, Xi, x, T, O, ybar, xbar, False, variant)
        G_first = vr.vjp_ref(A, B, Xi, x, T, O, ybar, xbar, False, variant)
        _CACHE[i] = dict(A=A, B=B, Xi=Xi, x=x, v=v, O=O, T=T, variant=variant, ybar=ybar, xbar=xbar, fd=fd, G_exact=G_exact,
                         G_first=G_first)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_exact_reference_agrees_with_central_differences(i):
    """G[c,t] against (l(x + h e_ct) - l(x - h e_ct)) / 2h, h = 1e-5: |G - G_fd|_inf <= 1e-6 |G_fd|_inf (the margin covers the
    cancellation error of the differences)"""
    c = case(i)
    dev = np.abs(c["G_exact"] - c["fd"]).max() / np.abs(c["fd"]).max()
    print(f"case {i} {CASES[i]}: exact pull-back against central differences: relative deviation {dev:.2e}")
    assert dev <= 1e-6, dev


@pytest.mark.parametrize("i", range(len(CASES)))
def test_first_order_reference_misses_the_same_differences(i):
    """the check discriminates: the first-order pull-back is off by > 1e-2 on every one of these coarse cases"""
    c = case(i)
    dev = np.abs(c["G_first"] - c["fd"]).max() / np.abs(c["fd"]).max()
    print(f"case {i} {CASES[i]}: first-order pull-back against central differences: relative deviation {dev:.2e}")
    assert dev > 1e-2, dev


@pytest.mark.parametrize("i", range(len(CASES)))
def test_exact_references_are_a_transpose_pair(i):
    """<(ybar, Xbar), J xdot> = <J' (ybar, Xbar), xdot> between the exact push-forward and the exact pull-back, 1e-12 relative
    to the sum of the absolute values of the terms"""
    c = case(i)
    rng = np.random.default_rng(9300 + i)
    ybar, xbar = cplx(rng, *c["ybar"].shape), cplx(rng, *c["xbar"].shape)
    xdot = rng.standard_normal(c["x"].shape)
    ydot, xdf = xr.exact_jvp_ref(c["A"], c["B"], c["Xi"], c["x"], xdot, c["T"], c["O"], False, c["variant"])
    G = xr.exact_vjp_ref(c["A"], c["B"], c["Xi"], c["x"], c["T"], c["O"], ybar, xbar, False, c["variant"])
    lhs, mag = jr.pairing(ybar, ydot, xbar, xdf)
    rhs = float(np.sum(G * xdot))
    assert not ydot[:, :, 0].any() and mag > 0
    assert abs(lhs - rhs) <= 1e-12 * mag, (lhs, rhs, mag)


def test_exact_tangent_agrees_with_central_differences_of_the_read_out():
    c = case(4)
    h = 1e-5
    yp, Xp = vr.observe(c["A"], c["B"], c["Xi"], c["x"] + h * c["v"], c["T"], c["O"], False, c["variant"])
    ym, Xm = vr.observe(c["A"], c["B"], c["Xi"], c["x"] - h * c["v"], c["T"], c["O"], False, c["variant"])
    ydot, xdf = xr.exact_jvp_ref(c["A"], c["B"], c["Xi"], c["x"], c["v"], c["T"], c["O"], False, c["variant"])
    assert np.abs(ydot - (yp - ym) / (2 * h)).max() <= 1e-6 * np.abs(ydot).max()
    assert np.abs(xdf - (Xp - Xm) / (2 * h)).max() <= 1e-6 * np.abs(xdf).max()


@pytest.mark.parametrize("n,N,Tc,herm", [(2, 9, 1.5, True), (3, 12, 3.0, False), (4, 7, 24.0, True), (4, 10, 1.0, False)])
def test_eigendecomposition_form_of_the_slice_derivatives_is_expm_frechet(n, N, Tc, herm):
    """the reference switches to slice_derivatives_eig above FRECHET_CALLS_MAX triples: the same numbers to 1e-12"""
    rng = np.random.default_rng(9500 + n)
    A, B, _, _ = rcr.random_problem(rng, n, n, K, E, hermitian=herm)
    x = rng.standard_normal((K, N))
    assert N * E * K <= xr.FRECHET_CALLS_MAX
    P, L = xr.slice_derivatives(A, B, x, Tc, 0)
    Pe, Le = xr.slice_derivatives_eig(A, B, x, Tc, 0)
    assert np.abs(Pe - P).max() <= 1e-12 * np.abs(P).max() and np.abs(Le - L).max() <= 1e-12 * np.abs(L).max()


# ---- the setting's plumbing --------------------------------------------------------------------------------------------------
class StandInExactEngine(StandInEngine):
    """the stand-in engine with GrapeEngine's setting: the mode picks the reference the pull-back / push-forward come from"""
    T = 1.5

    def __init__(self, **kw):
        super().__init__(**kw)
        self.trajectory_derivative = "first_order"

    def set_trajectory_derivative(self, mode):
        if mode not in ("first_order", "exact"):
            raise ValueError(mode)
        self.trajectory_derivative = mode

    def observe_vjp(self, x, ops, ybar=None, xbar_final=None, per_member=False):
        if self.trajectory_derivative == "first_order":
            return super().observe_vjp(x, ops, ybar, xbar_final, per_member)
        return xr.exact_vjp_ref(self.A, self.B, self.Xi, x, self.T, ops, ybar, xbar_final, per_member)

    def observe_jvp(self, x, xdot, ops, per_member=False, final=False):
        f = jr.jvp_ref if self.trajectory_derivative == "first_order" else xr.exact_jvp_ref
        ydot, xdf = f(self.A, self.B, self.Xi, x, xdot, self.T, ops, per_member)
        return (ydot, xdf) if final else ydot


def test_autograd_carries_the_engines_mode_and_gradcheck_needs_exact(qoc):
    import torch
    from quoptimalcontrol_jl_amd import autograd
    eng = StandInExactEngine(n=2, m=2, E=2, K=2, N=6)
    rng = np.random.default_rng(9400)
    ops = cplx(rng, 2, 2, 2)
    x = torch.tensor(rng.standard_normal((2, 6)), dtype=torch.float64, requires_grad=True)

    def f(xx):
        y, XN = autograd.trajectory(eng, xx, ops)
        return y, XN

    assert not torch.autograd.gradcheck(f, (x,), raise_exception=False)       # first order in dt: not the forward's derivative
    eng.set_trajectory_derivative("exact")
    assert torch.autograd.gradcheck(f, (x,))
    assert "gradcheck" in autograd.__doc__ and "set_trajectory_derivative" in autograd.__doc__


def test_engine_exposes_the_setting(qoc):
    eng_mod = qoc.engine
    assert "grape_set_trajectory_derivative" in eng_mod.EXPORTS
    assert eng_mod.TRAJ_DERIVATIVE_CODES == {"first_order": 0, "exact": 1}
    assert callable(qoc.GrapeEngine.set_trajectory_derivative)
    prop = qoc.GrapeEngine.trajectory_derivative
    assert isinstance(prop, property) and prop.fset is None                   # read-only
    header = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    assert re.search(r"GRAPE_TRAJ_FIRST_ORDER = 0, GRAPE_TRAJ_EXACT = 1", header)
    assert "int grape_set_trajectory_derivative(grape_ctx *ctx, int32_t mode);" in header
    assert "GRAPE_ABI_VERSION 8" in header or eng_mod.ABI_VERSION == 8


def test_python_layer_rejects_an_unknown_mode_before_the_library(qoc):
    class Probe(qoc.GrapeEngine):
        def __init__(self):                                                   # no context: the check comes first
            self._h = None
            self._traj_derivative = "first_order"

    p = Probe()
    with pytest.raises(ValueError):
        p.set_trajectory_derivative("second_order")
    assert p.trajectory_derivative == "first_order"
