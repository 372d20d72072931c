"""grape_eval_jvp on the host: the NumPy reference of tests/jvp_reference.py against the tangent recurrence of the header,
against the reference of the pull-back it is the transpose of (the adjoint identity, no finite differences), against central
differences of the read-out (first order in dt), and the forward-mode plumbing of quoptimalcontrol_jl_amd.autograd on a
stand-in engine built from the reference.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import rc_reference as rcr  # noqa: E402
import vjp_reference as vr  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_vjp_host import smooth_pulse  # noqa: E402

T = 1.5


def cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# n, m, N, E, K, J, hermitian, variant, per_member
CASES = [
    (2, 2, 1, 1, 1, 1, True, 0, False),
    (2, 1, 7, 3, 2, 3, False, 1, True),
    (3, 3, 12, 2, 2, 16, True, 1, False),
    (3, 2, 9, 3, 3, 2, False, 0, True),
    (4, 4, 10, 2, 2, 3, True, 0, True),
    (4, 1, 13, 1, 2, 4, False, 1, False),
]


@pytest.mark.parametrize("n,m,N,E,K,J,herm,variant,per_member", CASES)
def test_double_sum_equals_the_recurrence(n, m, N, E, K, J, herm, variant, per_member):
    rng = np.random.default_rng(1000 * n + 100 * m + N)
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
    x, xdot = rng.standard_normal((K, N)), rng.standard_normal((K, N))
    O = cplx(rng, E, J, n, m) if per_member else cplx(rng, J, n, m)
    yd, Xd = jr.jvp_ref(A, B, Xi, x, xdot, T, O, per_member, variant)
    yr, Xr = jr.jvp_recurrence(A, B, Xi, x, xdot, T, O, per_member, variant)
    assert yd.shape == (E, J, N + 1) and Xd.shape == (E, n, m) and np.abs(yd).max() > 0 and np.abs(Xd).max() > 0
    assert not yd[:, :, 0].any()                              # X_0 = Xi does not move
    assert np.abs(yd - yr).max() <= 1e-13 * np.abs(yd).max()
    assert np.abs(Xd - Xr).max() <= 1e-13 * np.abs(Xd).max()


@pytest.mark.parametrize("n,m,N,E,K,J,herm,variant,per_member", [(2, 2, 1, 2, 1, 2, True, 0, False), (3, 2, 23, 3, 2, 3, False, 1, True),
                                                                 (4, 4, 65, 2, 2, 3, True, 0, False), (4, 1, 64, 2, 3, 4, False, 1, True)])
@pytest.mark.parametrize("which", ["ybar", "xbar", "both"])
def test_adjoint_identity_against_the_pull_back_reference(n, m, N, E, K, J, herm, variant, per_member, which):
    """<(ybar, Xbar), J xdot> = <J' (ybar, Xbar), xdot>: both references use the same first-order linearisation, so the two
    sides agree to rounding (measured <= 3e-16 of the scale on these shapes); the bar is 1e-13 of
    sum |G xdot| + sum |ybar ydot| + sum |Xbar Xdot|."""
    rng = np.random.default_rng(7000 + 100 * n + 10 * m + N)
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
    x, xdot = rng.standard_normal((K, N)), rng.standard_normal((K, N))
    O = cplx(rng, E, J, n, m) if per_member else cplx(rng, J, n, m)
    ybar = cplx(rng, E, J, N + 1) if which != "xbar" else None
    xbar = cplx(rng, E, n, m) if which != "ybar" else None
    yd, Xd = jr.jvp_ref(A, B, Xi, x, xdot, T, O, per_member, variant)
    G = vr.vjp_ref(A, B, Xi, x, T, O, ybar, xbar, per_member, variant)
    lhs, mag = jr.pairing(ybar, yd, xbar, Xd)
    rhs, scale = float(np.sum(G * xdot)), float(np.sum(np.abs(G * xdot))) + mag
    print(f"n={n} m={m} N={N} {which}: |lhs - rhs| / scale = {abs(lhs - rhs) / scale:.2e}")
    assert abs(lhs) > 0 and abs(lhs - rhs) <= 1e-13 * scale


@pytest.mark.parametrize("i,n,m,herm,variant", [(0, 2, 2, True, 0), (1, 3, 1, False, 1), (2, 4, 4, True, 1), (3, 4, 2, False, 0),
                                                (4, 3, 3, True, 0)])
def test_first_order_convergence_against_central_differences(i, n, m, herm, variant):
    """The tangent is first order in dt (as grape_eval_vjp): on a smooth pulse, in a smooth direction, its relative
    deviation from the central difference of the read-out -- in max norm over all of ydot, and separately over
    Xdot_final -- falls by >= 3 per 4x in N (first order predicts 4; measured 3.89 - 4.03).  N = 50 and 200 take the O(N^2)
    double sum; N = 800 the recurrence, which test_double_sum_equals_the_recurrence pins to the double sum at 1e-13."""
    E, K, J = 2, 2, 3
    rng = np.random.default_rng(100 + i)
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
    O = cplx(rng, J, n, m)
    dev_y, dev_x = [], []
    for N in (50, 200, 800):
        x, v = smooth_pulse(K, N, 2)
        yd, Xd = (jr.jvp_ref if N <= 200 else jr.jvp_recurrence)(A, B, Xi, x, v, T, O, False, variant)
        h = 1e-5
        yp, Xp = vr.observe(A, B, Xi, x + h * v, T, O, False, variant)
        ym, Xm = vr.observe(A, B, Xi, x - h * v, T, O, False, variant)
        fy, fX = (yp - ym) / (2 * h), (Xp - Xm) / (2 * h)
        dev_y.append(np.abs(yd - fy).max() / np.abs(fy).max())
        dev_x.append(np.abs(Xd - fX).max() / np.abs(fX).max())
    for name, dev in (("ydot", dev_y), ("Xdot_final", dev_x)):
        print(f"problem {i} (n={n} m={m} herm={herm} variant={variant}) {name}: relative deviation {dev[0]:.3e} {dev[1]:.3e} "
              f"{dev[2]:.3e}, ratios {dev[0] / dev[1]:.2f} {dev[1] / dev[2]:.2f}")
        assert dev[0] / dev[1] >= 3.0 and dev[1] / dev[2] >= 3.0, (name, dev)


# ---- torch forward-mode plumbing -----------------------------------------------------------------------------------------
class StandInEngine:
    """observe / observe_vjp / observe_jvp of GrapeEngine from the NumPy references; keeps what observe_jvp returned"""

    def __init__(self, seed=3, n=3, m=2, E=2, K=2, N=6):
        rng = np.random.default_rng(seed)
        self.A, self.B, self.Xi, _ = rcr.random_problem(rng, n, m, K, E)
        self.n, self.m, self.E, self.K, self.N = n, m, E, K, N
        self.jvp_calls = []

    def observe(self, x, ops, per_member=False, final=False, want_F=False):
        y, XN = vr.observe(self.A, self.B, self.Xi, x, T, ops, per_member)
        return (y, XN) if final else y

    def observe_vjp(self, x, ops, ybar=None, xbar_final=None, per_member=False):
        return vr.vjp_ref(self.A, self.B, self.Xi, x, T, ops, ybar, xbar_final, per_member)

    def observe_jvp(self, x, xdot, ops, per_member=False, final=False):
        yd, Xd = jr.jvp_ref(self.A, self.B, self.Xi, x, xdot, T, ops, per_member)
        self.jvp_calls.append((np.array(x), np.array(xdot), final, yd, Xd))
        return (yd, Xd) if final else yd


@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("per_member", [False, True])
def test_forward_ad_tangent_is_observe_jvp(qoc, final, per_member):
    import torch
    import torch.autograd.forward_ad as fwad
    from quoptimalcontrol_jl_amd import autograd
    eng = StandInEngine()
    rng = np.random.default_rng(8)
    ops = cplx(rng, eng.E, 3, eng.n, eng.m) if per_member else cplx(rng, 3, eng.n, eng.m)
    x0, v0 = rng.standard_normal((eng.K, eng.N)), rng.standard_normal((eng.K, eng.N))
    with fwad.dual_level():
        xd = fwad.make_dual(torch.tensor(x0), torch.tensor(v0))
        out = autograd.trajectory(eng, xd, ops, per_member=per_member, final=final)
        y, XN = out if final else (out, None)                 # (a missing output: y alone comes back, with its tangent)
        yp, yt = fwad.unpack_dual(y)
        assert len(eng.jvp_calls) == 1
        got_x, got_v, got_final, yd, Xd = eng.jvp_calls[0]
        assert np.array_equal(got_x, x0) and np.array_equal(got_v, v0) and got_final == final
        assert np.array_equal(yp.numpy(), vr.observe(eng.A, eng.B, eng.Xi, x0, T, ops, per_member)[0])
        assert yt is not None and np.array_equal(yt.numpy(), yd)          # exactly what observe_jvp returned
        if final:
            Xt = fwad.unpack_dual(XN).tangent
            assert Xt is not None and np.array_equal(Xt.numpy(), Xd)
        # the dual number goes on through torch: d/dv of a log-barrier on a population = <its backward gradient, v>
        loss = -torch.log(100.0 - y[:, 0].abs() ** 2).sum()
        lt = fwad.unpack_dual(loss).tangent
    x = torch.tensor(x0, requires_grad=True)
    yb = autograd.trajectory(eng, x, ops, per_member=per_member, final=False)
    (-torch.log(100.0 - yb[:, 0].abs() ** 2).sum()).backward()
    want = float((x.grad * torch.tensor(v0)).sum())
    assert abs(float(lt) - want) <= 1e-12 * float((x.grad.abs() * torch.tensor(v0).abs()).sum())


def test_backward_is_untouched_by_the_jvp(qoc):
    """no dual level: nothing calls observe_jvp, the backward is observe_vjp's as before"""
    import torch
    from quoptimalcontrol_jl_amd import autograd
    eng = StandInEngine()
    rng = np.random.default_rng(9)
    ops = cplx(rng, 2, eng.n, eng.m)
    x0 = rng.standard_normal((eng.K, eng.N))
    x = torch.tensor(x0, requires_grad=True)
    y, XN = autograd.trajectory(eng, x, ops)
    (y.abs() ** 2).sum().backward()
    yn = vr.observe(eng.A, eng.B, eng.Xi, x0, T, ops)[0]
    assert not eng.jvp_calls
    want = vr.vjp_ref(eng.A, eng.B, eng.Xi, x0, T, ops, 2 * yn, None)
    assert np.abs(x.grad.numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_package_import_does_not_pull_torch_in():
    code = ("import sys; sys.path.insert(0, %r); import quoptimalcontrol_jl_amd as q; assert 'torch' not in sys.modules; "
            "assert 'grape_eval_jvp' in q.engine.EXPORTS and 'grape_eval_jvp_device' in q.engine.EXPORTS; "
            "assert hasattr(q.GrapeEngine, 'observe_jvp') and hasattr(q.GrapeEngine, 'observe_jvp_device')" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)
