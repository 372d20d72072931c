"""grape_eval_vjp on the host: the NumPy reference of tests/vjp_reference.py against the costate recurrence of the header,
against the running-cost reference it generalises, against central differences (first order in dt), and the
torch.autograd plumbing of quoptimalcontrol_jl_amd.autograd on a stand-in engine built from the reference.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rc_reference as rcr  # noqa: E402
import vjp_reference as vr  # noqa: E402
from conftest import ROOT  # noqa: E402

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
@pytest.mark.parametrize("which", ["ybar", "xbar", "both"])
def test_double_sum_equals_the_recurrence(n, m, N, E, K, J, herm, variant, per_member, which):
    rng = np.random.default_rng(1000 * n + 100 * m + N)
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
    x = rng.standard_normal((K, N))
    O = cplx(rng, E, J, n, m) if per_member else cplx(rng, J, n, m)
    ybar = cplx(rng, E, J, N + 1) if which != "xbar" else None
    xbar = cplx(rng, E, n, m) if which != "ybar" else None
    G = vr.vjp_ref(A, B, Xi, x, T, O, ybar, xbar, per_member, variant)
    R = vr.vjp_recurrence(A, B, Xi, x, T, O, ybar, xbar, per_member, variant)
    assert G.shape == (K, N) and np.abs(G).max() > 0
    assert np.abs(G - R).max() <= 1e-13 * np.abs(G).max()


def test_ybar_at_s0_contributes_nothing():
    rng = np.random.default_rng(5)
    A, B, Xi, _ = rcr.random_problem(rng, 3, 3, 2, 2)
    x = rng.standard_normal((2, 6))
    ybar = np.zeros((2, 2, 7), complex)
    ybar[:, :, 0] = cplx(rng, 2, 2)
    assert not vr.vjp_ref(A, B, Xi, x, T, cplx(rng, 2, 3, 3), ybar).any()


@pytest.mark.parametrize("n,m,N,E,J,herm,variant", [(2, 2, 9, 3, 1, True, 0), (3, 1, 12, 2, 3, False, 1), (4, 4, 8, 2, 2, True, 1),
                                                    (4, 2, 11, 1, 4, False, 0), (3, 3, 5, 3, 2, True, 0)])
def test_reproduces_the_running_cost_gradient(n, m, N, E, J, herm, variant):
    """l = sum_k w_k sum_j sum_s rho[j, s-1] |y_kjs|^2  has  ybar[k, j, s] = 2 w_k rho[j, s-1] y_kjs  (s >= 1) and Xbar = 0"""
    rng = np.random.default_rng(10 * n + m + N)
    A, B, Xi, wts = rcr.random_problem(rng, n, m, 2, E, hermitian=herm)
    x = rng.standard_normal((2, N))
    R = cplx(rng, J, E, n, m)
    rho = rng.uniform(-1.0, 1.5, (J, N))
    _, GJ = rcr.running_cost_ref(A, B, Xi, wts, x, T, R, rho, variant)
    O = np.swapaxes(R, 0, 1)                                  # (E, J, n, m)
    y, _ = vr.observe(A, B, Xi, x, T, O, True, variant)
    ybar = np.zeros_like(y)
    ybar[:, :, 1:] = 2.0 * wts[:, None, None] * rho[None] * y[:, :, 1:]
    G = vr.vjp_ref(A, B, Xi, x, T, O, ybar, None, True, variant)
    assert np.abs(G - GJ).max() <= 1e-13 * np.abs(GJ).max()


def smooth_pulse(K, N, shift):
    tau = (np.arange(N) + 0.5) / N
    c = np.arange(K)[:, None]
    return np.sin(2 * np.pi * (c + 1) * tau) + 0.3 * c, np.cos(2 * np.pi * (c + shift) * tau)


def nonquadratic_loss(y, XN, C, N):
    """l = sum sin(Re y) (Im y)^2 / N + sum |X_N - C|^4  and its cotangents (dl/dRe + i dl/dIm)"""
    D = XN - C
    loss = float(np.sum(np.sin(y.real) * y.imag ** 2) / N + np.sum(np.abs(D) ** 4))
    ybar = (np.cos(y.real) * y.imag ** 2 + 2j * np.sin(y.real) * y.imag) / N
    return loss, ybar, 4.0 * np.abs(D) ** 2 * D


@pytest.mark.parametrize("i,n,m,herm,variant", [(0, 2, 2, True, 0), (1, 3, 1, False, 1), (2, 4, 4, True, 1), (3, 4, 2, False, 0),
                                                (4, 3, 3, True, 0)])
def test_first_order_convergence_against_central_differences(i, n, m, herm, variant):
    """The gradient is first order in dt (as grad_func! and the running cost): on a smooth pulse, in a smooth direction, the
    relative deviation of <G, v> from the central difference of a non-quadratic loss falls by >= 3 per 4x in N (first order
    predicts 4).  N = 50 and 200 take the O(N^2) double sum; N = 800 (320 000 pair terms) the recurrence, which
    test_double_sum_equals_the_recurrence pins to the double sum at 1e-13."""
    E, K, J = 2, 2, 3
    rng = np.random.default_rng(100 + i)
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
    O = cplx(rng, J, n, m)
    C = cplx(rng, E, n, m)
    dev = []
    for N in (50, 200, 800):
        x, v = smooth_pulse(K, N, 2)

        def loss_at(xx):
            y, XN = vr.observe(A, B, Xi, xx, T, O, False, variant)
            return nonquadratic_loss(y, XN, C, N)

        _, ybar, xbar = loss_at(x)
        G = (vr.vjp_ref if N <= 200 else vr.vjp_recurrence)(A, B, Xi, x, T, O, ybar, xbar, False, variant)
        h = 1e-5
        fd = (loss_at(x + h * v)[0] - loss_at(x - h * v)[0]) / (2 * h)
        dev.append(abs(float(np.sum(G * v)) - fd) / abs(fd))
    print(f"problem {i} (n={n} m={m} herm={herm} variant={variant}): relative deviation {dev[0]:.3e} {dev[1]:.3e} {dev[2]:.3e}, "
          f"ratios {dev[0] / dev[1]:.2f} {dev[1] / dev[2]:.2f}")
    assert dev[0] / dev[1] >= 3.0 and dev[1] / dev[2] >= 3.0, dev


# ---- torch.autograd plumbing ---------------------------------------------------------------------------------------------
class StandInEngine:
    """observe / observe_vjp of GrapeEngine from the NumPy reference; records what the backward was handed"""

    def __init__(self, seed=3, n=3, m=2, E=2, K=2, N=6):
        rng = np.random.default_rng(seed)
        self.A, self.B, self.Xi, _ = rcr.random_problem(rng, n, m, K, E)
        self.n, self.m, self.E, self.K, self.N = n, m, E, K, N
        self.calls = []

    def observe(self, x, ops, per_member=False, final=False, want_F=False):
        y, XN = vr.observe(self.A, self.B, self.Xi, x, T, ops, per_member)
        return (y, XN) if final else y

    def observe_vjp(self, x, ops, ybar=None, xbar_final=None, per_member=False):
        self.calls.append((None if ybar is None else np.array(ybar), None if xbar_final is None else np.array(xbar_final)))
        return vr.vjp_ref(self.A, self.B, self.Xi, x, T, ops, ybar, xbar_final, per_member)


@pytest.mark.parametrize("which", ["both", "y_only", "x_only", "no_final"])
@pytest.mark.parametrize("per_member", [False, True])
def test_autograd_backward_is_observe_vjp_of_the_hand_cotangents(qoc, which, per_member):
    import torch
    from quoptimalcontrol_jl_amd import autograd
    eng = StandInEngine()
    rng = np.random.default_rng(8)
    ops = cplx(rng, eng.E, 3, eng.n, eng.m) if per_member else cplx(rng, 3, eng.n, eng.m)
    C = cplx(rng, eng.E, eng.n, eng.m)
    x0 = rng.standard_normal((eng.K, eng.N))
    x = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    if which == "no_final":
        y = autograd.trajectory(eng, x, ops, per_member=per_member, final=False)
        XN = None
    else:
        y, XN = autograd.trajectory(eng, x, ops, per_member=per_member)
    assert y.dtype == torch.complex128 and y.shape == (eng.E, 3, eng.N + 1)
    yn, XNn = vr.observe(eng.A, eng.B, eng.Xi, x0, T, ops, per_member)
    assert np.array_equal(y.detach().numpy(), yn)
    loss = 0.0
    ybar = xbar = None
    if which != "x_only":                                     # sin(Re y) Im y^2: ybar = cos(Re y) Im y^2 + 2i sin(Re y) Im y
        loss = loss + (torch.sin(y.real) * y.imag ** 2).sum()
        ybar = np.cos(yn.real) * yn.imag ** 2 + 2j * np.sin(yn.real) * yn.imag
    if which in ("both", "x_only"):                           # |X_N - C|^4: Xbar = 4 |D|^2 D
        loss = loss + ((XN - torch.from_numpy(C)).abs() ** 4).sum()
        xbar = 4.0 * np.abs(XNn - C) ** 2 * (XNn - C)
    loss.backward()
    assert len(eng.calls) == 1
    got_y, got_x = eng.calls[0]
    assert (got_y is None) == (ybar is None) and (got_x is None) == (xbar is None)      # a missing cotangent arrives as None
    if ybar is not None:
        assert np.abs(got_y - ybar).max() <= 1e-13 * np.abs(ybar).max()
    if xbar is not None:
        assert np.abs(got_x - xbar).max() <= 1e-13 * np.abs(xbar).max()
    want = vr.vjp_ref(eng.A, eng.B, eng.Xi, x0, T, ops, got_y, got_x, per_member)
    assert np.array_equal(x.grad.numpy(), want)               # exactly what observe_vjp returned for those cotangents
    hand = vr.vjp_ref(eng.A, eng.B, eng.Xi, x0, T, ops, ybar, xbar, per_member)
    assert np.abs(x.grad.numpy() - hand).max() <= 1e-12 * np.abs(hand).max()


def test_autograd_rejects_what_it_cannot_differentiate(qoc):
    import torch
    from quoptimalcontrol_jl_amd import autograd
    eng = StandInEngine()
    ops = np.ones((1, eng.n, eng.m), complex)
    with pytest.raises(TypeError):
        autograd.trajectory(eng, torch.zeros(eng.K, eng.N, dtype=torch.float32), ops)
    with pytest.raises(TypeError):
        autograd.trajectory(eng, np.zeros((eng.K, eng.N)), ops)
    with pytest.raises(ValueError):
        autograd.trajectory(eng, torch.zeros(eng.K, eng.N, dtype=torch.float64), None)


def test_package_import_does_not_pull_torch_in():
    code = ("import sys; sys.path.insert(0, %r); import quoptimalcontrol_jl_amd as q; assert 'torch' not in sys.modules; "
            "assert 'grape_eval_vjp' in q.engine.EXPORTS and hasattr(q.GrapeEngine, 'observe_vjp')" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)
