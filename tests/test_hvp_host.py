"""grape_eval_hvp on the host: the NumPy reference of tests/hvp_reference.py (forward-mode differentiation of the VJP
recurrence under Pdot_s = V_s P_s) against central differences of that recurrence over the same model, against the true
directional derivative of the pull-back (first order in dt), at xdot = 0, and the visibility of both terms of Gdot on every
parity case of the GPU tests.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hvp_cases as hc  # noqa: E402
import hvp_reference as hr  # noqa: E402
import rc_reference as rcr  # noqa: E402
import vjp_reference as vr  # noqa: E402
from test_vjp_host import smooth_pulse  # noqa: E402

T = 1.5


def cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def random_case(n, m, N, herm, E=2, K=2, J=3):
    rng = np.random.default_rng(3000 + 100 * n + 10 * m + N + herm)
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
    return dict(A=A, B=B, Xi=Xi, x=rng.standard_normal((K, N)), xdot=rng.standard_normal((K, N)), O=cplx(rng, J, n, m),
                ybar=cplx(rng, E, J, N + 1), xbar=cplx(rng, E, n, m), ybd=cplx(rng, E, J, N + 1), xbd=cplx(rng, E, n, m))


MODEL_SHAPES = [(3, 2, 8), (3, 2, 32), (3, 2, 128), (4, 4, 16), (2, 1, 5)]


@pytest.mark.parametrize("herm", [True, False])
@pytest.mark.parametrize("n,m,N", MODEL_SHAPES)
def test_reference_is_the_derivative_of_the_vjp_recurrence_under_the_pairs_rule(n, m, N, herm):
    """hvp_ref against central differences of the VJP recurrence over P_s(eps) = expm(eps V_s) P_s.  The only tolerance is
    the quotient's own error, C eps^2 + O(eps^4) (the cotangents enter linearly, so they add none): halving the step twice,
    the deviation has to fall by the quadratic factor each time -- by at least 3 of the ideal 4, which leaves the eps^4 term
    (a quarter of the eps^2 term's relative size at most at these steps) and nothing else.  An error delta of hvp_ref itself
    does not fall, so it fails the second halving as soon as it reaches the size of C (eps / 4)^2, ~1e-7 of |Gdot| at N = 128
    and more at the smaller N."""
    c = random_case(n, m, N, herm)
    args = (c["A"], c["B"], c["Xi"], c["x"], c["xdot"], T)
    kw = dict(O=c["O"], ybar=c["ybar"], xbar=c["xbar"], ybar_dot=c["ybd"], xbar_dot=c["xbd"])
    t_lam, t_x = hr.hvp_ref(*args, **kw)
    Gd = t_lam + t_x
    errs = [np.abs(hr.hvp_model_fd(*args, eps, **kw) - Gd).max() for eps in (0.5, 0.25, 0.125)]
    print(f"n={n} m={m} N={N} herm={herm}: |Gdot|_inf={np.abs(Gd).max():.3e} |fd - ref|_inf at eps = 0.5, 0.25, 0.125: "
          + ", ".join(f"{e:.3e}" for e in errs))
    assert np.abs(Gd).max() > 0 and errs[0] > 0
    assert errs[1] <= errs[0] / 3.0 and errs[2] <= errs[1] / 3.0


def test_the_perturbed_recurrence_is_the_vjp_recurrence():
    c = random_case(3, 2, 9, False)
    G = hr.hvp_model_fd(c["A"], c["B"], c["Xi"], c["x"], c["xdot"], T, 0.5, O=c["O"], ybar=c["ybar"], xbar=c["xbar"])  # (runs)
    P = rcr.propagators(c["A"], c["B"], c["x"], T, 0)
    Ok = vr.probes_per_member(c["O"], 2, False)
    G0 = hr.vjp_of_propagators(P, np.asarray(c["B"], complex), c["Xi"], T / 9, Ok, c["ybar"], c["xbar"])
    assert G.shape == G0.shape and np.array_equal(G0, vr.vjp_recurrence(c["A"], c["B"], c["Xi"], c["x"], T, c["O"], c["ybar"], c["xbar"]))


def smooth_case(N, herm):
    """one physical problem on N slices: a smooth pulse and direction, cotangents that are smooth functions of time with a
    total weight that does not depend on N"""
    n, m, K, E, J = 3, 2, 2, 2, 2
    rng = np.random.default_rng(3500 + herm)
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
    O, xbar, xbd = cplx(rng, J, n, m), cplx(rng, E, n, m), cplx(rng, E, n, m)
    amp = cplx(rng, 2, E, J, 2)
    x, xdot = smooth_pulse(K, N, 0.5)
    tau = np.arange(N + 1) / N
    wave = np.stack([np.cos(2 * np.pi * tau), np.sin(np.pi * tau)], axis=-1)          # (N + 1, 2)
    ybar, ybd = (np.einsum("kjf,sf->kjs", a, wave) / N for a in amp)
    return (A, B, Xi, x, xdot, T), dict(O=O, ybar=ybar, xbar=xbar, ybar_dot=ybd, xbar_dot=xbd)


@pytest.mark.parametrize("herm", [True, False])
def test_first_order_in_dt_against_the_true_directional_derivative(herm):
    """against central differences of the VJP recurrence with the pulse perturbed inside expm (step 1e-4: quotient error ~1e-8
    of |Gdot|, far below the deviations here) the deviation falls by at least 3 per 4x in N"""
    dev = []
    for N in (8, 32, 128):
        args, kw = smooth_case(N, herm)
        Gd = sum(hr.hvp_ref(*args, **kw))
        true = hr.hvp_true_fd(*args, 1e-4, **kw)
        dev.append(np.abs(Gd - true).max() / np.abs(true).max())
    print(f"herm={herm}: |ref - true|_inf / |true|_inf at N = 8, 32, 128: " + ", ".join(f"{d:.3e}" for d in dev))
    assert dev[1] <= dev[0] / 3.0 and dev[2] <= dev[1] / 3.0


@pytest.mark.parametrize("n,m,N", [(3, 2, 8), (4, 4, 16), (2, 1, 5)])
def test_a_zero_direction_is_the_pull_back_of_the_tangent_cotangents(n, m, N):
    c = random_case(n, m, N, False)
    t_lam, t_x = hr.hvp_ref(c["A"], c["B"], c["Xi"], c["x"], np.zeros_like(c["x"]), T, c["O"], c["ybar"], c["xbar"], c["ybd"], c["xbd"])
    G = vr.vjp_recurrence(c["A"], c["B"], c["Xi"], c["x"], T, c["O"], c["ybd"], c["xbd"])
    assert not t_x.any() and np.abs(G).max() > 0
    assert np.abs(t_lam - G).max() <= 1e-13 * np.abs(G).max()


class StandInEngine:
    """observe / observe_vjp / observe_jvp / observe_hvp of GrapeEngine from the NumPy references"""

    def __init__(self, seed=3, n=3, m=2, E=2, K=2, N=6):
        rng = np.random.default_rng(seed)
        self.A, self.B, self.Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=False)
        self.n, self.m, self.E, self.K, self.N = n, m, E, K, N
        self.hvp_calls = 0

    def observe(self, x, ops, per_member=False, final=False, want_F=False):
        y, XN = vr.observe(self.A, self.B, self.Xi, x, T, ops, per_member)
        return (y, XN) if final else y

    def observe_vjp(self, x, ops, ybar=None, xbar_final=None, per_member=False):
        return vr.vjp_recurrence(self.A, self.B, self.Xi, x, T, ops, ybar, xbar_final, per_member)

    def observe_jvp(self, x, xdot, ops, per_member=False, final=False):
        import jvp_reference as jr
        yd, Xd = jr.jvp_recurrence(self.A, self.B, self.Xi, x, xdot, T, ops, per_member)
        return (yd, Xd) if final else yd

    def observe_hvp(self, x, xdot, ops, ybar=None, xbar_final=None, ybar_dot=None, xbar_final_dot=None, per_member=False):
        self.hvp_calls += 1
        return sum(hr.hvp_ref(self.A, self.B, self.Xi, x, xdot, T, ops, ybar, xbar_final, ybar_dot, xbar_final_dot, per_member))


@pytest.mark.parametrize("final", [True, False])
def test_twice_differentiable_trajectory_on_a_stand_in_engine(final):
    """the plumbing of autograd.trajectory(twice=True), no GPU: torch.autograd.functional.hvp and a create_graph backward of a
    quartic loss equal observe_hvp fed with the cotangents and their tangents worked out by hand; twice=False stays once
    differentiable"""
    import torch
    from quoptimalcontrol_jl_amd import autograd
    eng = StandInEngine()
    rng = np.random.default_rng(11)
    ops, Cm = cplx(rng, 2, eng.n, eng.m), cplx(rng, eng.E, eng.n, eng.m)
    x0, v = rng.standard_normal((eng.K, eng.N)), rng.standard_normal((eng.K, eng.N))
    Ct = torch.from_numpy(Cm)

    def loss_of(x, twice):
        out = autograd.trajectory(eng, x, ops, final=final, twice=twice)
        y, XN = out if final else (out, None)
        return (y.abs() ** 4).sum() + (((XN - Ct).abs() ** 4).sum() if final else 0.0)

    _, hv = torch.autograd.functional.hvp(lambda x: loss_of(x, True), torch.tensor(x0), torch.tensor(v))
    assert eng.hvp_calls > 0
    y, XN = eng.observe(x0, ops, final=True)
    yd, Xd = eng.observe_jvp(x0, v, ops, final=True)
    cot = lambda z: 4.0 * np.abs(z) ** 2 * z
    cot_dot = lambda z, zd: 8.0 * np.real(np.conj(z) * zd) * z + 4.0 * np.abs(z) ** 2 * zd
    D = XN - Cm
    want = eng.observe_hvp(x0, v, ops, cot(y), cot(D) if final else None, cot_dot(y, yd), cot_dot(D, Xd) if final else None)
    assert np.abs(hv.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    x = torch.tensor(x0, requires_grad=True)
    (g,) = torch.autograd.grad(loss_of(x, True), x, create_graph=True)
    (hv2,) = torch.autograd.grad((g * torch.tensor(v)).sum(), x)
    assert np.abs(hv2.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    x = torch.tensor(x0, requires_grad=True)
    (g1,) = torch.autograd.grad(loss_of(x, False), x, create_graph=True)
    assert np.array_equal(g1.detach().numpy(), g.detach().numpy()) and not g1.requires_grad
    with pytest.raises(RuntimeError):
        torch.autograd.grad((g1 * torch.tensor(v)).sum(), x)


@pytest.mark.parametrize("row", hc.SHAPES, ids=lambda r: f"{r[0]}x{r[1]}-N{r[2]}-E{r[3]}-{r[6]}")
def test_both_terms_are_visible_on_every_gpu_parity_case(row):
    """a kernel that lost one of the two terms of Gdot must not pass under the parity tolerance: each term is at least 1e-3
    of the sum, on the reference values the GPU tests compare with.  The one exception is a matter of definition, not of size:
    on a single slice without tangent cotangents Lamd_N = Xbar_dot + sum ybar_dot O = 0 is the only costate tangent there is,
    so the Lamd term is exactly zero (and asserted to be)."""
    N = row[2]
    for key, (t_lam, t_x) in hc.shape_reference(row).items():
        total = np.abs(t_lam + t_x).max()
        a, b = np.abs(t_lam).max(), np.abs(t_x).max()
        assert total > 0 and b >= 1e-3 * total, (key, a, b, total)
        if N == 1 and key[0] == "no_dots":
            assert a == 0.0, (key, a)
        else:
            assert a >= 1e-3 * total, (key, a, b, total)
