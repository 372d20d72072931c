"""grape_eval_hvp on the GPU: the directional derivative of the trajectory pull-back against the NumPy / SciPy reference of
tests/hvp_reference.py (expm per slice, forward-mode differentiation of the VJP recurrence by a plain loop -- no chunks, no
scans) at the project's parity bar relative to |ref|_inf; the zero direction against the shipped pull-back; exact scaling;
its invariants, coordinates, refusals, and torch's double backward end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hvp_cases as hc  # noqa: E402
import hvp_reference as hr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_vjp import invariant_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5
cplx = hc.cplx


def close(a, ref, what):
    amax = np.abs(ref).max()
    err = np.abs(np.asarray(a) - ref).max()
    print(f"{what}: |a-ref|_inf={err:.3e} |ref|_inf={amax:.3e}")
    assert amax > 0 and err <= PARITY_RTOL * amax, f"{what}: |a-ref|_inf={err:.3e} > {PARITY_RTOL * amax:.3e}"


# ---- 1: parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W,J,rho_kind", SHAPES)
def test_parity_against_the_forward_mode_reference(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, J, rho_kind):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, d = hc.shape_problem(n, m, N, E, herm, variant)
    ref = hc.shape_reference((n, m, N, E, herm, variant))
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        for (way, n_obs, pm), (t_lam, t_x) in ref.items():
            ops, yb, xb, ybd, xbd = hc.call_arguments(d, way, n_obs, pm)
            Gd = eng.observe_hvp(c["x"], d["xdot"], ops, ybar=yb, xbar_final=xb, ybar_dot=ybd, xbar_final_dot=xbd, per_member=bool(pm))
            assert Gd.shape == (c["K"], N)
            close(Gd, t_lam + t_x, f"n={n} m={m} N={N} E={E} {kernel} {way} n_obs={n_obs} per_member={pm}")
            names = eng.kernel_names()
            assert "trajectory_hvp_kernel" in names and "vjp_sum_kernel" in names and "trajectory_vjp_kernel" not in names, names


# ---- 2: the zero direction, scaling -------------------------------------------------------------------------------------------
CASES3 = [(3, 2, 23, 2, False, "lane", 2, 0), (4, 4, 65, 3, True, "pair", 1, 3), (2, 2, 130, 5, True, "lane", 0, 0)]


def small_problem(n, m, N, E, herm):
    c = make_case(6300 + n, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(6301)
    return c, dict(O=cplx(rng, 3, n, m), xdot=rng.standard_normal((c["K"], N)), ybar=cplx(rng, E, 3, N + 1), xbar=cplx(rng, E, n, m),
                   ybd=cplx(rng, E, 3, N + 1), xbd=cplx(rng, E, n, m))


@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", CASES3)
def test_a_zero_direction_is_the_pull_back_of_the_tangent_cotangents(qoc, monkeypatch, n, m, N, E, herm, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, d = small_problem(n, m, N, E, herm)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        Gd = eng.observe_hvp(c["x"], np.zeros_like(c["x"]), d["O"], d["ybar"], d["xbar"], d["ybd"], d["xbd"])
        G = eng.observe_vjp(c["x"], d["O"], ybar=d["ybd"], xbar_final=d["xbd"])
        Gx = eng.observe_hvp(c["x"], np.zeros_like(c["x"]), d["O"], d["ybar"], None, None, d["xbd"])       # mixed NULLs
        Gv = eng.observe_vjp(c["x"], None, xbar_final=d["xbd"])
        G0 = eng.observe_hvp(c["x"], np.zeros_like(c["x"]), d["O"], d["ybar"], d["xbar"])
    close(Gd, G, f"n={n} m={m} N={N} {kernel}: xdot = 0")
    close(Gx, Gv, f"n={n} m={m} N={N} {kernel}: xdot = 0, ybar with Xbar_dot")
    assert not G0.any()                                       # nothing moves: exactly zero


@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", CASES3)
def test_scaling_is_exact(qoc, monkeypatch, n, m, N, E, herm, kernel, S, W):
    """every operation is linear in (xdot, ybar_dot, Xbar_dot) and a power of two commutes with rounding"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, d = small_problem(n, m, N, E, herm)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        f = lambda s: eng.observe_hvp(c["x"], s * d["xdot"], d["O"], d["ybar"], d["xbar"], s * d["ybd"], s * d["xbd"])
        G1, G2, Gm = f(1.0), f(2.0), f(-1.0)
    assert np.abs(G1).max() > 0
    assert np.array_equal(G2, 2.0 * G1) and np.array_equal(Gm, -G1)


# ---- 3: invariants -------------------------------------------------------------------------------------------------------------
def hvp_case(herm=False, E=10):
    c, O, yb, xb = invariant_case(herm, E)
    rng = np.random.default_rng(6401)
    return c, O, yb, xb, rng.standard_normal((c["K"], c["N"])), cplx(rng, *yb.shape), cplx(rng, *xb.shape)


def test_bitwise_call_to_call_and_eval_hvp_eval(qoc):
    c, O, yb, xb, xdot, ybd, xbd = hvp_case()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        Ga = eng.observe_hvp(c["x"], xdot, O, yb, xb, ybd, xbd)
        assert "trajectory_hvp_kernel" in eng.kernel_names()
        F1, G1 = eng.eval(c["x"])
        assert eng.kernel_names() == names0 and "trajectory_hvp_kernel" not in names0
        Gb = eng.observe_hvp(c["x"], xdot, O, yb, xb, ybd, xbd)
        Go = eng.observe_hvp(-c["x"], xdot, O, yb, xb, ybd, xbd)          # another call in between
        Gc = eng.observe_hvp(c["x"], xdot, O, yb, xb, ybd, xbd)
    assert F1 == F0 and np.array_equal(G1, G0)
    assert np.array_equal(Ga, Gb) and np.array_equal(Ga, Gc) and not np.array_equal(Ga, Go)


@pytest.mark.parametrize("herm,E,members", [(False, 10, 4), (True, 10, 4), (True, 70, 24)])
def test_member_chunked_context_is_bitwise_the_unchunked_one(qoc, monkeypatch, herm, E, members):
    c, O, yb, xb, xdot, ybd, xbd = hvp_case(herm, E)
    with engine(qoc, c) as eng:
        Gd = eng.observe_hvp(c["x"], xdot, O, yb, xb, ybd, xbd)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, herm, members)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < E and eng.info["member_chunk"] % 32 != 0, eng.info["member_chunk"]
        Gc = eng.observe_hvp(c["x"], xdot, O, yb, xb, ybd, xbd)
    assert np.array_equal(Gc, Gd)


@pytest.mark.parametrize("standing", ["running_cost", "penalties", "risk"])
def test_standing_costs_do_not_enter(qoc, standing):
    c, O, yb, xb, xdot, ybd, xbd = hvp_case()
    with engine(qoc, c) as eng:
        Gd = eng.observe_hvp(c["x"], xdot, O, yb, xb, ybd, xbd)
        F0, _ = eng.eval(c["x"])
        if standing == "running_cost":
            eng.set_running_cost(c["R"], c["rho"])
        elif standing == "penalties":
            eng.set_penalties(np.array([0.3, 0.1]), np.array([0.05, 0.2]))
        else:
            eng.set_risk(2.0)
        F1, _ = eng.eval(c["x"])
        Gs = eng.observe_hvp(c["x"], xdot, O, yb, xb, ybd, xbd)
        F2, _ = eng.eval(c["x"])
    assert F1 != F0 and F2 == F1                              # the cost is in force, before and after
    assert np.array_equal(Gs, Gd)


# ---- 4: coordinates --------------------------------------------------------------------------------------------------------------
def test_basis_direction_expanded_and_result_projected(qoc):
    """Gdot under a basis = the reference's physical Gdot along thetadot phi', projected onto phi"""
    c = make_case(6501, 4, 2, 50, 3, hermitian=False)
    N, K, E = c["N"], c["K"], c["E"]
    rng = np.random.default_rng(6502)
    O, yb, xb, ybd, xbd = cplx(rng, 2, 4, 2), cplx(rng, E, 2, N + 1), cplx(rng, E, 4, 2), cplx(rng, E, 2, N + 1), cplx(rng, E, 4, 2)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    x0 = 0.2 * rng.standard_normal((K, N))
    theta, thetadot = 0.4 * rng.standard_normal((K, 5)), rng.standard_normal((K, 5))
    with engine(qoc, c) as eng:
        eng.set_basis(phi, x0)
        Gd = eng.observe_hvp(theta, thetadot, O, yb, xb, ybd, xbd)
        names = eng.kernel_names()
    assert Gd.shape == (K, 5)
    assert "basis_expand_kernel" in names and "basis_project_kernel" in names and "trajectory_hvp_kernel" in names, names
    t_lam, t_x = hr.hvp_ref(c["A"], c["B"], c["Xi"], x0 + theta @ phi.T, thetadot @ phi.T, T, O, yb, xb, ybd, xbd, False, c["variant"])
    close(Gd, (t_lam + t_x) @ phi, "basis: Gdot")


# ---- 5: refusals and arguments -----------------------------------------------------------------------------------------------
def raw_call(qoc, eng, x, xdot, n_obs, per_member, O, ybar, Xbar, ybd, Xbd, Gdot):
    lib = qoc.load_library()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.grape_eval_hvp(eng._h, ptr(x), ptr(xdot), n_obs, per_member, ptr(O), ptr(ybar), ptr(Xbar), ptr(ybd), ptr(Xbd), ptr(Gdot))
    return rc, lib.grape_last_error(eng._h).decode()


def test_refusals(qoc):
    c = make_case(6601, 4, 4, 20, 2)
    GE = qoc.GrapeError

    def refused(eng, case, word, x=None):
        x = case["x"] if x is None else x
        F0, G0 = eng.eval(x)                                  # the bits from before the refusal
        with pytest.raises(GE) as ei:
            eng.observe_hvp(x, np.ones_like(x), None, xbar_final=np.ones((case["E"], case["n"], case["m"]), complex))
        assert ei.value.status == -2 and word in str(ei.value) and "grape_eval_hvp" in str(ei.value), str(ei.value)
        F, G = eng.eval(x)
        assert F == F0 and np.array_equal(G, G0)

    for nbad in (5, 1):
        big = make_case(6602 + nbad, nbad, nbad, 8, 1)
        with engine(qoc, big) as eng:
            refused(eng, big, "dimension")
    for sys_type in ("StateTransfer", "CoherenceTransfer"):
        with qoc.GrapeEngine(sys_type, c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], T, 20) as eng:
            refused(eng, c, "StateTransfer")
    with engine(qoc, c, gradient="exact") as eng:
        refused(eng, c, "exact")
    with engine(qoc, c, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM) as eng:
        refused(eng, c, "multi-device")
    with engine(qoc, c, force_collective=True) as eng:
        refused(eng, c, "communicator")
    # the two refusals of this call alone
    with engine(qoc, c) as eng:
        eng.set_bounds(np.array([-0.8, -0.5]), np.array([0.9, 0.6]))
        refused(eng, c, "bounds", 0.3 * c["x"])
        eng.set_bounds(None, None)
        eng.set_trajectory_derivative("exact")
        refused(eng, c, "trajectory_derivative")
        eng.set_trajectory_derivative("first_order")
        assert eng.observe_hvp(c["x"], np.ones_like(c["x"]), None, xbar_final=np.ones((2, 4, 4), complex)).any()


def test_invalid_arguments(qoc):
    c = make_case(6701, 4, 4, 20, 2)
    E, N, K = c["E"], c["N"], c["K"]
    rng = np.random.default_rng(6702)
    O = cplx(rng, 2, 4, 4)
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])

        def same_bits():
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)

        xf = np.ascontiguousarray(c["x"].T)
        xdf = np.ascontiguousarray(rng.standard_normal((N, K)))
        Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
        yb, Xb, ybd, Xbd = cplx(rng, E, 2, N + 1), cplx(rng, E, 4, 4), cplx(rng, E, 2, N + 1), cplx(rng, E, 4, 4)
        Gd = np.empty((N, K))
        bad_args = [
            (None, xdf, 2, 0, Of, yb, Xb, ybd, Xbd, Gd),      # null x
            (xf, None, 2, 0, Of, yb, Xb, ybd, Xbd, Gd),       # null xdot
            (xf, xdf, 2, 0, Of, yb, Xb, ybd, Xbd, None),      # null Gdot
            (xf, xdf, 2, 0, Of, None, None, ybd, Xbd, Gd),    # ybar and Xbar_final both NULL (the tangents do not stand in)
            (xf, xdf, -1, 0, Of, yb, Xb, ybd, Xbd, Gd), (xf, xdf, 17, 0, Of, yb, Xb, ybd, Xbd, Gd),     # n_obs outside 0..16
            (xf, xdf, 0, 0, Of, yb, Xb, None, Xbd, Gd),       # n_obs = 0 with a non-NULL ybar
            (xf, xdf, 0, 0, Of, None, Xb, ybd, Xbd, Gd),      # n_obs = 0 with a non-NULL ybar_dot
            (xf, xdf, 2, 0, None, yb, Xb, ybd, Xbd, Gd),      # n_obs > 0 with a NULL O
            (xf, xdf, 2, 2, Of, yb, Xb, ybd, Xbd, Gd), (xf, xdf, 2, -1, Of, yb, Xb, ybd, Xbd, Gd),      # per_member other than 0 or 1
        ]
        for args in bad_args:
            rc, msg = raw_call(qoc, eng, *args)
            assert rc == -1 and "grape_eval_hvp" in msg, (rc, msg)
            same_bits()
        names = ["O[", "xdot[", "ybar[", "Xbar_final[", "ybar_dot[", "Xbar_final_dot["]
        for which in range(6):                                # a non-finite entry of every host array
            arrs = [Of.copy(), xdf.copy(), yb.copy(), Xb.copy(), ybd.copy(), Xbd.copy()]
            arrs[which].reshape(-1)[5] = [np.nan, np.inf][which % 2]
            rc, msg = raw_call(qoc, eng, xf, arrs[1], 2, 0, arrs[0], arrs[2], arrs[3], arrs[4], arrs[5], Gd)
            assert rc == -1 and "not finite" in msg and names[which] in msg, (rc, msg)
            same_bits()
        # every valid NULL combination: (ybar, Xbar) x (ybar_dot, Xbar_dot), and Xbar alone with n_obs = 0
        for ya, xa in ((yb, Xb), (yb, None), (None, Xb)):
            for yd_, xd_ in ((ybd, Xbd), (ybd, None), (None, Xbd), (None, None)):
                rc, msg = raw_call(qoc, eng, xf, xdf, 2, 0, Of, ya, xa, yd_, xd_, Gd)
                assert rc == 0, msg
        for xd_ in (Xbd, None):
            rc, msg = raw_call(qoc, eng, xf, xdf, 0, 0, None, None, Xb, None, xd_, Gd)
            assert rc == 0, msg
        same_bits()
        # the Python layer catches wrong shapes before the library is called
        for call in (lambda: eng.observe_hvp(c["x"], xdf.T[:, :5], O, yb), lambda: eng.observe_hvp(c["x"][:, :5], xdf.T, O, yb),
                     lambda: eng.observe_hvp(c["x"], xdf.T, O), lambda: eng.observe_hvp(c["x"], xdf.T, None, yb),
                     lambda: eng.observe_hvp(c["x"], xdf.T, O, yb[:, :1]), lambda: eng.observe_hvp(c["x"], xdf.T, O, yb, ybar_dot=ybd[:1]),
                     lambda: eng.observe_hvp(c["x"], xdf.T, O, yb, xbar_final_dot=Xbd[:, :3])):
            with pytest.raises(ValueError):
                call()
    # before grape_set_operators
    lib = qoc.load_library()
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.grape_eval_hvp(h, p(xf), p(xdf), 2, 0, p(Of), p(yb), None, None, None, p(Gd)) == -5
        assert b"operators not set" in lib.grape_last_error(h)
    finally:
        lib.grape_destroy(h)


# ---- 6: torch, end to end --------------------------------------------------------------------------------------------------------
def test_torch_hvp_of_a_quartic_loss_through_trajectory(qoc):
    """l = sum |y|^4 / N + sum |X_N - C|^4: torch.autograd.functional.hvp through trajectory(twice=True) against observe_hvp
    fed with the cotangents and their tangents worked out by hand,
      ybar = 4 |y|^2 y / N ,  ybar_dot = (8 Re(conj(y) ydot) y + 4 |y|^2 ydot) / N   (and likewise for D = X_N - C)"""
    import torch
    from quoptimalcontrol_jl_amd import autograd
    N = 40
    c = make_case(6801, 3, 2, N, 2, hermitian=False)
    rng = np.random.default_rng(6802)
    ops, Cm, v = cplx(rng, 2, 3, 2), cplx(rng, 2, 3, 2), rng.standard_normal(c["x"].shape)
    Ct = torch.from_numpy(Cm)

    def loss_of(x, eng, twice):
        y, XN = autograd.trajectory(eng, x, ops, twice=twice)
        return (y.abs() ** 4).sum() / N + ((XN - Ct).abs() ** 4).sum()

    with engine(qoc, c) as eng:
        _, hv = torch.autograd.functional.hvp(lambda x: loss_of(x, eng, True), torch.tensor(c["x"]), torch.tensor(v))
        y, XN = eng.observe(c["x"], ops, final=True)
        yd, Xd = eng.observe_jvp(c["x"], v, ops, final=True)
        D = XN - Cm
        cot = lambda z: 4.0 * np.abs(z) ** 2 * z
        cot_dot = lambda z, zd: 8.0 * np.real(np.conj(z) * zd) * z + 4.0 * np.abs(z) ** 2 * zd
        want = eng.observe_hvp(c["x"], v, ops, cot(y) / N, cot(D), cot_dot(y, yd) / N, cot_dot(D, Xd))
        close(hv.numpy(), want, "torch.autograd.functional.hvp against observe_hvp")
        # twice=False behaves as before: once differentiable
        x = torch.tensor(c["x"], requires_grad=True)
        (g,) = torch.autograd.grad(loss_of(x, eng, False), x, create_graph=True)
        close(g.detach().numpy(), eng.observe_vjp(c["x"], ops, ybar=cot(y) / N, xbar_final=cot(D)), "x.grad against observe_vjp")
        assert not g.requires_grad
        with pytest.raises(RuntimeError):
            torch.autograd.grad((g * torch.tensor(v)).sum(), x)
        # twice=True, first order: the same gradient bits
        x2 = torch.tensor(c["x"], requires_grad=True)
        (g2,) = torch.autograd.grad(loss_of(x2, eng, True), x2)
        assert np.array_equal(g2.numpy(), g.detach().numpy())
