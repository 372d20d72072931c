"""grape_eval_jvp on the GPU: the Jacobian-vector product of the trajectory read-out against the NumPy / SciPy reference of
tests/jvp_reference.py (expm per slice, states by a loop, the first-order tangent from the O(N^2) double sum -- no tangent
recursion), at the project's parity bar relative to |ref|_inf; the adjoint identity against the shipped pull-back kernel;
exact causality and scaling; its invariants, coordinates, refusals, and torch forward-mode AD end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_vjp import invariant_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5


def cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def close(a, ref, what):
    amax = np.abs(ref).max()
    err = np.abs(np.asarray(a) - ref).max()
    print(f"{what}: |a-ref|_inf={err:.3e} |ref|_inf={amax:.3e}")
    assert amax > 0 and err <= PARITY_RTOL * amax, f"{what}: |a-ref|_inf={err:.3e} > {PARITY_RTOL * amax:.3e}"
    return err / amax


# ---- 1: parity ---------------------------------------------------------------------------------------------------------------
# n_obs x per_member: the reference is linear in the probes -- ONE pass of the double sum per shape gives the tangent states,
# every combination is a read-out of them
COMBOS = [(n_obs, pm) for n_obs in (1, 3, 16) for pm in (0, 1)]
_REF = {}


def shape_problem(n, m, N, E, herm, variant):
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    rng = np.random.default_rng(8000 + 100 * n + 10 * m + N + E)
    return c, cplx(rng, E, 16, n, m), cplx(rng, 16, n, m), rng.standard_normal((c["K"], N))


def shape_reference(key, c, xdot):
    if key not in _REF:
        D = jr.tangent_states_ref(c["A"], c["B"], c["Xi"], c["x"], xdot, c["T"], c["variant"])
        D.setflags(write=False)
        _REF[key] = D
    return _REF[key]


@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W,J,rho_kind", SHAPES)
def test_parity_against_the_double_sum_reference(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, J, rho_kind):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, O_mem, O_sh, xdot = shape_problem(n, m, N, E, herm, variant)
    D = shape_reference((n, m, N, E, herm, variant), c, xdot)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        for n_obs, pm in COMBOS:
            ops = O_mem[:, :n_obs] if pm else O_sh[:n_obs]
            yd, Xd = eng.observe_jvp(c["x"], xdot, ops, per_member=bool(pm), final=True)
            y_ref, X_ref = jr.read_out(D, ops, bool(pm))
            assert yd.shape == (E, n_obs, N + 1) and Xd.shape == (E, n, m)
            what = f"n={n} m={m} N={N} E={E} {kernel} n_obs={n_obs} per_member={pm}"
            close(yd, y_ref, what + " ydot")
            close(Xd, X_ref, what + " Xdot_final")
        names = eng.kernel_names()
        Xonly = eng.observe_jvp(c["x"], xdot, None, final=True)[1]           # the final tangent alone: n_obs = 0
    assert "trajectory_jvp_kernel" in names
    assert np.array_equal(Xonly, Xd)


# ---- 2: the adjoint identity against the shipped pull-back ------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,E,herm,kernel", [(4, 4, 65, 3, True, "pair"), (3, 1, 64, 3, False, "lane"), (2, 2, 130, 5, True, "lane")])
def test_adjoint_identity_against_the_pull_back_kernel(qoc, monkeypatch, n, m, N, E, herm, kernel):
    """<(ybar, Xbar), J xdot> = <J' (ybar, Xbar), xdot> with J' from trajectory_vjp_kernel, the parent's kernel: new code
    against shipped code, no finite differences (both linearise to first order in dt the same way)"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(5200 + 10 * n + m, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(5201 + n)
    O, xdot = cplx(rng, 3, n, m), rng.standard_normal((c["K"], N))
    ybar, xbar = cplx(rng, E, 3, N + 1), cplx(rng, E, n, m)
    with engine(qoc, c) as eng:
        yd, Xd = eng.observe_jvp(c["x"], xdot, O, final=True)
        G = eng.observe_vjp(c["x"], O, ybar=ybar, xbar_final=xbar)
        assert "trajectory_vjp_kernel" in eng.kernel_names()
    lhs, mag = jr.pairing(ybar, yd, xbar, Xd)
    rhs, scale = float(np.sum(G * xdot)), float(np.sum(np.abs(G * xdot))) + mag
    print(f"n={n} m={m} N={N} {kernel}: lhs={lhs:.15e} rhs={rhs:.15e} |lhs - rhs| / scale = {abs(lhs - rhs) / scale:.2e}")
    assert abs(lhs) > 0 and abs(lhs - rhs) <= PARITY_RTOL * scale


# ---- 3: causality and scaling, exact -----------------------------------------------------------------------------------------
def index_case():
    c = make_case(5101, 3, 2, 23, 2, hermitian=False)
    rng = np.random.default_rng(5102)
    return c, cplx(rng, 3, 3, 2), rng


def raw_jvp(qoc, eng, x, xdot, O, per_member=0):
    """the C entry point on NaN-filled outputs -> (ydot (E, n_obs, N+1), Xdot_final (E, n, m))"""
    lib = qoc.load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n_obs = O.shape[0]
    yd = np.full((eng.E, n_obs, eng.N + 1), np.nan + 1j * np.nan)
    Xd = np.full((eng.E, eng.m, eng.n), np.nan + 1j * np.nan)
    xf, xdf = np.ascontiguousarray(x.T), np.ascontiguousarray(xdot.T)
    Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
    rc = lib.grape_eval_jvp(eng._h, p(xf), p(xdf), n_obs, per_member, p(Of), p(yd), p(Xd))
    assert rc == 0, lib.grape_last_error(eng._h).decode()
    return yd, np.swapaxes(Xd, -1, -2)


def test_causality_is_exact(qoc):
    c, O, rng = index_case()
    t0 = 9
    xdot = np.zeros((2, 23))
    xdot[:, t0] = rng.standard_normal(2)
    with engine(qoc, c, slices_per_lane=2) as eng:
        yd, Xd = raw_jvp(qoc, eng, c["x"], xdot, O)
        y0, X0 = raw_jvp(qoc, eng, c["x"], np.zeros((2, 23)), O)
    assert not np.isnan(yd).any() and not np.isnan(Xd).any()  # fully overwritten, ydot[..., 0] included
    assert not yd[:, :, :t0 + 1].any()                        # the state after s <= t0 slices cannot see slice t0
    assert (yd[:, :, t0 + 1:] != 0).all() and (Xd != 0).all()
    y_ref, X_ref = jr.jvp_ref(c["A"], c["B"], c["Xi"], c["x"], xdot, T, O, False, c["variant"])
    close(yd, y_ref, "xdot at t0 = 9, ydot")
    close(Xd, X_ref, "xdot at t0 = 9, Xdot_final")
    assert not np.isnan(y0).any() and not y0.any() and not np.isnan(X0).any() and not X0.any()      # xdot = 0: exactly zero


@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", [(3, 2, 23, 2, False, "lane", 2, 0), (4, 4, 65, 3, True, "pair", 1, 3),
                                                     (2, 2, 130, 5, True, "lane", 0, 0)])
def test_scaling_is_exact(qoc, monkeypatch, n, m, N, E, herm, kernel, S, W):
    """every operation is linear in xdot and a power of two commutes with rounding"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(5300 + n, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(5301)
    O, xdot = cplx(rng, 3, n, m), rng.standard_normal((c["K"], N))
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        yd, Xd = eng.observe_jvp(c["x"], xdot, O, final=True)
        y2, X2 = eng.observe_jvp(c["x"], 2.0 * xdot, O, final=True)
        ym, Xm = eng.observe_jvp(c["x"], -xdot, O, final=True)
    assert np.abs(yd).max() > 0
    assert np.array_equal(y2, 2.0 * yd) and np.array_equal(X2, 2.0 * Xd)
    assert np.array_equal(ym, -yd) and np.array_equal(Xm, -Xd)


# ---- 4: invariants -------------------------------------------------------------------------------------------------------------
def jvp_case(herm=False, E=10):
    c, O, _, _ = invariant_case(herm, E)
    return c, O, np.random.default_rng(5401).standard_normal((c["K"], c["N"]))


def test_bitwise_call_to_call_and_eval_jvp_eval(qoc):
    c, O, xdot = jvp_case()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        ya, Xa = eng.observe_jvp(c["x"], xdot, O, final=True)
        assert "trajectory_jvp_kernel" in eng.kernel_names()
        F1, G1 = eng.eval(c["x"])
        assert eng.kernel_names() == names0 and "trajectory_jvp_kernel" not in names0
        yb, Xb = eng.observe_jvp(c["x"], xdot, O, final=True)
        yo = eng.observe_jvp(-c["x"], xdot, O)                # another call in between
        yc, Xc = eng.observe_jvp(c["x"], xdot, O, final=True)
    assert F1 == F0 and np.array_equal(G1, G0)
    assert np.array_equal(ya, yb) and np.array_equal(ya, yc) and np.array_equal(Xa, Xb) and np.array_equal(Xa, Xc)
    assert not np.array_equal(ya, yo)


@pytest.mark.parametrize("herm,E,members", [(False, 10, 4), (True, 10, 4), (True, 70, 24)])
def test_member_chunked_context_is_bitwise_the_unchunked_one(qoc, monkeypatch, herm, E, members):
    c, O, xdot = jvp_case(herm, E)
    with engine(qoc, c) as eng:
        yd, Xd = eng.observe_jvp(c["x"], xdot, O, final=True)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, herm, members)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < E and eng.info["member_chunk"] % 32 != 0, eng.info["member_chunk"]
        yc, Xc = eng.observe_jvp(c["x"], xdot, O, final=True)
    assert np.array_equal(yc, yd) and np.array_equal(Xc, Xd)


@pytest.mark.parametrize("standing", ["running_cost", "penalties", "risk"])
def test_standing_costs_do_not_enter(qoc, standing):
    c, O, xdot = jvp_case()
    with engine(qoc, c) as eng:
        yd, Xd = eng.observe_jvp(c["x"], xdot, O, final=True)
        F0, _ = eng.eval(c["x"])
        if standing == "running_cost":
            eng.set_running_cost(c["R"], c["rho"])
        elif standing == "penalties":
            eng.set_penalties(np.array([0.3, 0.1]), np.array([0.05, 0.2]))
        else:
            eng.set_risk(2.0)
        F1, _ = eng.eval(c["x"])
        ys, Xs = eng.observe_jvp(c["x"], xdot, O, final=True)
        F2, _ = eng.eval(c["x"])
    assert F1 != F0 and F2 == F1                              # the cost is in force, before and after
    assert np.array_equal(ys, yd) and np.array_equal(Xs, Xd)


# ---- 5: coordinates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["basis", "bounds", "both"])
def test_direction_is_taken_in_the_coordinates_of_x(qoc, mode):
    """the JVP under a pulse map = a plain context's JVP of the physical pulse along s * (thetadot phi'), formed in NumPy"""
    c = make_case(4401, 4, 2, 50, 3, hermitian=False)
    N, K = c["N"], c["K"]
    rng = np.random.default_rng(4402)
    O = cplx(rng, 2, 4, 2)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    assert phi.shape == (N, 5)
    x0 = 0.2 * rng.standard_normal((K, N))
    lo, hi = np.array([-0.8, -0.5]), np.array([0.9, 0.6])
    with engine(qoc, c) as eng:
        if mode != "bounds":
            eng.set_basis(phi, x0)
            theta, thetadot = 0.4 * rng.standard_normal((K, 5)), rng.standard_normal((K, 5))
            a, adot = x0 + theta @ phi.T, thetadot @ phi.T
        else:
            theta, thetadot = 0.7 * rng.standard_normal((K, N)), rng.standard_normal((K, N))
            a, adot = theta, thetadot
        if mode != "basis":
            eng.set_bounds(lo, hi)
        x = eng.controls(theta)
        yd, Xd = eng.observe_jvp(theta, thetadot, O, final=True)
        names = eng.kernel_names()
    assert ("bounds_tangent_kernel" if mode == "bounds" else "basis_expand_kernel") in names and "trajectory_jvp_kernel" in names
    xdot_phys = adot
    if mode != "basis":
        mid, half = (0.5 * (lo + hi))[:, None], (0.5 * (hi - lo))[:, None]
        xdot_phys = adot * (1.0 - np.tanh((a - mid) / half) ** 2)
    with engine(qoc, c) as eng:
        y_plain, X_plain = eng.observe_jvp(x, xdot_phys, O, final=True)
    close(yd, y_plain, mode + " ydot")
    close(Xd, X_plain, mode + " Xdot_final")


# ---- 6: refusals and arguments -----------------------------------------------------------------------------------------------
def raw_call(qoc, eng, x, xdot, n_obs, per_member, O, ydot, Xdot):
    lib = qoc.load_library()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.grape_eval_jvp(eng._h, ptr(x), ptr(xdot), n_obs, per_member, ptr(O), ptr(ydot), ptr(Xdot))
    return rc, lib.grape_last_error(eng._h).decode()


def test_refusals(qoc):
    c = make_case(4501, 4, 4, 20, 2)
    GE = qoc.GrapeError

    def refused(eng, case, word):
        F0, G0 = eng.eval(case["x"])                          # the bits from before the refusal
        with pytest.raises(GE) as ei:
            eng.observe_jvp(case["x"], np.ones_like(case["x"]), None, final=True)
        assert ei.value.status == -2 and word in str(ei.value) and "grape_eval_jvp" in str(ei.value), str(ei.value)
        F, G = eng.eval(case["x"])
        assert F == F0 and np.array_equal(G, G0)

    for nbad in (5, 1):
        big = make_case(4502 + nbad, nbad, nbad, 8, 1)
        with engine(qoc, big) as eng:
            refused(eng, big, "dimension")
    for sys_type in ("StateTransfer", "CoherenceTransfer"):
        with qoc.GrapeEngine(sys_type, c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], T, 20) as eng:
            refused(eng, c, "StateTransfer")
    with engine(qoc, c, gradient="exact") as eng:
        refused(eng, c, "exact")
    with engine(qoc, c, gradient="exact", objective="c1") as eng:
        refused(eng, c, "exact")
    with engine(qoc, c, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM) as eng:
        refused(eng, c, "multi-device")
    with engine(qoc, c, force_collective=True) as eng:
        refused(eng, c, "communicator")


def test_invalid_arguments(qoc):
    c = make_case(4601, 4, 4, 20, 2)
    E, N, K = c["E"], c["N"], c["K"]
    rng = np.random.default_rng(4602)
    O = cplx(rng, 2, 4, 4)
    GE = qoc.GrapeError
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])

        def same_bits():
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)

        xf = np.ascontiguousarray(c["x"].T)
        xdf = np.ascontiguousarray(rng.standard_normal((N, K)))
        Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
        yd, Xd = np.empty((E, 2, N + 1), complex), np.empty((E, 4, 4), complex)
        bad_args = [
            (None, xdf, 2, 0, Of, yd, Xd),                    # null x
            (xf, None, 2, 0, Of, yd, Xd),                     # null xdot
            (xf, xdf, 2, 0, Of, None, None),                  # ydot and Xdot_final both NULL
            (xf, xdf, -1, 0, Of, yd, Xd), (xf, xdf, 17, 0, Of, yd, Xd),       # n_obs outside 0..16
            (xf, xdf, 0, 0, Of, yd, Xd),                      # n_obs = 0 with a non-NULL ydot
            (xf, xdf, 2, 0, None, yd, Xd),                    # n_obs > 0 with a NULL O
            (xf, xdf, 2, 2, Of, yd, Xd), (xf, xdf, 2, -1, Of, yd, Xd),        # per_member other than 0 or 1
        ]
        for args in bad_args:
            rc, msg = raw_call(qoc, eng, *args)
            assert rc == -1 and "grape_eval_jvp" in msg, (rc, msg)
            same_bits()
        for which in range(2):                                # a non-finite entry of O, xdot
            arrs = [Of.copy(), xdf.copy()]
            arrs[which].reshape(-1)[5] = [np.nan, np.inf][which]
            rc, msg = raw_call(qoc, eng, xf, arrs[1], 2, 0, arrs[0], yd, Xd)
            assert rc == -1 and "not finite" in msg and ["O[", "xdot["][which] in msg, (rc, msg)
            same_bits()
        # valid corners: Xdot_final alone with n_obs = 0; ydot alone
        rc, msg = raw_call(qoc, eng, xf, xdf, 0, 0, None, None, Xd)
        assert rc == 0, msg
        rc, msg = raw_call(qoc, eng, xf, xdf, 2, 0, Of, yd, None)
        assert rc == 0, msg
        # the Python layer catches wrong shapes before the library is called
        for call in (lambda: eng.observe_jvp(c["x"], xdf.T[:, :5], O), lambda: eng.observe_jvp(c["x"][:, :5], xdf.T, O),
                     lambda: eng.observe_jvp(c["x"], xdf.T, None), lambda: eng.observe_jvp(c["x"], xdf.T, np.zeros((17, 4, 4))),
                     lambda: eng.observe_jvp(c["x"], xdf.T, O[:, :3])):
            with pytest.raises(ValueError):
                call()
        # a NaN in x gives NaN out and no error
        xn = c["x"].copy()
        xn[1, 7] = np.nan
        assert np.isnan(eng.observe_jvp(xn, xdf.T, O)).any()
        same_bits()
    # before grape_set_operators
    lib = qoc.load_library()
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.grape_eval_jvp(h, p(xf), p(xdf), 2, 0, p(Of), p(yd), None) == -5
        assert b"operators not set" in lib.grape_last_error(h)
    finally:
        lib.grape_destroy(h)


# ---- 7: torch forward mode, end to end -----------------------------------------------------------------------------------------
def test_forward_ad_through_trajectory_on_cpu_tensors(qoc):
    """the forward_ad tangent of autograd.trajectory is observe_jvp's output exactly; for a log-barrier loss the dual-number
    derivative equals <x.grad from backward, xdot> at the parity bar (of sum |x.grad xdot|)"""
    import torch
    import torch.autograd.forward_ad as fwad
    from quoptimalcontrol_jl_amd import autograd
    N, mu = 40, 0.5
    c = make_case(4701, 3, 1, N, 1)
    c["Xi"] = np.array([[[1.0], [0.0], [0.0]]], complex)
    c["Xt"] = np.array([[[0.0], [1.0], [0.0]]], complex)
    ops = np.array([[[0.0], [1.0], [0.0]], [[0.0], [0.0], [1.0]]], complex)
    xdot = np.random.default_rng(5701).standard_normal(c["x"].shape)

    def loss_of(y):
        return 1.0 - y[0, 0, N].abs() ** 2 - mu / N * torch.log(1.0 - y[0, 1].abs() ** 2).sum()

    with engine(qoc, c) as eng:
        with fwad.dual_level():
            xd = fwad.make_dual(torch.tensor(c["x"]), torch.tensor(xdot))
            y, XN = autograd.trajectory(eng, xd, ops)
            assert "trajectory_jvp_kernel" in eng.kernel_names()
            yt, Xt = fwad.unpack_dual(y).tangent, fwad.unpack_dual(XN).tangent
            lt = float(fwad.unpack_dual(loss_of(y)).tangent)
        yd, Xd = eng.observe_jvp(c["x"], xdot, ops, final=True)
        assert np.array_equal(yt.numpy(), yd) and np.array_equal(Xt.numpy(), Xd)
        x = torch.tensor(c["x"], requires_grad=True)
        loss_of(autograd.trajectory(eng, x, ops, final=False)).backward()
    g = x.grad.numpy()
    want, scale = float(np.sum(g * xdot)), float(np.sum(np.abs(g * xdot)))
    print(f"log-barrier loss: forward-mode derivative {lt:.15e}, <x.grad, xdot> {want:.15e}, scale {scale:.3e}")
    assert abs(lt - want) <= PARITY_RTOL * scale
