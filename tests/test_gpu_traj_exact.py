"""grape_set_trajectory_derivative(GRAPE_TRAJ_EXACT) on the GPU: the exact derivative mode of the trajectory pull-back and
push-forward against the NumPy / SciPy reference of tests/traj_exact_reference.py (scipy.linalg.expm_frechet per slice, the
pull-back from the O(N^2) double sum, the push-forward from the plain recurrence) at the project's parity bar; with scaled
slices (the Frechet kernels' squarings must be the sweep's); against central differences of the device's own read-out and
torch.autograd.gradcheck; the transpose pairing and the linearity of the push-forward; bit identities (call to call, host =
device, reuse, member chunks); mode 0 untouched; the compositions, the refusals, and one optimisation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import mixed_norm_cases as mn  # noqa: E402
import traj_exact_reference as xr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_jvp_device import jvp_dev, swept  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_traj_device import observe_dev, vjp_dev  # noqa: E402
from test_gpu_vjp import cplx, invariant_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5
ROWS = [r[:9] for r in SHAPES]                                # (n, m, N, E, hermitian, variant, kernel, S, W)
VJP_EXACT = ["trajectory_vjp_exact_kernel", "traj_frechet_rows_kernel", "vjp_sum_kernel"]
JVP_EXACT = ["traj_frechet_dir_kernel", "trajectory_jvp_exact_kernel"]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def exact(eng):
    eng.set_trajectory_derivative("exact")
    assert eng.trajectory_derivative == "exact"
    return eng


def close(got, ref, what):
    """|got - ref|_inf <= PARITY_RTOL |ref|_inf, per output array"""
    scale = np.abs(ref).max()
    err = np.abs(np.asarray(got) - ref).max()
    assert scale > 0 and err <= PARITY_RTOL * scale, f"{what}: |got-ref|_inf={err:.3e} > {PARITY_RTOL * scale:.3e}"
    return err / scale


# ---- 1: parity -----------------------------------------------------------------------------------------------------------------
_REF = {}


def parity_problem(c, n_obs, per_member, seed):
    rng = np.random.default_rng(seed)
    E, n, m, N, K = c["E"], c["n"], c["m"], c["N"], c["K"]
    O = cplx(rng, E, n_obs, n, m) if per_member else cplx(rng, n_obs, n, m)
    return O, cplx(rng, E, n_obs, N + 1), cplx(rng, E, n, m), rng.standard_normal((K, N))


def parity_reference(key, c, O, yb, xb, xdot, per_member):
    """(G, ydot, Xdot_final) of the reference, once per case; the slice derivatives are shared by both directions"""
    if key not in _REF:
        PL = xr.slice_derivatives(c["A"], c["B"], c["x"], c["T"], c["variant"])
        G = xr.exact_vjp_ref(c["A"], c["B"], c["Xi"], c["x"], c["T"], O, yb, xb, per_member, c["variant"], PL)
        ydot, xdf = xr.exact_jvp_ref(c["A"], c["B"], c["Xi"], c["x"], xdot, c["T"], O, per_member, c["variant"], PL)
        for a in (G, ydot, xdf):
            a.setflags(write=False)
        _REF[key] = (G, ydot, xdf)
    return _REF[key]


def check_parity(eng, c, key, n_obs, per_member, seed, what):
    O, yb, xb, xdot = parity_problem(c, n_obs, per_member, seed)
    G_ref, yd_ref, xdf_ref = parity_reference(key, c, O, yb, xb, xdot, per_member)
    G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb, per_member=per_member)
    names = eng.kernel_names()
    assert all(k in names for k in VJP_EXACT) and "trajectory_vjp_kernel" not in names, names
    ydot, xdf = eng.observe_jvp(c["x"], xdot, O, per_member=per_member, final=True)
    names = eng.kernel_names()
    assert all(k in names for k in JVP_EXACT) and "trajectory_jvp_kernel" not in names, names
    errs = (close(G, G_ref, what + " G"), close(ydot, yd_ref, what + " ydot"), close(xdf, xdf_ref, what + " Xdot_final"))
    print(f"{what}: rel G {errs[0]:.2e} ydot {errs[1]:.2e} Xdot_final {errs[2]:.2e}")
    assert not ydot[:, :, 0].any()                            # row 0 is zero and written


@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W", ROWS)
def test_parity_against_the_expm_frechet_reference(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        check_parity(exact(eng), c, ("shape", n, m, N, E, herm, variant), 3, False, 8000 + 100 * n + 10 * m + N + E,
                     f"n={n} m={m} N={N} E={E} {kernel}")


# one lane shape, one pair shape, one n x 1 shape: 16 per-member probes
@pytest.mark.parametrize("row", [6, 8, 10])
def test_parity_with_sixteen_per_member_probes(qoc, monkeypatch, row):
    n, m, N, E, herm, variant, kernel, S, W = ROWS[row]
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        check_parity(exact(eng), c, ("pm16", row), 16, True, 8100 + row, f"row {row} n={n} m={m} N={N} E={E} {kernel} 16 per member")


# ---- 2: squarings ------------------------------------------------------------------------------------------------------------------
def slice_squarings(c):
    """(E, N) squarings_for(norm1_bound(G_t)) on the host"""
    b = mn.slice_bounds(c["A"], c["B"], c["x"], c["T"] / c["N"])
    return np.vectorize(mn.squarings)(b)


# n, m, N, T, hermitian, kernel: lane and pair at N = 7 and N = 65, T so that every slice needs s >= 2
SCALED = [(2, 2, 7, 1.5, True, "pair"), (2, 1, 65, 24.0, False, "lane"), (3, 3, 7, 1.5, False, "lane"), (3, 2, 65, 24.0, True, "lane"),
          (4, 4, 7, 1.5, True, "pair"), (4, 4, 65, 24.0, True, "pair"), (4, 2, 7, 1.5, False, "lane"), (4, 1, 65, 24.0, False, "pair")]


@pytest.mark.parametrize("n,m,N,Tc,herm,kernel", SCALED)
def test_parity_on_scaled_slices(qoc, monkeypatch, n, m, N, Tc, herm, kernel):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(8200 + 10 * n + m + N, n, m, N, 2, hermitian=herm, T=Tc)
    s = slice_squarings(c)
    assert s.min() >= 2, s                                    # a test that never leaves s = 0 proves nothing
    with engine(qoc, c) as eng:
        check_parity(exact(eng), c, ("scaled", n, m, N, herm), 3, False, 8300 + 10 * n + m + N,
                     f"scaled n={n} m={m} N={N} T={Tc} {kernel} s={s.min()}..{s.max()}")


@pytest.mark.parametrize("n,cols,kernel,herm", [(4, None, "pair", True), (3, 2, "lane", False)])
def test_parity_on_a_pulse_whose_slices_need_different_squarings(qoc, monkeypatch, n, cols, kernel, herm):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    A, B, Xi, Xt, wts, x, Tc = mn.make_case(n, 2, 23, 3, "UnitaryGate", herm, "shuffled", 4, 8400 + n, cols=cols)
    c = dict(n=n, m=Xi.shape[2], N=23, E=3, K=2, A=A, B=B, Xi=Xi, Xt=Xt, wts=wts, x=x, variant=0, T=Tc)
    s = slice_squarings(c)
    assert 0 in s and len(np.unique(s)) >= 4 and s.max() >= 4, s      # different s within one pulse, s = 0 among them
    with engine(qoc, c) as eng:
        check_parity(exact(eng), c, ("mixed", n), 3, False, 8500 + n, f"mixed norms n={n} {kernel} s={s.min()}..{s.max()}")


@pytest.mark.parametrize("forced", [0, 3])
@pytest.mark.parametrize("n,m,kernel,herm", [(4, 4, "pair", True), (3, 3, "lane", False), (2, 2, "pair", False)])
def test_parity_with_forced_squarings(qoc, monkeypatch, forced, n, m, kernel, herm):
    """(N = 64 at T = 0.2: every slice's norm bound is below 0.08 -- the Taylor polynomial is accurate unscaled, as the sweep
    evaluates it under expm_squarings = 0, and scaled 3 times)"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(8600 + 10 * n + m, n, m, 64, 2, hermitian=herm, T=0.2)
    assert mn.slice_bounds(c["A"], c["B"], c["x"], c["T"] / 64).max() < mn.THETA8
    with engine(qoc, c, expm_squarings=forced) as eng:
        check_parity(exact(eng), c, ("forced", n, m), 3, False, 8700 + 10 * n + m, f"forced s={forced} n={n} m={m} {kernel}")


# ---- 3: against the device itself ---------------------------------------------------------------------------------------------
def device_loss(eng, x, O):
    y, XN = eng.observe(x, O, final=True)
    return xr.smooth_loss(y, XN)


def central_differences(eng, x, O, h=1e-5):
    g = np.empty_like(x)
    for cc in range(x.shape[0]):
        for t in range(x.shape[1]):
            d = np.zeros_like(x)
            d[cc, t] = h
            g[cc, t] = (device_loss(eng, x + d, O)[0] - device_loss(eng, x - d, O)[0]) / (2 * h)
    return g


@pytest.mark.parametrize("n,m,N,E", [(4, 4, 8, 3), (3, 1, 8, 2)])
def test_against_central_differences_of_the_devices_read_out(qoc, n, m, N, E):
    c = make_case(8800 + n, n, m, N, E, hermitian=(n == 4))
    O = cplx(np.random.default_rng(8801), 3, n, m)
    with engine(qoc, c) as eng:
        _, ybar, xbar = device_loss(eng, c["x"], O)
        G1 = eng.observe_vjp(c["x"], O, ybar=ybar, xbar_final=xbar)
        G = exact(eng).observe_vjp(c["x"], O, ybar=ybar, xbar_final=xbar)
        fd = central_differences(eng, c["x"], O)
    dev_x, dev_1 = np.abs(G - fd).max() / np.abs(fd).max(), np.abs(G1 - fd).max() / np.abs(fd).max()
    print(f"n={n} m={m} N={N} E={E}: against central differences: exact {dev_x:.2e}, first order {dev_1:.2e}")
    assert dev_x <= 1e-6, dev_x


def test_gradcheck_passes_in_exact_mode(qoc, torch):
    from quoptimalcontrol_jl_amd import autograd
    c = make_case(8900, 2, 2, 6, 2)
    O = cplx(np.random.default_rng(8901), 2, 2, 2)
    with engine(qoc, c) as eng:
        exact(eng)
        x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
        assert torch.autograd.gradcheck(lambda xx: autograd.trajectory(eng, xx, O), (x,))


# ---- 4: pairing and linearity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [2, 6, 9, 12])
def test_push_forward_and_pull_back_are_a_transpose_pair(qoc, monkeypatch, row):
    n, m, N, E, herm, variant, kernel, S, W = ROWS[row]
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    O, yb, xb, xdot = parity_problem(c, 3, False, 9000 + row)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        exact(eng)
        G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        ydot, xdf = eng.observe_jvp(c["x"], xdot, O, final=True)
        y2, x2 = eng.observe_jvp(c["x"], 2.0 * xdot, O, final=True)
        ym, xm = eng.observe_jvp(c["x"], -xdot, O, final=True)
        y0, x0 = eng.observe_jvp(c["x"], 0.0 * xdot, O, final=True)
    lhs, mag = jr.pairing(yb, ydot, xb, xdf)
    rhs = float(np.sum(G * xdot))
    print(f"row {row}: <cot, J v> = {lhs:.15e}, <J' cot, v> = {rhs:.15e}, relative {abs(lhs - rhs) / mag:.2e}")
    assert abs(lhs - rhs) <= 1e-12 * mag
    assert np.array_equal(y2, 2.0 * ydot) and np.array_equal(x2, 2.0 * xdf)
    assert np.array_equal(ym, -ydot) and np.array_equal(xm, -xdf)
    assert not y0.any() and not x0.any()


# ---- 5: bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("herm", [False, True])
def test_bits_call_to_call_host_device_and_reuse(qoc, torch, herm):
    c, O, yb, xb = invariant_case(herm)
    xdot = np.random.default_rng(9101).standard_normal((c["K"], c["N"]))
    with engine(qoc, c) as eng:
        exact(eng)
        G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        yd, Xd = eng.observe_jvp(c["x"], xdot, O, final=True)
        eng.observe_vjp(-c["x"], O, ybar=yb)                  # another call in between
        assert np.array_equal(eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb), G)
        yd2, Xd2 = eng.observe_jvp(c["x"], xdot, O, final=True)
        assert np.array_equal(yd2, yd) and np.array_equal(Xd2, Xd)
        # the device forms, with d_x and along the stored trajectory
        Gd = vjp_dev(torch, eng, c["x"], O, yb, xb, False)
        names = eng.kernel_names()
        assert swept(names) and all(k in names for k in VJP_EXACT) and "trajectory_vjp_staged_kernel" not in names, names
        Gr = vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)
        names = eng.kernel_names()
        assert not swept(names) and all(k in names for k in VJP_EXACT), names
        assert np.array_equal(Gd, G) and np.array_equal(Gr, G)
        ydd, Xdd = jvp_dev(torch, eng, c["x"], xdot, O, False)
        assert swept(eng.kernel_names())
        ydr, Xdr = jvp_dev(torch, eng, None, xdot, O, False, reuse=True)
        names = eng.kernel_names()
        assert not swept(names) and all(k in names for k in JVP_EXACT), names
        for a, b in ((ydd, yd), (Xdd, Xd), (ydr, yd), (Xdr, Xd)):
            assert np.array_equal(a, b)
        # the Gauss-Newton sequence: one read-out, then J v and J' w along its trajectory (the buffer of W_t and E_t is shared)
        observe_dev(torch, eng, c["x"], O, False)
        ygn, Xgn = jvp_dev(torch, eng, None, xdot, O, False, reuse=True)
        Ggn = vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)
        ygn2, Xgn2 = jvp_dev(torch, eng, None, xdot, O, False, reuse=True)
        assert not swept(eng.kernel_names())
        assert np.array_equal(ygn, yd) and np.array_equal(Xgn, Xd) and np.array_equal(Ggn, G)
        assert np.array_equal(ygn2, yd) and np.array_equal(Xgn2, Xd)


# (the members' rows are summed in groups of 32 consecutive members: blocks of 4 of 10 members split one group three ways,
# blocks of 24 of 70 cut through every group)
@pytest.mark.parametrize("herm,E,members", [(False, 10, 4), (True, 10, 4), (True, 70, 24)])
def test_member_chunked_context_is_bitwise_the_unchunked_one(qoc, monkeypatch, herm, E, members):
    c, O, yb, xb = invariant_case(herm, E)
    xdot = np.random.default_rng(9201).standard_normal((c["K"], c["N"]))
    with engine(qoc, c) as eng:
        exact(eng)
        G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        yd, Xd = eng.observe_jvp(c["x"], xdot, O, final=True)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, herm, members)))
    with engine(qoc, c) as eng:
        exact(eng)
        assert 0 < eng.info["member_chunk"] < E and eng.info["member_chunk"] % 32 != 0, eng.info["member_chunk"]
        Gc = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        ydc, Xdc = eng.observe_jvp(c["x"], xdot, O, final=True)
    assert np.array_equal(Gc, G) and np.array_equal(ydc, yd) and np.array_equal(Xdc, Xd)


# ---- 6: mode 0 is untouched ------------------------------------------------------------------------------------------------------
def test_first_order_mode_is_untouched(qoc):
    c, O, yb, xb = invariant_case()
    xdot = np.random.default_rng(9301).standard_normal((c["K"], c["N"]))

    def first_order(eng):
        G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        nv = eng.kernel_names()
        yd, Xd = eng.observe_jvp(c["x"], xdot, O, final=True)
        return G, yd, Xd, nv, eng.kernel_names()

    with engine(qoc, c) as eng:                               # a context that never calls the setting
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        never = first_order(eng)
        ws0 = eng.info["workspace_bytes"]
    with engine(qoc, c) as eng:
        assert eng.trajectory_derivative == "first_order"
        eng.set_trajectory_derivative("first_order")
        F1, G1 = eng.eval(c["x"])
        first = first_order(eng)
        exact(eng)
        Gx = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        ydx, _ = eng.observe_jvp(c["x"], xdot, O, final=True)
        assert eng.info["workspace_bytes"] > ws0              # the per-slice blocks are counted
        F2, G2 = eng.eval(c["x"])
        assert eng.kernel_names() == names0
        eng.set_trajectory_derivative("first_order")
        assert eng.trajectory_derivative == "first_order"
        third = first_order(eng)
        F3, G3 = eng.eval(c["x"])
    for F, G in ((F1, G1), (F2, G2), (F3, G3)):
        assert F == F0 and np.array_equal(G, G0)
    for a, b in ((first, never), (third, never)):
        assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])) and a[3:] == b[3:]
    nv, nj = never[3], never[4]
    assert "trajectory_vjp_kernel" in nv and "trajectory_jvp_kernel" in nj
    assert not any("exact" in k or "frechet" in k for k in nv + nj), (nv, nj)
    assert not np.array_equal(Gx, never[0]) and not np.array_equal(ydx, never[1])


# ---- 7: composition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["basis", "bounds", "both"])
def test_results_come_back_in_the_coordinates_of_x(qoc, mode):
    c = make_case(4401, 4, 2, 50, 3, hermitian=False)
    N, K = c["N"], c["K"]
    rng = np.random.default_rng(9402)
    O, yb, xb = cplx(rng, 2, 4, 2), cplx(rng, 3, 2, N + 1), cplx(rng, 3, 4, 2)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    assert phi.shape == (N, 5)
    x0 = 0.2 * rng.standard_normal((K, N))
    lo, hi = np.array([-0.8, -0.5]), np.array([0.9, 0.6])
    with engine(qoc, c) as eng:
        exact(eng)
        if mode != "bounds":
            eng.set_basis(phi, x0)
            theta, tdot = 0.4 * rng.standard_normal((K, 5)), rng.standard_normal((K, 5))
            a, adot = x0 + theta @ phi.T, tdot @ phi.T
        else:
            theta, tdot = 0.7 * rng.standard_normal((K, N)), rng.standard_normal((K, N))
            a, adot = theta, tdot
        if mode != "basis":
            eng.set_bounds(lo, hi)
        assert eng.trajectory_derivative == "exact"
        x = eng.controls(theta)
        G = eng.observe_vjp(theta, O, ybar=yb, xbar_final=xb)
        ydot, xdf = eng.observe_jvp(theta, tdot, O, final=True)
    slope = np.ones((K, N))
    if mode != "basis":
        mid, half = (0.5 * (lo + hi))[:, None], (0.5 * (hi - lo))[:, None]
        slope = 1.0 - np.tanh((a - mid) / half) ** 2
    with engine(qoc, c) as eng:
        exact(eng)
        G_plain = eng.observe_vjp(x, O, ybar=yb, xbar_final=xb)
        yd_plain, xdf_plain = eng.observe_jvp(x, slope * adot, O, final=True)
    want = G_plain * slope
    if mode != "bounds":
        want = want @ phi
    assert G.shape == want.shape == ((K, N) if mode == "bounds" else (K, 5))
    close(G, want, mode + " G")
    close(ydot, yd_plain, mode + " ydot")
    close(xdf, xdf_plain, mode + " Xdot_final")


@pytest.mark.parametrize("standing", ["running_cost", "penalties", "risk"])
def test_standing_costs_do_not_enter(qoc, standing):
    c, O, yb, xb = invariant_case()
    with engine(qoc, c) as eng:
        exact(eng)
        G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        F0, _ = eng.eval(c["x"])
        if standing == "running_cost":
            eng.set_running_cost(c["R"], c["rho"])
        elif standing == "penalties":
            eng.set_penalties(np.array([0.3, 0.1]), np.array([0.05, 0.2]))
        else:
            eng.set_risk(2.0)
        F1, _ = eng.eval(c["x"])
        Gs = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        if standing == "running_cost":
            assert "running_cost_kernel" in eng.kernel_names()
        F2, _ = eng.eval(c["x"])
    assert F1 != F0 and F2 == F1                              # the cost is in force, before and after
    assert np.array_equal(Gs, G)


# ---- 8: refusals and arguments -----------------------------------------------------------------------------------------------------
def test_refusals_and_invalid_arguments(qoc):
    c = make_case(4501, 4, 4, 20, 2)
    GE = qoc.GrapeError
    lib = qoc.load_library()

    def refused(eng, case, word):
        F0, G0 = eng.eval(case["x"])
        with pytest.raises(GE) as ei:
            eng.set_trajectory_derivative("exact")
        assert ei.value.status == -2 and word in str(ei.value) and "grape_set_trajectory_derivative" in str(ei.value), str(ei.value)
        assert eng.trajectory_derivative == "first_order"
        eng.set_trajectory_derivative("first_order")          # (switching off what can never be on)
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

    rng = np.random.default_rng(9501)
    O, yb = cplx(rng, 2, 4, 4), cplx(rng, 2, 2, 21)
    with engine(qoc, c) as eng:
        exact(eng)
        G = eng.observe_vjp(c["x"], O, ybar=yb)
        for bad in (2, -1, 7):                                # mode outside {0, 1}: the exact mode stays in force
            assert lib.grape_set_trajectory_derivative(eng._h, bad) == -1
            assert b"grape_set_trajectory_derivative" in lib.grape_last_error(eng._h)
            assert np.array_equal(eng.observe_vjp(c["x"], O, ybar=yb), G)
        with pytest.raises(GE) as ei:                         # attaching an exchange while the mode is exact
            eng.ipc_attach([eng.ipc_export(1)], 0, 1)
        assert ei.value.status == -2 and "trajectory derivative" in str(ei.value)
        with pytest.raises(GE) as ei:
            eng.comm_attach(bytes(128), 0, 1)
        assert ei.value.status == -2 and "trajectory derivative" in str(ei.value)
        assert np.array_equal(eng.observe_vjp(c["x"], O, ybar=yb), G)
        eng.set_operators(c["A"], c["B"], c["Xi"], c["Xt"], c["wts"])       # the setting persists
        assert np.array_equal(eng.observe_vjp(c["x"], O, ybar=yb), G)
        assert "traj_frechet_rows_kernel" in eng.kernel_names()
    assert lib.grape_set_trajectory_derivative(None, 1) == -1


def test_the_setting_clears_the_trajectory_valid_flag(qoc, torch):
    c, O, yb, xb = invariant_case()
    with engine(qoc, c) as eng:
        observe_dev(torch, eng, c["x"], O, False)
        eng.set_trajectory_derivative("exact")
        with pytest.raises(qoc.GrapeError) as ei:
            vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)
        assert ei.value.status == -5 and "reuse" in str(ei.value)


# ---- 9: one optimisation -----------------------------------------------------------------------------------------------------------
def test_lbfgs_on_a_custom_loss_converges_in_exact_mode(qoc, torch):
    """L-BFGS on l = sum 0.1 cos(Re z + j) + 0.01 |z|^4 over (y, X_N) at (n, m, N, E) = (3, 3, 12, 2), from one start in both
    modes, by one procedure: SciPy's L-BFGS-B (memory 20) until it stops; where it stops within 1e-6 of a stationary point
    of its own gradient, torch's L-BFGS with unit steps and no line search goes on from there on gradients alone.
    (L-BFGS-B's line search works on differences of l, which run out of digits at |g| ~ 1e-8: it stops there, with
    "relative reduction of f" or an abnormal line search, however good the gradient is -- at 2.2e-8 here.)  Exact mode must reach |g|_inf <= 1e-8 by the optimiser's own gradient, and the
    central-difference gradient (h = 1e-5) at its stopping point must be <= 1e-6.  First-order mode: L-BFGS-B ends in an
    abnormal line search (its direction is no descent direction of l); the central-difference gradient at that point is
    printed, not asserted -- 0.29 next to an own |g|_inf of 0.12 in the run recorded in DESIGN.md 4.18."""
    from scipy.optimize import minimize
    c = make_case(9600, 3, 3, 12, 2)
    O = cplx(np.random.default_rng(9601), 2, 3, 3)
    K, N = c["K"], c["N"]
    out = {}
    with engine(qoc, c) as eng:
        def fun(z):
            x = z.reshape(K, N)
            l, ybar, xbar = device_loss(eng, x, O)
            return l, eng.observe_vjp(x, O, ybar=ybar, xbar_final=xbar).ravel()

        def unit_steps(z0):
            z = torch.tensor(z0, dtype=torch.float64, requires_grad=True)
            opt = torch.optim.LBFGS([z], lr=1.0, max_iter=100, max_eval=200, tolerance_grad=1e-9, tolerance_change=0.0,
                                    history_size=20, line_search_fn=None)

            def closure():
                l, g = fun(z.detach().numpy())
                z.grad = torch.from_numpy(g.copy())
                return torch.tensor(l)

            opt.step(closure)
            return z.detach().numpy()

        for mode in ("first_order", "exact"):
            eng.set_trajectory_derivative(mode)
            res = minimize(fun, c["x"].ravel(), jac=True, method="L-BFGS-B",
                           options=dict(maxiter=2000, maxfun=20000, gtol=1e-9, ftol=0.0, maxcor=20))
            z, own1 = res.x, np.abs(fun(res.x)[1]).max()
            if own1 <= 1e-6:
                z = unit_steps(z)
            l, g = fun(z)
            own, fd = np.abs(g).max(), np.abs(central_differences(eng, z.reshape(K, N), O)).max()
            out[mode] = (own, fd, res.nit, l)
            print(f"{mode}: L-BFGS-B {res.nit} iterations, own |g|_inf {own1:.2e} (status {res.status}: {res.message}); at the end: "
                  f"loss {l:.12f}, own |g|_inf {own:.2e}, central-difference |g|_inf {fd:.2e}")
    own, fd, _, _ = out["exact"]
    assert own <= 1e-8 and fd <= 1e-6, out
