"""grape_eval_gnvp on the GPU: the weighted Gauss-Newton product of the trajectory read-out against the NumPy / SciPy reference of
tests/gnvp_reference.py (jvp_recurrence -> weight blocks -> vjp_of_propagators: no chunks, no scans, no stored sources) at the
project's parity bar relative to |ref|_inf; against the composition of the shipped push-forward and pull-back on the device;
its exact identities, symmetry and definiteness, invariants, coordinates, device form, refusals, and the Levenberg-Marquardt
loop of quoptimalcontrol_jl_amd.gauss_newton end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnvp_cases as gc  # noqa: E402
import gnvp_reference as gr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_traj_device import _probes_cm, dev, observe_dev, ptr, vjp_dev  # noqa: E402
from test_gpu_jvp_device import jvp_dev, swept  # noqa: E402
from test_gpu_vjp import invariant_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5
cplx = gc.cplx


def close(a, ref, what):
    amax = np.abs(ref).max()
    err = np.abs(np.asarray(a) - ref).max()
    print(f"{what}: |a-ref|_inf={err:.3e} |ref|_inf={amax:.3e}")
    assert amax > 0 and err <= PARITY_RTOL * amax, f"{what}: |a-ref|_inf={err:.3e} > {PARITY_RTOL * amax:.3e}"


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---- 1: parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W,J,rho_kind", SHAPES)
def test_parity_against_the_composed_reference(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, J, rho_kind):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, d = gc.shape_problem(n, m, N, E, herm, variant)
    ref = gc.shape_reference((n, m, N, E, herm, variant))
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        for (way, n_obs, pm), want in ref.items():
            ops, w, wf = gc.call_arguments(d, way, n_obs, pm)
            Gn = eng.observe_gnvp(c["x"], d["xdot"], ops, w=w, wf=wf, per_member=bool(pm))
            assert Gn.shape == (c["K"], N)
            close(Gn, want, f"n={n} m={m} N={N} E={E} {kernel} {way} n_obs={n_obs} per_member={pm}")
            names = eng.kernel_names()
            assert "trajectory_gnvp_kernel" in names and "vjp_sum_kernel" in names, names
            assert "trajectory_jvp_kernel" not in names and "trajectory_vjp_kernel" not in names, names


# ---- 2: fused against composed on the device; exact identities ------------------------------------------------------------------
CASES3 = [(3, 2, 23, 2, False, "lane", 2, 0), (4, 4, 65, 3, True, "pair", 1, 3), (2, 2, 130, 5, True, "lane", 0, 0)]


def small_problem(n, m, N, E, herm):
    c = make_case(7300 + n, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(7301)
    return c, dict(O=cplx(rng, 3, n, m), xdot=rng.standard_normal((c["K"], N)), u=rng.standard_normal((c["K"], N)),
                   w=rng.uniform(0.2, 1.5, (3, N + 1)), blocks=gc.psd_blocks(rng, E, 3, N + 1), wf=rng.uniform(0.2, 1.5, E))


@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", CASES3)
def test_fused_against_the_composition_of_jvp_and_vjp(qoc, monkeypatch, n, m, N, E, herm, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, d = small_problem(n, m, N, E, herm)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        Gn = eng.observe_gnvp(c["x"], d["xdot"], d["O"], w=d["blocks"], wf=d["wf"])
        yd, Xd = eng.observe_jvp(c["x"], d["xdot"], d["O"], final=True)
        Gc = eng.observe_vjp(c["x"], d["O"], ybar=gr.apply_weights(d["blocks"], yd), xbar_final=d["wf"][:, None, None] * Xd)
    close(Gn, Gc, f"n={n} m={m} N={N} {kernel}: fused against composed")


@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", CASES3)
def test_exact_identities(qoc, monkeypatch, n, m, N, E, herm, kernel, S, W):
    """every operation is linear in xdot and in (w, wf), and a power of two commutes with rounding; the binding expands scalar
    weights into the planes (w, 0, w); shared weights are read where the per-member copies are"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, d = small_problem(n, m, N, E, herm)
    x, v, O, w, B, wf = c["x"], d["xdot"], d["O"], d["w"], d["blocks"], d["wf"]
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        f = lambda s, ws=1.0: eng.observe_gnvp(x, s * v, O, w=ws * B, wf=ws * wf)
        G1, G2, Gm, G0, Gw = f(1.0), f(2.0), f(-1.0), f(0.0), f(1.0, 2.0)
        Gs = eng.observe_gnvp(x, v, O, w=w, wf=wf)
        wm = np.broadcast_to(w, (E,) + w.shape).copy()         # the same weights repeated per member
        Gr = eng.observe_gnvp(x, v, O, w=wm, wf=wf)
        # (blocks=True: at E = 3 the shared planes (3, n_obs, N+1) have y's shape, which alone would mean scalars per member)
        Gp = eng.observe_gnvp(x, v, O, w=np.stack([w, np.zeros_like(w), w]), wf=wf, blocks=True)
        Bs = B[:, 0]                                           # member 0's blocks, shared and repeated
        Gb = eng.observe_gnvp(x, v, O, w=Bs, wf=wf, blocks=True)
        Gbr = eng.observe_gnvp(x, v, O, w=np.broadcast_to(Bs[:, None], (3, E) + Bs.shape[1:]).copy(), wf=wf)
        Gq = eng.observe_gnvp(x, v, O, w=wm, wf=wf, blocks=False)                  # scalars per member, said outright
    assert np.abs(G1).max() > 0 and np.abs(Gs).max() > 0
    assert np.array_equal(G2, 2.0 * G1) and np.array_equal(Gm, -G1) and not G0.any()
    assert np.array_equal(Gw, 2.0 * G1)
    assert np.array_equal(Gs, Gp) and np.array_equal(Gs, Gr)
    assert np.array_equal(Gb, Gbr) and not np.array_equal(Gb, Gs) and np.array_equal(Gq, Gs)


@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", CASES3)
def test_symmetric_and_positive(qoc, monkeypatch, n, m, N, E, herm, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, d = small_problem(n, m, N, E, herm)
    u, v = d["u"], d["xdot"]
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        Gv = eng.observe_gnvp(c["x"], v, d["O"], w=d["blocks"], wf=d["wf"])
        Gu = eng.observe_gnvp(c["x"], u, d["O"], w=d["blocks"], wf=d["wf"])
    uv, vu, mag = float(np.sum(u * Gv)), float(np.sum(v * Gu)), float(np.sum(np.abs(u) * np.abs(Gv)))
    print(f"n={n} m={m} N={N} {kernel}: <u, Gn v>={uv:.15e} <v, Gn u>={vu:.15e} sum |u||Gn v|={mag:.3e}")
    assert abs(uv - vu) <= PARITY_RTOL * mag
    assert float(np.sum(v * Gv)) > 0 and float(np.sum(u * Gu)) > 0


# ---- 3: invariants -------------------------------------------------------------------------------------------------------------
def gnvp_case(herm=False, E=10):
    c, O, _, _ = invariant_case(herm, E)
    rng = np.random.default_rng(7401)
    return c, O, rng.standard_normal((c["K"], c["N"])), gc.psd_blocks(rng, E, O.shape[0], c["N"] + 1), rng.uniform(0.2, 1.5, E)


def test_bitwise_call_to_call_and_eval_gnvp_eval(qoc):
    c, O, xdot, w, wf = gnvp_case()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        Ga = eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
        assert "trajectory_gnvp_kernel" in eng.kernel_names()
        F1, G1 = eng.eval(c["x"])
        assert eng.kernel_names() == names0 and "trajectory_gnvp_kernel" not in names0
        Gb = eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
        Go = eng.observe_gnvp(-c["x"], xdot, O, w=w, wf=wf)      # another call in between
        Gc = eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
    assert F1 == F0 and np.array_equal(G1, G0)
    assert np.array_equal(Ga, Gb) and np.array_equal(Ga, Gc) and not np.array_equal(Ga, Go)


@pytest.mark.parametrize("herm,E,members", [(False, 10, 4), (True, 10, 4), (True, 70, 24)])
def test_member_chunked_context_is_bitwise_the_unchunked_one(qoc, monkeypatch, herm, E, members):
    c, O, xdot, w, wf = gnvp_case(herm, E)
    with engine(qoc, c) as eng:
        Gd = eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, herm, members)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < E and eng.info["member_chunk"] % 32 != 0, eng.info["member_chunk"]
        Gc = eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
    assert np.array_equal(Gc, Gd)


@pytest.mark.parametrize("standing", ["running_cost", "penalties", "risk"])
def test_standing_costs_do_not_enter(qoc, standing):
    c, O, xdot, w, wf = gnvp_case()
    with engine(qoc, c) as eng:
        Gd = eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
        F0, _ = eng.eval(c["x"])
        if standing == "running_cost":
            eng.set_running_cost(c["R"], c["rho"])
        elif standing == "penalties":
            eng.set_penalties(np.array([0.3, 0.1]), np.array([0.05, 0.2]))
        else:
            eng.set_risk(2.0)
        F1, _ = eng.eval(c["x"])
        Gs = eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
        F2, _ = eng.eval(c["x"])
    assert F1 != F0 and F2 == F1                              # the cost is in force, before and after
    assert np.array_equal(Gs, Gd)


def test_scratch_is_counted_in_workspace_bytes(qoc):
    c, O, xdot, w, wf = gnvp_case()
    with engine(qoc, c) as eng:
        eng.observe_vjp(c["x"], O, ybar=np.ones((c["E"], O.shape[0], c["N"] + 1), complex))
        eng.observe_jvp(c["x"], xdot, O)
        before = eng.info["workspace_bytes"]
        eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
        grown = eng.info["workspace_bytes"] - before
        eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
        assert eng.info["workspace_bytes"] - before == grown   # allocated once
    # at least the costate's sources: one n x m block per slice and member
    assert grown >= 16 * c["E"] * c["N"] * c["n"] * c["m"], grown


# ---- 4: coordinates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["basis", "bounds", "both"])
def test_operator_is_wrapped_by_the_pulse_map(qoc, mode):
    """Gn under a pulse map = Phi' s (J' W J) s Phi applied to thetadot: the reference operator on the physical pulse along
    s * (thetadot phi'), then the slope and the projection"""
    c = make_case(7501, 4, 2, 50, 3, hermitian=False)
    N, K, E = c["N"], c["K"], c["E"]
    rng = np.random.default_rng(7502)
    O, w, wf = cplx(rng, 2, 4, 2), gc.psd_blocks(rng, E, 2, N + 1), rng.uniform(0.2, 1.5, E)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
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
            eng.set_bounds(lo, hi)                               # (bounds are served)
        x = eng.controls(theta)
        Gn = eng.observe_gnvp(theta, thetadot, O, w=w, wf=wf)
        names = eng.kernel_names()
    assert Gn.shape == theta.shape and "trajectory_gnvp_kernel" in names, names
    assert ("bounds_tangent_kernel" if mode == "bounds" else "basis_expand_kernel") in names, names
    slope = np.ones_like(a)
    if mode != "basis":
        mid, half = (0.5 * (lo + hi))[:, None], (0.5 * (hi - lo))[:, None]
        slope = 1.0 - np.tanh((a - mid) / half) ** 2
    want = slope * gr.gnvp_ref(c["A"], c["B"], c["Xi"], x, slope * adot, c["T"], O, w, wf, False, c["variant"])
    if mode != "bounds":
        want = want @ phi
    close(Gn, want, mode + ": Gn")


# ---- 5: the device form -------------------------------------------------------------------------------------------------------
def planes_cm(w, E, n_obs, N):
    """(w_per_member, planes as the library reads them) of scalar weights or planes, shared or per member"""
    w = np.asarray(w, float)
    if w.shape in ((n_obs, N + 1), (E, n_obs, N + 1)):
        w = np.stack([w, np.zeros_like(w), w])
    return (1 if w.ndim == 4 else 0), np.ascontiguousarray(w)


def gnvp_dev(torch, eng, x, xdot, O, w, wf, per_member=False, stream=0, reuse=False, cols=None):
    """observe_gnvp_device on CUDA tensors -> Gn (K, cols) as numpy, after a synchronise; x=None with reuse"""
    cols = cols or eng._cols
    n_obs = 0 if (O is None or w is None) else (O.shape[1] if per_member else O.shape[0])
    xd = None if reuse else dev(torch, np.asarray(x).T)
    xdd = dev(torch, np.asarray(xdot).T)
    Od = dev(torch, _probes_cm(O, per_member)) if n_obs else None
    wpm, wd = 0, None
    if w is not None:
        wpm, planes = planes_cm(w, eng.E, n_obs, eng.N)
        wd = dev(torch, planes)
    wfd = None if wf is None else dev(torch, np.asarray(wf, float))
    G = torch.full((cols, eng.K), float("nan"), dtype=torch.float64, device="cuda")
    eng.observe_gnvp_device(ptr(xd), ptr(xdd), n_obs, per_member, ptr(Od), wpm, ptr(wd), ptr(wfd), ptr(G), stream)
    torch.cuda.synchronize()
    return np.ascontiguousarray(G.cpu().numpy().T)


@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", CASES3)
def test_device_form_is_bitwise_the_host_form(qoc, torch, monkeypatch, n, m, N, E, herm, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, d = small_problem(n, m, N, E, herm)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        for w, wf in ((d["blocks"], d["wf"]), (d["w"], None), (None, d["wf"])):
            Gh = eng.observe_gnvp(c["x"], d["xdot"], d["O"] if w is not None else None, w=w, wf=wf)
            Gd = gnvp_dev(torch, eng, c["x"], d["xdot"], d["O"], w, wf)
            names = eng.kernel_names()
            assert "trajectory_gnvp_kernel" in names and swept(names), names
            Gr = gnvp_dev(torch, eng, None, d["xdot"], d["O"], w, wf, reuse=True)
            names = eng.kernel_names()
            assert "trajectory_gnvp_kernel" in names and "vjp_sum_kernel" in names and not swept(names), names
            assert np.array_equal(Gd, Gh) and np.array_equal(Gr, Gh)


@pytest.mark.parametrize("herm", [False, True])
def test_reuse_behind_the_other_device_forms(qoc, torch, herm):
    """observe_device / jvp_device leave the trajectory: gnvp_device(NULL) runs along it with no sweep, keeps the flag, and a
    vjp_device(NULL) still works behind it"""
    c, O, xdot, w, wf = gnvp_case(herm)
    rng = np.random.default_rng(7601)
    yb, xb = cplx(rng, c["E"], O.shape[0], c["N"] + 1), cplx(rng, c["E"], c["n"], c["m"])
    with engine(qoc, c) as eng:
        Gh = eng.observe_gnvp(c["x"], xdot, O, w=w, wf=wf)
        Gv = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        observe_dev(torch, eng, c["x"], O, False)
        G1 = gnvp_dev(torch, eng, None, xdot, O, w, wf, reuse=True)
        names = eng.kernel_names()
        assert not swept(names) and "trajectory_gnvp_kernel" in names, names
        jvp_dev(torch, eng, c["x"], xdot, O, False)
        G2 = gnvp_dev(torch, eng, None, xdot, O, w, wf, reuse=True)
        assert not swept(eng.kernel_names())
        G3 = gnvp_dev(torch, eng, None, 2.0 * xdot, O, w, wf, reuse=True)      # again, another direction: a CG loop
        Gr = vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)
        assert not swept(eng.kernel_names())
    assert np.array_equal(G1, Gh) and np.array_equal(G2, Gh) and np.array_equal(G3, 2.0 * Gh) and np.array_equal(Gr, Gv)


def reuse_refused(torch, qoc, eng, O, xdot, wf, word=None):
    G = torch.zeros((eng._cols, eng.K), dtype=torch.float64, device="cuda")
    with pytest.raises(qoc.GrapeError) as ei:
        eng.observe_gnvp_device(0, ptr(dev(torch, xdot.T)), 0, False, 0, 0, 0, ptr(dev(torch, wf)), ptr(G))
    assert ei.value.status == -5 and "reuse" in str(ei.value) and "grape_eval_gnvp_device" in str(ei.value), str(ei.value)
    if word:
        assert word in str(ei.value), str(ei.value)


def test_reuse_is_refused_without_a_trajectory(qoc, torch, monkeypatch):
    c, O, xdot, w, wf = gnvp_case()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        reuse_refused(torch, qoc, eng, O, xdot, wf)            # a fresh context (one eval, no device form)
        touches = (lambda: eng.set_penalties(0.1, 0.2), lambda: eng.set_operators(c["A"], c["B"], c["Xi"], c["Xt"], c["wts"]),
                   lambda: eng.set_trajectory_derivative("first_order"))
        for touch in touches:
            Gd = gnvp_dev(torch, eng, c["x"], xdot, O, w, wf)
            touch()
            reuse_refused(torch, qoc, eng, O, xdot, wf)
            reuse_refused(torch, qoc, eng, O, xdot, wf)        # (a refused call leaves the flag clear)
        eng.set_penalties(None, None)
        F, G = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G, G0)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, False, 4)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < c["E"]
        Gc = gnvp_dev(torch, eng, c["x"], xdot, O, w, wf)      # member-chunked: the unchunked bits
        assert np.array_equal(Gc, Gd)
        reuse_refused(torch, qoc, eng, O, xdot, wf, "member_chunk")


# ---- 6: refusals and arguments -----------------------------------------------------------------------------------------------
def raw_call(qoc, eng, x, xdot, n_obs, per_member, O, wpm, wy, wf, Gn):
    lib = qoc.load_library()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.grape_eval_gnvp(eng._h, p(x), p(xdot), n_obs, per_member, p(O), wpm, p(wy), p(wf), p(Gn))
    return rc, lib.grape_last_error(eng._h).decode()


def test_refusals(qoc):
    c = make_case(7701, 4, 4, 20, 2)
    GE = qoc.GrapeError

    def refused(eng, case, word, x=None):
        x = case["x"] if x is None else x
        F0, G0 = eng.eval(x)                                  # the bits from before the refusal
        with pytest.raises(GE) as ei:
            eng.observe_gnvp(x, np.ones_like(x), None, wf=np.ones(case["E"]))
        assert ei.value.status == -2 and word in str(ei.value) and "grape_eval_gnvp" in str(ei.value), str(ei.value)
        F, G = eng.eval(x)
        assert F == F0 and np.array_equal(G, G0)

    big = make_case(7707, 5, 5, 8, 1)
    with engine(qoc, big) as eng:
        refused(eng, big, "dimension")
    for sys_type in ("StateTransfer", "CoherenceTransfer"):
        with qoc.GrapeEngine(sys_type, c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], T, 20) as eng:
            refused(eng, c, "StateTransfer")
    with engine(qoc, c, gradient="exact") as eng:
        refused(eng, c, "exact")
    with engine(qoc, c, gradient="exact", objective="c1") as eng:      # (objective = c1 exists on gradient = exact contexts only)
        refused(eng, c, "exact")
    with engine(qoc, c, force_collective=True) as eng:
        refused(eng, c, "communicator")
    with engine(qoc, c) as eng:                                # the refusal of this call alone
        eng.set_trajectory_derivative("exact")
        refused(eng, c, "trajectory_derivative")
        eng.set_trajectory_derivative("first_order")
        eng.set_bounds(np.array([-0.8, -0.5]), np.array([0.9, 0.6]))          # bounds are NOT refused
        assert eng.observe_gnvp(0.3 * c["x"], np.ones_like(c["x"]), None, wf=np.ones(2)).any()


def test_invalid_arguments(qoc):
    c = make_case(7801, 4, 4, 20, 2)
    E, N, K = c["E"], c["N"], c["K"]
    rng = np.random.default_rng(7802)
    O = cplx(rng, 2, 4, 4)
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])

        def same_bits():
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)

        xf = np.ascontiguousarray(c["x"].T)
        xdf = np.ascontiguousarray(rng.standard_normal((N, K)))
        Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
        wy, wym, wf = gc.psd_blocks(rng, 2, N + 1), gc.psd_blocks(rng, E, 2, N + 1), rng.uniform(0.2, 1.5, E)
        Gn = np.empty((N, K))
        bad_args = [
            (None, xdf, 2, 0, Of, 0, wy, wf, Gn),             # null x
            (xf, None, 2, 0, Of, 0, wy, wf, Gn),              # null xdot
            (xf, xdf, 2, 0, Of, 0, wy, wf, None),             # null Gn
            (xf, xdf, 2, 0, Of, 0, None, None, Gn),           # both weights NULL
            (xf, xdf, 2, 0, Of, 2, wy, wf, Gn), (xf, xdf, 2, 0, Of, -1, wy, wf, Gn),      # w_per_member other than 0 or 1
            (xf, xdf, 0, 0, Of, 0, wy, wf, Gn),               # n_obs = 0 with a non-NULL wy
            (xf, xdf, -1, 0, Of, 0, wy, wf, Gn), (xf, xdf, 17, 0, Of, 0, wy, wf, Gn),     # n_obs outside 0..16
            (xf, xdf, 2, 0, None, 0, wy, wf, Gn),             # n_obs > 0 with a NULL O
            (xf, xdf, 2, 2, Of, 0, wy, wf, Gn),               # per_member other than 0 or 1
        ]
        for args in bad_args:
            rc, msg = raw_call(qoc, eng, *args)
            assert rc == -1 and "grape_eval_gnvp" in msg, (rc, msg)
            same_bits()
        names = ["O[", "xdot[", "wy[", "wf["]
        for which in range(4):                                # NaN, then inf, in every host array
            for bad in (np.nan, np.inf):
                arrs = [Of.copy(), xdf.copy(), wy.copy(), wf.copy()]
                arrs[which].reshape(-1)[1] = bad
                rc, msg = raw_call(qoc, eng, xf, arrs[1], 2, 0, arrs[0], 0, arrs[2], arrs[3], Gn)
                assert rc == -1 and "not finite" in msg and names[which] in msg, (rc, msg)
            same_bits()
        for args in ((2, 0, Of, 0, wy, wf), (2, 0, Of, 0, wy, None), (2, 0, Of, 1, wym, wf), (2, 0, Of, 0, None, wf),
                     (0, 0, None, 0, None, wf)):             # every valid NULL combination
            rc, msg = raw_call(qoc, eng, xf, xdf, *args, Gn)
            assert rc == 0, msg
        same_bits()
        # the Python layer catches wrong shapes before the library is called
        for call in (lambda: eng.observe_gnvp(c["x"], xdf.T[:, :5], O, w=wy), lambda: eng.observe_gnvp(c["x"], xdf.T, O),
                     lambda: eng.observe_gnvp(c["x"], xdf.T, None, w=wy), lambda: eng.observe_gnvp(c["x"], xdf.T, O, w=wy[:, :1]),
                     lambda: eng.observe_gnvp(c["x"], xdf.T, O, w=wy, wf=wf[:1])):
            with pytest.raises(ValueError):
                call()
    # before grape_set_operators
    lib = qoc.load_library()
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.grape_eval_gnvp(h, p(xf), p(xdf), 2, 0, p(Of), 0, p(wy), None, p(Gn)) == -5
        assert b"operators not set" in lib.grape_last_error(h)
    finally:
        lib.grape_destroy(h)


# ---- 7: the Levenberg-Marquardt loop, end to end -----------------------------------------------------------------------------------
def test_fit_trajectory_tracks_the_curve_of_a_known_pulse(qoc):
    """y_target = y(x*), start x* + 0.1 randn.  The loss never rises over accepted iterates; "fused" and "composed" give the
    same first accepted step; the final loss is at most 10x that of the same loop driven by the NumPy operator (the factor
    covers CG paths that part at rounding level) -- a bar measured in the test, not fixed in advance."""
    from quoptimalcontrol_jl_amd import gauss_newton as gn
    c = make_case(7901, 2, 1, 12, 2, K=2, hermitian=True)
    rng = np.random.default_rng(7902)
    O = cplx(rng, 3, 2, 1)
    w = rng.uniform(0.5, 1.5, (3, 13))
    x_star = c["x"]
    x0 = x_star + 0.1 * rng.standard_normal(x_star.shape)
    # 24 unknowns.  The steps of two operators that agree to rounding can be compared only where CG CONVERGES: a truncated CG
    # iterate is not a continuous function of the operator at rounding level (its Lanczos basis loses orthogonality as soon as
    # a Ritz value has converged), the solution of the damped system is -- to cond * cg_rtol, and lam0 = 0.1 under an operator
    # of norm < 100 bounds cond by 1e3, so by 1e-9 of the step.  Later iterations relax lam and may stop at cg_iter.
    kw = dict(max_iter=10, cg_iter=60, lam0=0.1, cg_rtol=1e-12)
    with engine(qoc, c) as eng:
        y_target = eng.observe(x_star, O)
        fused = gn.fit_trajectory(eng, x0, O, y_target, w=w, operator="fused", **kw)
        composed = gn.fit_trajectory(eng, x0, O, y_target, w=w, operator="composed", **kw)
        by_ref = gn.fit_trajectory(eng, x0, O, y_target, w=w, **kw, operator=lambda x: (
            lambda v: gr.gnvp_ref(c["A"], c["B"], c["Xi"], x, v, c["T"], O, w, None, False, c["variant"])))
    for res in (fused, composed, by_ref):
        assert res["accepted"] >= 1 and all(b < a for a, b in zip(res["losses"], res["losses"][1:])), res["losses"]
    step = fused["steps"][0]
    dstep = np.linalg.norm(step - composed["steps"][0])
    print(f"losses: start {fused['losses'][0]:.3e}; fused {fused['loss']:.3e} composed {composed['loss']:.3e} "
          f"reference-driven {by_ref['loss']:.3e}; first steps differ by {dstep:.3e} of {np.linalg.norm(step):.3e}")
    assert dstep <= 1e-8 * np.linalg.norm(step)
    assert fused["loss"] < fused["losses"][0]
    assert fused["loss"] <= 10.0 * by_ref["loss"] and composed["loss"] <= 10.0 * by_ref["loss"]
