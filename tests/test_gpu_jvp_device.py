"""grape_eval_jvp_device on the GPU: the device-resident form of the Jacobian-vector product of the trajectory read-out.  The
oracle is bit-for-bit identity with the host form (which tests/test_gpu_jvp.py holds to the NumPy reference at the parity
bar); then the reuse of the stored trajectory, the Gauss-Newton chain with the other two device forms, the pulse maps, the
refusals, and torch forward-mode AD on CUDA tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_traj_device import _probes_cm, dev, observe_dev, ptr, vjp_dev  # noqa: E402
from test_gpu_vjp import cplx, invariant_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5
ROWS = [r[:9] for r in SHAPES]                                # (n, m, N, E, hermitian, variant, kernel, S, W)


def swept(names):
    """a sweep kernel ran (sweep_small_kernel, sweep_pair_kernel, sweep_pair_vec_kernel, ...)"""
    return any(k.startswith("sweep_") for k in names)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def jvp_dev(torch, eng, x, xdot, O, per_member, final=True, stream=0, reuse=False):
    """observe_jvp_device on NaN-filled CUDA tensors -> (ydot (E, n_obs, N+1), Xdot_final (E, n, m)) as numpy, after a
    synchronise; x=None with reuse"""
    E, n, m, N = eng.E, eng.n, eng.m, eng.N
    n_obs = 0 if O is None else (O.shape[1] if per_member else O.shape[0])
    xd = None if reuse else dev(torch, np.asarray(x).T)
    xdd = dev(torch, np.asarray(xdot).T)
    Od = None if O is None else dev(torch, _probes_cm(O, per_member))
    yd = torch.full((E, n_obs, N + 1), float("nan"), dtype=torch.complex128, device="cuda") if n_obs else None
    Xd = torch.full((E, m, n), float("nan"), dtype=torch.complex128, device="cuda") if final else None
    eng.observe_jvp_device(ptr(xd), ptr(xdd), n_obs, per_member, ptr(Od), ptr(yd), ptr(Xd), stream)
    torch.cuda.synchronize()
    return (None if yd is None else yd.cpu().numpy(),
            None if Xd is None else np.ascontiguousarray(np.swapaxes(Xd.cpu().numpy(), -1, -2)))


def jvp_case(herm=False, E=10):
    c, O, yb, xb = invariant_case(herm, E)
    return c, O, yb, xb, np.random.default_rng(5401).standard_normal((c["K"], c["N"]))


# ---- 1: device = host ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W", ROWS)
def test_jvp_is_bitwise_the_host_form(qoc, torch, monkeypatch, n, m, N, E, herm, variant, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    rng = np.random.default_rng(N + E)
    xdot = rng.standard_normal((c["K"], N))
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        for n_obs, per_member in ((1, False), (3, True), (16, False)):
            O = cplx(rng, E, n_obs, n, m) if per_member else cplx(rng, n_obs, n, m)
            yh, Xh = eng.observe_jvp(c["x"], xdot, O, per_member=per_member, final=True)
            yd, Xd = jvp_dev(torch, eng, c["x"], xdot, O, per_member)
            names = eng.kernel_names()
            what = f"n={n} m={m} N={N} E={E} n_obs={n_obs} per_member={per_member}"
            assert "trajectory_jvp_kernel" in names and swept(names), (what, names)
            assert np.array_equal(yd, yh) and np.array_equal(Xd, Xh), what
            yr, Xr = jvp_dev(torch, eng, None, xdot, O, per_member, reuse=True)
            names = eng.kernel_names()
            assert "trajectory_jvp_kernel" in names and not swept(names), (what, names)
            assert np.array_equal(yr, yh) and np.array_equal(Xr, Xh), what


# ---- 2: reuse and the Gauss-Newton chain -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("herm", [False, True])
def test_chain_observe_jvp_vjp_along_one_stored_trajectory(qoc, torch, herm):
    """observe_device -> jvp_device(NULL) -> vjp_device(NULL): the bits of the three calls with d_x, one sweep in all"""
    c, O, yb, xb, xdot = jvp_case(herm)
    with engine(qoc, c) as eng:
        y1, X1, _ = observe_dev(torch, eng, c["x"], O, False)
        yd1, Xd1 = jvp_dev(torch, eng, c["x"], xdot, O, False)
        G1 = vjp_dev(torch, eng, c["x"], O, yb, xb, False)
        y, Xf, _ = observe_dev(torch, eng, c["x"], O, False)
        assert swept(eng.kernel_names())
        yd, Xd = jvp_dev(torch, eng, None, xdot, O, False, reuse=True)
        names = eng.kernel_names()
        assert not swept(names) and "trajectory_jvp_kernel" in names, names
        G = vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)
        names = eng.kernel_names()
        assert not swept(names) and "vjp_sum_kernel" in names, names
        yd2 = jvp_dev(torch, eng, None, 2.0 * xdot, O[:2], False, final=False, reuse=True)[0]     # again, another direction
        assert np.array_equal(yd2, 2.0 * yd[:, :2])
        assert np.array_equal(G, eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb))
    assert np.array_equal(y, y1) and np.array_equal(Xf, X1)
    assert np.array_equal(yd, yd1) and np.array_equal(Xd, Xd1) and np.array_equal(G, G1)


def reuse_refused(torch, qoc, eng, O, xdot, word=None):
    yd = torch.zeros((eng.E, O.shape[0], eng.N + 1), dtype=torch.complex128, device="cuda")
    with pytest.raises(qoc.GrapeError) as ei:
        eng.observe_jvp_device(0, ptr(dev(torch, xdot.T)), O.shape[0], False, ptr(dev(torch, _probes_cm(O, False))), ptr(yd), 0)
    assert ei.value.status == -5 and "reuse" in str(ei.value) and "grape_eval_jvp_device" in str(ei.value), str(ei.value)
    if word:
        assert word in str(ei.value), str(ei.value)


def test_reuse_is_refused_without_a_trajectory(qoc, torch, monkeypatch):
    c, O, yb, xb, xdot = jvp_case()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])

        def same_bits():
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)

        reuse_refused(torch, qoc, eng, O, xdot)               # a fresh context (one eval, no device form)
        same_bits()
        for touch in (lambda: eng.eval(c["x"]), lambda: eng.set_penalties(0.1, 0.2), lambda: eng.observe_jvp(c["x"], xdot, O)):
            jvp_dev(torch, eng, c["x"], xdot, O, False)
            touch()
            reuse_refused(torch, qoc, eng, O, xdot)
            reuse_refused(torch, qoc, eng, O, xdot)           # (a refused call leaves the flag clear)
        eng.set_penalties(None, None)
        same_bits()
        yd, Xd = jvp_dev(torch, eng, c["x"], xdot, O, False)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, False, 4)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < c["E"]
        F0, G0 = eng.eval(c["x"])
        yc, Xc = jvp_dev(torch, eng, c["x"], xdot, O, False)  # member-chunked: the unchunked bits
        assert np.array_equal(yc, yd) and np.array_equal(Xc, Xd)
        reuse_refused(torch, qoc, eng, O, xdot, "member_chunk")
        F, G1 = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G1, G0)


# ---- 3: pulse maps ---------------------------------------------------------------------------------------------------------------
def test_composition_with_every_standing_setting(qoc, torch):
    c = make_case(4401, 4, 2, 50, 3, hermitian=False, J=2, rho_kind="mixed")
    N, K = c["N"], c["K"]
    rng = np.random.default_rng(4402)
    O = cplx(rng, 2, 4, 2)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    theta, thetadot = 0.4 * rng.standard_normal((K, 5)), rng.standard_normal((K, 5))
    with engine(qoc, c) as eng:
        eng.set_penalties(np.array([0.3, 0.1]), np.array([0.05, 0.2]))
        eng.set_running_cost(c["R"], c["rho"])
        eng.set_basis(phi, 0.2 * rng.standard_normal((K, N)))
        eng.set_bounds(np.array([-0.8, -0.5]), np.array([0.9, 0.6]))
        F0, G0 = eng.eval(theta)
        yh, Xh = eng.observe_jvp(theta, thetadot, O, final=True)
        yd, Xd = jvp_dev(torch, eng, theta, thetadot, O, False)
        names = eng.kernel_names()
        assert "running_cost_kernel" in names and names.count("basis_expand_kernel") == 2 and "trajectory_jvp_kernel" in names, names
        yr, Xr = jvp_dev(torch, eng, None, thetadot, O, False, reuse=True)
        names = eng.kernel_names()
        assert not swept(names) and names.count("basis_expand_kernel") == 1, names
        assert np.array_equal(yd, yh) and np.array_equal(Xd, Xh) and np.array_equal(yr, yh) and np.array_equal(Xr, Xh)
        F1, G1 = eng.eval(theta)
        assert F1 == F0 and np.array_equal(G1, G0)
        eng.set_basis(None)                                   # bounds alone: the slope-only tangent
        u, udot = 0.7 * rng.standard_normal((K, N)), rng.standard_normal((K, N))
        yh, Xh = eng.observe_jvp(u, udot, O, final=True)
        yd, Xd = jvp_dev(torch, eng, u, udot, O, False)
        yr, Xr = jvp_dev(torch, eng, None, udot, O, False, reuse=True)
        assert "bounds_tangent_kernel" in eng.kernel_names()
        assert np.array_equal(yd, yh) and np.array_equal(Xd, Xh) and np.array_equal(yr, yh) and np.array_equal(Xr, Xh)


# ---- 4: a non-default stream -------------------------------------------------------------------------------------------------------
def test_on_a_side_stream_behind_the_producer_of_xdot(qoc, torch):
    c, O, yb, xb, xdot = jvp_case()
    with engine(qoc, c) as eng:
        yh, Xh = eng.observe_jvp(c["x"], xdot, O, final=True)
        half, xd = dev(torch, 0.5 * xdot.T), dev(torch, c["x"].T)
        Od = dev(torch, _probes_cm(O, False))
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            xdd = half + half                                 # produced on the side stream (0.5 v + 0.5 v = v exactly)
            yd = torch.full((eng.E, 4, eng.N + 1), float("nan"), dtype=torch.complex128, device="cuda")
            Xd = torch.full((eng.E, eng.m, eng.n), float("nan"), dtype=torch.complex128, device="cuda")
            yr, Xr = torch.full_like(yd, float("nan")), torch.full_like(Xd, float("nan"))
            eng.observe_jvp_device(xd.data_ptr(), xdd.data_ptr(), 4, False, Od.data_ptr(), yd.data_ptr(), Xd.data_ptr(), side.cuda_stream)
            eng.observe_jvp_device(0, xdd.data_ptr(), 4, False, Od.data_ptr(), yr.data_ptr(), Xr.data_ptr(), side.cuda_stream)
            side.synchronize()
        F0, G0 = eng.eval(c["x"])                             # a blocking call behind the device calls
    for y_t, X_t in ((yd, Xd), (yr, Xr)):
        assert np.array_equal(y_t.cpu().numpy(), yh) and np.array_equal(np.swapaxes(X_t.cpu().numpy(), -1, -2), Xh)
    assert np.isfinite(F0) and np.isfinite(G0).all()


# ---- 5: refusals and arguments -----------------------------------------------------------------------------------------------------
def raw(qoc, eng, *args):
    lib = qoc.load_library()
    rc = lib.grape_eval_jvp_device(eng._h, *[C.c_void_p(a) if i not in (2, 3) else a for i, a in enumerate(args)], None)
    return rc, lib.grape_last_error(eng._h).decode()


def test_refusals(qoc, torch):
    c = make_case(4501, 4, 4, 20, 2)
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")       # (nothing is read or written: the refusal comes first)
    p = buf.data_ptr()

    def refused(eng, case, word):
        F0, G0 = eng.eval(case["x"])                          # the bits from before the refusal
        rc, msg = raw(qoc, eng, p, p, 0, 0, 0, 0, p)
        assert rc == -2 and word in msg and "grape_eval_jvp_device" in msg, (rc, msg)
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


def test_invalid_arguments(qoc, torch):
    c = make_case(4601, 4, 4, 20, 2)
    buf = torch.zeros(8192, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        bad = [(p, 0, 2, 0, p, p, p),                         # null d_xdot
               (p, p, 2, 0, p, 0, 0),                         # d_ydot and d_Xdot_final both null
               (p, p, 17, 0, p, p, p), (p, p, -1, 0, p, p, p),
               (p, p, 2, 2, p, p, p),                         # per_member = 2
               (p, p, 0, 0, 0, p, p),                         # n_obs = 0 with a non-null d_ydot
               (p, p, 2, 0, 0, p, p)]                         # n_obs > 0 with a null d_O
        for args in bad:
            rc, msg = raw(qoc, eng, *args)
            assert rc == -1 and "grape_eval_jvp_device" in msg, (args, rc, msg)
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)
        assert "xdot is null" in raw(qoc, eng, *bad[0])[1] and "both null" in raw(qoc, eng, *bad[1])[1]
        assert "n_obs = 17" in raw(qoc, eng, *bad[2])[1] and "per_member = 2" in raw(qoc, eng, *bad[4])[1]
        for call in (lambda: eng.observe_jvp_device(p, p, 17, False, p, p, p), lambda: eng.observe_jvp_device(p, p, 2, False, p, 0, 0),
                     lambda: eng.observe_jvp_device(p, 0, 2, False, p, p, p), lambda: eng.observe_jvp_device(p, p, 2, False, 0, p, p)):
            with pytest.raises(ValueError):
                call()
    lib = qoc.load_library()                                  # before grape_set_operators
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        v = C.c_void_p(p)
        assert lib.grape_eval_jvp_device(h, v, v, 2, 0, v, v, None, None) == -5
        assert b"operators not set" in lib.grape_last_error(h)
    finally:
        lib.grape_destroy(h)


def test_nan_in_device_xdot_propagates(qoc, torch):
    c, O, yb, xb, xdot = jvp_case()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        bad = xdot.copy()
        bad[1, 17] = np.nan
        yd, Xd = jvp_dev(torch, eng, c["x"], bad, O, False)   # status 0
        assert np.isnan(yd).any() and not np.isnan(yd[:, :, :18]).any()
        F, G1 = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G1, G0)


# ---- 6: torch forward mode on CUDA tensors -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_member", [False, True])
def test_forward_ad_through_trajectory_device(qoc, torch, per_member):
    """the forward_ad tangent of trajectory_device is observe_jvp's output exactly, along the stored trajectory when nothing
    has touched the engine in between; a backward that follows reuses it too"""
    import torch.autograd.forward_ad as fwad
    from quoptimalcontrol_jl_amd import autograd
    c, O, _, _, xdot = jvp_case()
    E, n, m, N = c["E"], c["n"], c["m"], c["N"]
    rng = np.random.default_rng(5801)
    ops = cplx(rng, E, 3, n, m) if per_member else O[:3]
    with engine(qoc, c) as eng:
        yh, Xh = eng.observe_jvp(c["x"], xdot, ops, per_member=per_member, final=True)
        for reuse in (True, False):
            with fwad.dual_level():
                xd = fwad.make_dual(torch.tensor(c["x"], device="cuda"), torch.tensor(xdot, device="cuda"))
                y, XN = autograd.trajectory_device(eng, xd, ops, per_member=per_member, reuse=reuse)
                torch.cuda.synchronize()
                names = eng.kernel_names()
                assert "trajectory_jvp_kernel" in names and swept(names) != reuse, (reuse, names)
                yt, Xt = fwad.unpack_dual(y).tangent, fwad.unpack_dual(XN).tangent
                assert yt.is_cuda and Xt.is_cuda
                assert np.array_equal(yt.cpu().numpy(), yh) and np.array_equal(Xt.cpu().numpy(), Xh), reuse
        # another call between forward and jvp cannot happen inside apply; a dual AND requires_grad input: both modes at once
        xr = torch.tensor(c["x"], device="cuda", requires_grad=True)
        cy = dev(torch, cplx(rng, E, 3, N + 1))
        with fwad.dual_level():
            y = autograd.trajectory_device(eng, fwad.make_dual(xr, torch.tensor(xdot, device="cuda")), ops, per_member=per_member,
                                           final=False)
            yp, yt = fwad.unpack_dual(y)
            assert np.array_equal(yt.cpu().numpy(), yh)
            (cy * yp).real.sum().backward()
            torch.cuda.synchronize()
            assert not swept(eng.kernel_names())       # forward, jvp and backward: one sweep
        want = eng.observe_vjp(c["x"], ops, ybar=cy.conj().cpu().numpy(), per_member=per_member)
        assert np.array_equal(xr.grad.cpu().numpy(), want)


def test_log_barrier_dual_number_derivative_on_the_gpu(qoc, torch):
    """the loss of tests/test_gpu_vjp.py's last test on a CUDA dual number: d loss along xdot = <x.grad from backward, xdot>
    at the parity bar (of sum |x.grad xdot|)"""
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
            xd = fwad.make_dual(torch.tensor(c["x"], device="cuda"), torch.tensor(xdot, device="cuda"))
            lt = float(fwad.unpack_dual(loss_of(autograd.trajectory_device(eng, xd, ops, final=False))).tangent)
        x = torch.tensor(c["x"], device="cuda", requires_grad=True)
        loss_of(autograd.trajectory_device(eng, x, ops, final=False)).backward()
    g = x.grad.cpu().numpy()
    want, scale = float(np.sum(g * xdot)), float(np.sum(np.abs(g * xdot)))
    print(f"log-barrier loss on the GPU: forward-mode derivative {lt:.15e}, <x.grad, xdot> {want:.15e}, scale {scale:.3e}")
    assert abs(lt - want) <= PARITY_RTOL * scale
