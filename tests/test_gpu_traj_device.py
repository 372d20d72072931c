"""grape_eval_observables_device / grape_eval_vjp_device on the GPU: the device-resident forms of the trajectory read-out and
its vector-Jacobian product.  The oracle is bit-for-bit identity with the host forms (which tests/test_gpu_observe.py and
tests/test_gpu_vjp.py hold to the NumPy references at the parity bar), for the direct and the staged instance of each kernel,
over the shapes that reach every edge of the decomposition; then the reuse of the stored trajectory, the compositions, the
refusals, and torch.autograd on CUDA tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_observe import close as obs_close, probes, ref as obs_ref  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_vjp import COMBOS, cplx, invariant_case, shape_problem  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5
ROWS = [r[:9] for r in SHAPES]                                # (n, m, N, E, hermitian, variant, kernel, S, W)
SWEEPS = ("sweep_small_kernel", "sweep_pair_kernel")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _cm(a):
    return np.ascontiguousarray(np.swapaxes(np.asarray(a, dtype=np.complex128), -1, -2))


def _probes_cm(O, per_member):
    return _cm(np.swapaxes(O, 0, 1) if per_member else O)     # column-major (n, m, [E,] n_obs)


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return 0 if t is None else t.data_ptr()


def observe_dev(torch, eng, x, O, per_member, final=True, stream=0, xd=None):
    """observe_device on fresh CUDA tensors -> (y (E, n_obs, N+1), X_final (E, n, m), fg row), as numpy, after a synchronise"""
    E, n, m, N, K = eng.E, eng.n, eng.m, eng.N, eng.K
    n_obs = 0 if O is None else (O.shape[1] if per_member else O.shape[0])
    xd = dev(torch, np.asarray(x).T) if xd is None else xd
    Od = None if O is None else dev(torch, _probes_cm(O, per_member))
    y = torch.full((E, n_obs, N + 1), float("nan"), dtype=torch.complex128, device="cuda") if n_obs else None
    Xf = torch.full((E, m, n), float("nan"), dtype=torch.complex128, device="cuda") if final else None
    fg = torch.full((xd.numel() + 1,), float("nan"), dtype=torch.float64, device="cuda")
    eng.observe_device(ptr(xd), n_obs, per_member, ptr(Od), ptr(y), ptr(Xf), ptr(fg), stream)
    torch.cuda.synchronize()
    return (None if y is None else y.cpu().numpy(), None if Xf is None else np.ascontiguousarray(np.swapaxes(Xf.cpu().numpy(), -1, -2)),
            fg.cpu().numpy())


def vjp_dev(torch, eng, x, O, yb, xb, per_member, stream=0, reuse=False, cols=None):
    """observe_vjp_device -> G (K, cols) as numpy, after a synchronise; x=None with reuse"""
    cols = cols or eng._cols
    n_obs = 0 if (O is None or yb is None) else (O.shape[1] if per_member else O.shape[0])
    xd = None if reuse else dev(torch, np.asarray(x).T)
    Od = dev(torch, _probes_cm(O, per_member)) if n_obs else None
    ybd = dev(torch, yb)
    xbd = None if xb is None else dev(torch, _cm(xb))
    G = torch.full((cols, eng.K), float("nan"), dtype=torch.float64, device="cuda")
    eng.observe_vjp_device(ptr(xd), n_obs, per_member, ptr(Od), ptr(ybd), ptr(xbd), ptr(G), stream)
    torch.cuda.synchronize()
    return np.ascontiguousarray(G.cpu().numpy().T)


# ---- 1: read-out, device = host ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W", ROWS)
def test_readout_is_bitwise_the_host_form(qoc, torch, monkeypatch, n, m, N, E, herm, variant, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    rng = np.random.default_rng(N + E)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        xd = dev(torch, c["x"].T)
        row = torch.empty(c["K"] * N + 1, dtype=torch.float64, device="cuda")
        eng.eval_device(xd.data_ptr(), row.data_ptr())
        torch.cuda.synchronize()
        row = row.cpu().numpy()
        for n_obs in (1, 3, 16):
            for per_member in (False, True):
                O = probes(rng, c, n_obs, per_member)
                y, Xf, F = eng.observe(c["x"], O, per_member=per_member, final=True, want_F=True)
                assert "observe_kernel" in eng.kernel_names()
                for staged in ("0", "1"):
                    monkeypatch.setenv("GRAPE_TRAJ_STAGED", staged)
                    yd, Xd, fg = observe_dev(torch, eng, c["x"], O, per_member)
                    names = eng.kernel_names()
                    what = f"n={n} m={m} N={N} E={E} n_obs={n_obs} per_member={per_member} staged={staged}"
                    assert ("observe_staged_kernel" if staged == "1" else "observe_kernel") in names, (what, names)
                    assert ("observe_kernel" if staged == "1" else "observe_staged_kernel") not in names, (what, names)
                    assert np.array_equal(yd, y) and np.array_equal(Xd, Xf), what
                    assert fg[-1] == F and np.array_equal(fg, row), what
                monkeypatch.delenv("GRAPE_TRAJ_STAGED")


def test_readout_against_the_numpy_reference(qoc, torch, monkeypatch):
    """(a sanity anchor: the host form is held to this reference over every row)"""
    n, m, N, E, herm, variant, kernel, S, W = ROWS[9]
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    monkeypatch.setenv("GRAPE_TRAJ_STAGED", "1")
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    O = probes(np.random.default_rng(3), c, 3, False)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        yd, Xd, _ = observe_dev(torch, eng, c["x"], O, False)
        assert "observe_staged_kernel" in eng.kernel_names()
    y_ref, X_ref = obs_ref(c, O, False)
    obs_close(yd, y_ref, "device y")
    obs_close(Xd, X_ref, "device X_final", min_scale=0.0)


# ---- 2: VJP, device = host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W", ROWS)
def test_vjp_is_bitwise_the_host_form(qoc, torch, monkeypatch, n, m, N, E, herm, variant, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, O_mem, O_sh, cots = shape_problem(n, m, N, E, herm, variant)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        for (n_obs, pm, which), (yb, xb) in zip(COMBOS, cots):
            ops = O_mem[:, :n_obs] if pm else O_sh[:n_obs]
            G = eng.observe_vjp(c["x"], ops, ybar=yb, xbar_final=xb, per_member=bool(pm))
            for staged in ("0", "1"):
                monkeypatch.setenv("GRAPE_TRAJ_STAGED", staged)
                Gd = vjp_dev(torch, eng, c["x"], ops, yb, xb, bool(pm))
                names = eng.kernel_names()
                what = f"n={n} m={m} N={N} E={E} n_obs={n_obs} per_member={pm} {which} staged={staged}"
                want = "trajectory_vjp_staged_kernel" if staged == "1" and yb is not None else "trajectory_vjp_kernel"
                other = "trajectory_vjp_kernel" if want == "trajectory_vjp_staged_kernel" else "trajectory_vjp_staged_kernel"
                assert want in names and other not in names and "vjp_sum_kernel" in names, (what, names)
                assert np.array_equal(Gd, G), what
            monkeypatch.delenv("GRAPE_TRAJ_STAGED")


# ---- 3: the LDS budget -----------------------------------------------------------------------------------------------------------
def test_a_block_beyond_the_budget_runs_direct(qoc, torch, monkeypatch):
    """N = 130: one probe row is 131 * 16 = 2 096 B, three are 6 288 B; the budget is 4 096 B"""
    n, m, N, E, herm, variant = 3, 2, 130, 3, True, 1
    c, O_mem, O_sh, _ = shape_problem(n, m, N, E, herm, variant)
    rng = np.random.default_rng(31)
    monkeypatch.setenv("GRAPE_TRAJ_STAGED", "1")
    monkeypatch.setenv("GRAPE_TRAJ_LDS_BYTES", "4096")
    with engine(qoc, c, slices_per_lane=1, waves_per_member=3) as eng:
        for n_obs, staged in ((1, True), (3, False)):
            O, yb = O_sh[:n_obs], cplx(rng, E, n_obs, N + 1)
            y, Xf = eng.observe(c["x"], O, final=True)
            G = eng.observe_vjp(c["x"], O, ybar=yb)
            yd, Xd, _ = observe_dev(torch, eng, c["x"], O, False)
            assert ("observe_staged_kernel" in eng.kernel_names()) == staged and ("observe_kernel" in eng.kernel_names()) != staged
            Gd = vjp_dev(torch, eng, c["x"], O, yb, None, False)
            assert ("trajectory_vjp_staged_kernel" in eng.kernel_names()) == staged
            assert ("trajectory_vjp_kernel" in eng.kernel_names()) != staged
            assert np.array_equal(yd, y) and np.array_equal(Xd, Xf) and np.array_equal(Gd, G)


# ---- 4: reuse --------------------------------------------------------------------------------------------------------------------
def reuse_refused(torch, qoc, eng, O, yb, word=None):
    G = torch.zeros((eng._cols, eng.K), dtype=torch.float64, device="cuda")
    with pytest.raises(qoc.GrapeError) as ei:
        eng.observe_vjp_device(0, O.shape[0], False, ptr(dev(torch, _probes_cm(O, False))), ptr(dev(torch, yb)), 0, ptr(G))
    assert ei.value.status == -5 and "reuse" in str(ei.value), str(ei.value)
    if word:
        assert word in str(ei.value), str(ei.value)


@pytest.mark.parametrize("herm", [False, True])
@pytest.mark.parametrize("staged", ["0", "1"])
def test_reuse_of_the_stored_trajectory(qoc, torch, monkeypatch, herm, staged):
    monkeypatch.setenv("GRAPE_TRAJ_STAGED", staged)
    c, O, yb, xb = invariant_case(herm)
    with engine(qoc, c) as eng:
        G = vjp_dev(torch, eng, c["x"], O, yb, xb, False)
        assert any(k in eng.kernel_names() for k in SWEEPS)
        Gr = vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)         # behind a VJP with x
        names = eng.kernel_names()
        assert not any(k in names for k in SWEEPS) and "vjp_sum_kernel" in names, names
        assert ("trajectory_vjp_staged_kernel" if staged == "1" else "trajectory_vjp_kernel") in names
        assert np.array_equal(Gr, G)
        observe_dev(torch, eng, c["x"], O, False)
        Gr = vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)         # behind a read-out
        assert not any(k in eng.kernel_names() for k in SWEEPS)
        Gr2 = vjp_dev(torch, eng, None, O[:2], yb[:, :2], None, False, reuse=True)      # again, other cotangents
        assert np.array_equal(Gr, G) and np.array_equal(Gr2, eng.observe_vjp(c["x"], O[:2], ybar=yb[:, :2]))


def test_reuse_is_refused_without_a_trajectory(qoc, torch, monkeypatch):
    c, O, yb, xb = invariant_case()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])

        def same_bits():
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)

        reuse_refused(torch, qoc, eng, O, yb)                 # a fresh context (one eval, no device form)
        same_bits()
        for touch in (lambda: eng.eval(c["x"]), lambda: eng.set_penalties(0.1, 0.2), lambda: eng.observe(c["x"], O),
                      lambda: eng.fom(c["x"]), lambda: eng.observe_vjp(c["x"], O, ybar=yb)):
            observe_dev(torch, eng, c["x"], O, False)
            touch()
            reuse_refused(torch, qoc, eng, O, yb)
            reuse_refused(torch, qoc, eng, O, yb)             # (a refused call leaves the flag clear)
        eng.set_penalties(None, None)
        same_bits()
        G = vjp_dev(torch, eng, c["x"], O, yb, xb, False)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, False, 4)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < c["E"]
        F0, G0 = eng.eval(c["x"])
        assert np.array_equal(vjp_dev(torch, eng, c["x"], O, yb, xb, False), G)
        reuse_refused(torch, qoc, eng, O, yb, "member_chunk")
        F, G1 = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G1, G0)


# ---- 5: composition ----------------------------------------------------------------------------------------------------------------
def test_composition_with_every_standing_setting(qoc, torch):
    c = make_case(4401, 4, 2, 50, 3, hermitian=False, J=2, rho_kind="mixed")
    N, K = c["N"], c["K"]
    rng = np.random.default_rng(4402)
    O, yb, xb = cplx(rng, 2, 4, 2), cplx(rng, 3, 2, N + 1), cplx(rng, 3, 4, 2)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    assert phi.shape == (N, 5)
    theta = 0.4 * rng.standard_normal((K, 5))
    with engine(qoc, c) as eng:
        eng.set_penalties(np.array([0.3, 0.1]), np.array([0.05, 0.2]))
        eng.set_running_cost(c["R"], c["rho"])
        eng.set_basis(phi, 0.2 * rng.standard_normal((K, N)))
        eng.set_bounds(np.array([-0.8, -0.5]), np.array([0.9, 0.6]))
        y, Xf, F = eng.observe(theta, O, final=True, want_F=True)
        F0, G0 = eng.eval(theta)
        G = eng.observe_vjp(theta, O, ybar=yb, xbar_final=xb)
        assert G.shape == (K, 5) and F0 == F
        yd, Xd, fg = observe_dev(torch, eng, theta, O, False)
        names = eng.kernel_names()
        assert "running_cost_kernel" in names and "basis_expand_kernel" in names and "basis_project_kernel" in names, names
        assert np.array_equal(yd, y) and np.array_equal(Xd, Xf)
        assert fg[-1] == F and np.array_equal(fg[:-1].reshape(5, K).T, G0)
        Gr = vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)
        names = eng.kernel_names()
        assert not any(k in names for k in SWEEPS) and "basis_project_kernel" in names and "basis_expand_kernel" not in names, names
        Gd = vjp_dev(torch, eng, theta, O, yb, xb, False)
        assert np.array_equal(Gd, G) and np.array_equal(Gr, G)
        F1, G1 = eng.eval(theta)
        assert F1 == F0 and np.array_equal(G1, G0)
        eng.set_basis(None)                                   # bounds alone: the slope kernel
        u = 0.7 * rng.standard_normal((K, N))
        G = eng.observe_vjp(u, O, ybar=yb, xbar_final=xb)
        Gd = vjp_dev(torch, eng, u, O, yb, xb, False)
        Gr = vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)
        assert "bounds_slope_kernel" in eng.kernel_names()
        assert np.array_equal(Gd, G) and np.array_equal(Gr, G)


# ---- 6: member chunks --------------------------------------------------------------------------------------------------------------
# (the members' rows are summed in groups of 32 consecutive members: blocks of 4 of 10 members split one group three ways,
# blocks of 24 of 70 cut through every group)
@pytest.mark.parametrize("herm,E,members", [(False, 10, 4), (True, 70, 24)])
@pytest.mark.parametrize("staged", ["0", "1"])
def test_member_chunked_context_gives_the_unchunked_host_bits(qoc, torch, monkeypatch, herm, E, members, staged):
    c, O, yb, xb = invariant_case(herm, E)
    with engine(qoc, c) as eng:
        G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        y, Xf = eng.observe(c["x"], O, final=True)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, herm, members)))
    monkeypatch.setenv("GRAPE_TRAJ_STAGED", staged)
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < E and eng.info["member_chunk"] % 32 != 0, eng.info["member_chunk"]
        yd, Xd, _ = observe_dev(torch, eng, c["x"], O, False)
        assert ("observe_staged_kernel" if staged == "1" else "observe_kernel") in eng.kernel_names()
        Gd = vjp_dev(torch, eng, c["x"], O, yb, xb, False)
    assert np.array_equal(yd, y) and np.array_equal(Xd, Xf) and np.array_equal(Gd, G)


# ---- 7: a non-default stream -------------------------------------------------------------------------------------------------------
def test_on_a_side_stream_behind_the_producer_of_x(qoc, torch):
    c, O, yb, xb = invariant_case()
    with engine(qoc, c) as eng:
        y, Xf = eng.observe(c["x"], O, final=True)
        G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        half = dev(torch, 0.5 * c["x"].T)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            xd = half + half                                  # produced on the side stream (0.5 x + 0.5 x = x exactly)
            yd, Xd, _ = observe_dev(torch, eng, None, O, False, stream=side.cuda_stream, xd=xd)
            Od, ybd, xbd = dev(torch, _probes_cm(O, False)), dev(torch, yb), dev(torch, _cm(xb))
            Gt = torch.empty((eng.N, eng.K), dtype=torch.float64, device="cuda")
            Gr = torch.empty_like(Gt)
            xd2 = half + half
            eng.observe_vjp_device(xd2.data_ptr(), 4, False, Od.data_ptr(), ybd.data_ptr(), xbd.data_ptr(), Gt.data_ptr(), side.cuda_stream)
            eng.observe_vjp_device(0, 4, False, Od.data_ptr(), ybd.data_ptr(), xbd.data_ptr(), Gr.data_ptr(), side.cuda_stream)
            side.synchronize()
        F0, G0 = eng.eval(c["x"])                             # a blocking call behind the device calls
    assert np.array_equal(yd, y) and np.array_equal(Xd, Xf)
    assert np.array_equal(Gt.cpu().numpy().T, G) and np.array_equal(Gr.cpu().numpy().T, G)
    assert np.isfinite(F0) and np.isfinite(G0).all()


# ---- 8: refusals and arguments -----------------------------------------------------------------------------------------------------
def raw(qoc, eng, which, *args):
    lib = qoc.load_library()
    fn = lib.grape_eval_observables_device if which == "obs" else lib.grape_eval_vjp_device
    rc = fn(eng._h, *[C.c_void_p(a) if i not in (1, 2) else a for i, a in enumerate(args)], None)
    return rc, lib.grape_last_error(eng._h).decode()


def test_refusals(qoc, torch):
    c = make_case(4501, 4, 4, 20, 2)
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")       # (nothing is read or written: the refusal comes first)
    p = buf.data_ptr()

    def refused(eng, case, word, obs=True, vjp_word=None):
        F0, G0 = eng.eval(case["x"])                          # the bits from before the refusal
        for which, args in (("obs", (p, 0, 0, 0, 0, p, 0)), ("vjp", (p, 0, 0, 0, 0, p, p))):
            if which == "obs" and not obs:
                continue
            rc, msg = raw(qoc, eng, which, *args)
            assert rc == -2 and (vjp_word if which == "vjp" and vjp_word else word) in msg and "_device" in msg, (which, rc, msg)
        F, G = eng.eval(case["x"])
        assert F == F0 and np.array_equal(G, G0)

    for nbad in (5, 1):
        big = make_case(4502 + nbad, nbad, nbad, 8, 1)
        with engine(qoc, big) as eng:
            refused(eng, big, "dimension")
    for sys_type in ("StateTransfer", "CoherenceTransfer"):
        with qoc.GrapeEngine(sys_type, c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], T, 20) as eng:
            refused(eng, c, "StateTransfer", obs=False)
    with engine(qoc, c, gradient="exact") as eng:
        refused(eng, c, "exact")
    with engine(qoc, c, gradient="exact", objective="c1") as eng:
        refused(eng, c, "c1", vjp_word="exact")
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
        bad = [("obs", (p, 2, 0, p, 0, 0, 0)),                # d_y and d_X_final both null
               ("obs", (p, 17, 0, p, p, p, 0)), ("obs", (p, -1, 0, p, p, p, 0)),
               ("obs", (p, 2, 2, p, p, p, 0)),                # per_member = 2
               ("obs", (0, 2, 0, p, p, p, 0)),                # null d_x: the read-out has no reuse
               ("obs", (p, 0, 0, 0, p, p, 0)), ("obs", (p, 2, 0, 0, p, p, 0)),
               ("vjp", (p, 2, 0, p, p, p, 0)),                # null d_G
               ("vjp", (p, 2, 0, p, 0, 0, p)), ("vjp", (p, 17, 0, p, p, p, p)), ("vjp", (p, 2, 2, p, p, p, p)),
               ("vjp", (p, 0, 0, 0, p, p, p)), ("vjp", (p, 2, 0, 0, p, p, p))]
        for which, args in bad:
            rc, msg = raw(qoc, eng, which, *args)
            assert rc == -1 and "_device" in msg, (which, args, rc, msg)
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)
        assert "both null" in raw(qoc, eng, "obs", *bad[0][1])[1] and "n_obs = 17" in raw(qoc, eng, "obs", *bad[1][1])[1]
        assert "per_member = 2" in raw(qoc, eng, "obs", *bad[3][1])[1] and "G is null" in raw(qoc, eng, "vjp", *bad[7][1])[1]
        for call in (lambda: eng.observe_device(p, 17, False, p, p, p), lambda: eng.observe_device(p, 2, False, p, 0, 0),
                     lambda: eng.observe_vjp_device(p, 2, False, p, p, p, 0), lambda: eng.observe_vjp_device(0, 2, False, p, 0, 0, p)):
            with pytest.raises(ValueError):
                call()
    lib = qoc.load_library()                                  # before grape_set_operators
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        v = C.c_void_p(p)
        assert lib.grape_eval_observables_device(h, v, 2, 0, v, v, None, None, None) == -5
        assert b"operators not set" in lib.grape_last_error(h)
        assert lib.grape_eval_vjp_device(h, v, 2, 0, v, v, None, v, None) == -5
    finally:
        lib.grape_destroy(h)


# ---- 9: non-finite device entries are not checked ----------------------------------------------------------------------------------
def test_nan_in_device_ybar_propagates(qoc, torch):
    c, O, yb, xb = invariant_case()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        bad = yb.copy()
        bad[3, 1, 17] = np.nan
        G = vjp_dev(torch, eng, c["x"], O, bad, xb, False)    # status 0
        assert np.isnan(G).any()
        F, G1 = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G1, G0)
        assert np.array_equal(vjp_dev(torch, eng, c["x"], O, yb, xb, False), eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb))


# ---- 10: torch.autograd on CUDA tensors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_member", [False, True])
def test_autograd_linear_loss_is_bitwise_the_cpu_path(qoc, torch, per_member):
    """l = Re sum c y + Re sum d X_final: the cotangents are conj(c), conj(d) exactly on both devices"""
    from quoptimalcontrol_jl_amd import autograd
    c, O, _, _ = invariant_case()
    E, n, m, N = c["E"], c["n"], c["m"], c["N"]
    rng = np.random.default_rng(5101)
    ops = cplx(rng, E, 3, n, m) if per_member else O[:3]
    cy, dx = cplx(rng, E, 3, N + 1), cplx(rng, E, n, m)
    with engine(qoc, c) as eng:
        x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
        y, XN = autograd.trajectory(eng, x, ops, per_member=per_member)
        ((torch.from_numpy(cy) * y).real.sum() + (torch.from_numpy(dx) * XN).real.sum()).backward()
        want = x.grad.numpy()
        for reuse in (True, False):
            xc = torch.tensor(c["x"], dtype=torch.float64, device="cuda", requires_grad=True)
            yc, XNc = autograd.trajectory_device(eng, xc, ops, per_member=per_member, reuse=reuse)
            assert yc.is_cuda and XNc.is_cuda and yc.shape == (E, 3, N + 1) and XNc.shape == (E, n, m)
            assert np.array_equal(yc.detach().cpu().numpy(), y.detach().numpy())
            assert np.array_equal(XNc.detach().cpu().numpy(), XN.detach().numpy())
            ((dev(torch, cy) * yc).real.sum() + (dev(torch, dx) * XNc).real.sum()).backward()
            torch.cuda.synchronize()
            names = eng.kernel_names()
            assert any(k in names for k in SWEEPS) != reuse, (reuse, names)
            assert xc.grad.is_cuda and np.array_equal(xc.grad.cpu().numpy(), want), reuse
        # another call between forward and backward: the backward notices and runs with the saved x
        xc = torch.tensor(c["x"], dtype=torch.float64, device="cuda", requires_grad=True)
        yc = autograd.trajectory_device(eng, xc, ops, per_member=per_member, final=False)
        eng.eval(-c["x"])
        (dev(torch, cy) * yc).real.sum().backward()
        xg = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
        (torch.from_numpy(cy) * autograd.trajectory(eng, xg, ops, per_member=per_member, final=False)).real.sum().backward()
        assert np.array_equal(xc.grad.cpu().numpy(), xg.grad.numpy())


def test_adam_on_a_log_barrier_leakage_loss_on_the_gpu(qoc, torch):
    """The loss of tests/test_gpu_vjp.py's last test, on a CUDA parameter.  torch's CPU and GPU elementwise maths may differ
    in the last bits and G is linear in the cotangents: the gradients agree at the parity bar relative to max |G|."""
    from quoptimalcontrol_jl_amd import autograd
    N, mu = 40, 0.5
    c = make_case(4701, 3, 1, N, 1)
    c["Xi"] = np.array([[[1.0], [0.0], [0.0]]], complex)
    c["Xt"] = np.array([[[0.0], [1.0], [0.0]]], complex)
    ops = np.array([[[0.0], [1.0], [0.0]], [[0.0], [0.0], [1.0]]], complex)

    def loss_of(y):
        return 1.0 - y[0, 0, N].abs() ** 2 - mu / N * torch.log(1.0 - y[0, 1].abs() ** 2).sum()

    with engine(qoc, c) as eng:
        xh = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
        loss_of(autograd.trajectory(eng, xh, ops, final=False)).backward()
        G = xh.grad.numpy()
        x = torch.tensor(c["x"], dtype=torch.float64, device="cuda", requires_grad=True)
        opt = torch.optim.Adam([x], lr=0.03)
        losses = []
        for step in range(8):
            opt.zero_grad()
            loss = loss_of(autograd.trajectory_device(eng, x, ops, final=False))
            loss.backward()
            if step == 0:
                err = np.abs(x.grad.cpu().numpy() - G).max()
                print(f"log-barrier gradient, GPU against CPU autograd: |dG|_inf={err:.2e} |G|_inf={np.abs(G).max():.2e}")
                assert err <= PARITY_RTOL * np.abs(G).max()
            losses.append(float(loss.detach()))
            opt.step()
        losses.append(float(loss_of(autograd.trajectory_device(eng, x.detach(), ops, final=False))))
    print("log-barrier leakage loss over eight Adam steps on the GPU:", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0]
