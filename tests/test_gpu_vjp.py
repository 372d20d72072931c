"""grape_eval_vjp on the GPU: the vector-Jacobian product of the trajectory read-out against the NumPy / SciPy reference of
tests/vjp_reference.py (expm per slice, states by a loop, the first-order gradient from the O(N^2) double sum -- no costate
recursion), at the project's parity bar relative to max |G_ref|; against the shipped running-cost kernel; its invariants,
coordinates, refusals, and torch.autograd end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vjp_reference as vr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5


def cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def close(G, G_ref, what):
    gmax = np.abs(G_ref).max()
    err = np.abs(np.asarray(G) - G_ref).max()
    assert gmax > 0 and err <= PARITY_RTOL * gmax, f"{what}: |G-G_ref|_inf={err:.3e} > {PARITY_RTOL * gmax:.3e}"
    return err / gmax


# ---- 1: parity ---------------------------------------------------------------------------------------------------------------
# n_obs x per_member x (ybar only, Xbar only, both): G is linear in the cotangents, so ONE pass of the double sum per shape
# serves all 18 -- the probes are stacked as 32 per-member ones (16 per member, then 16 shared ones repeated for every
# member) and each combination's ybar is zero outside the probes it uses
COMBOS = [(n_obs, pm, which) for n_obs in (1, 3, 16) for pm in (0, 1) for which in ("ybar", "xbar", "both")]
_REF = {}


def shape_problem(n, m, N, E, herm, variant):
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    rng = np.random.default_rng(7000 + 100 * n + 10 * m + N + E)
    O_mem, O_sh = cplx(rng, E, 16, n, m), cplx(rng, 16, n, m)
    cots = [(cplx(rng, E, n_obs, N + 1) if which != "xbar" else None, cplx(rng, E, n, m) if which != "ybar" else None)
            for n_obs, pm, which in COMBOS]
    return c, O_mem, O_sh, cots


def shape_reference(key, c, O_mem, O_sh, cots):
    if key not in _REF:
        E, N = c["E"], c["N"]
        O_all = np.concatenate([O_mem, np.broadcast_to(O_sh, (E,) + O_sh.shape)], axis=1)
        ybars = np.zeros((len(COMBOS), E, 32, N + 1), complex)
        xbars = np.zeros((len(COMBOS), E, c["n"], c["m"]), complex)
        for r, ((n_obs, pm, which), (yb, xb)) in enumerate(zip(COMBOS, cots)):
            if yb is not None:
                ybars[r, :, (0 if pm else 16):(0 if pm else 16) + n_obs] = yb
            if xb is not None:
                xbars[r] = xb
        G = vr.vjp_ref_many(c["A"], c["B"], c["Xi"], c["x"], c["T"], O_all, ybars, xbars, c["variant"])
        G.setflags(write=False)
        _REF[key] = G
    return _REF[key]


@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W,J,rho_kind", SHAPES)
def test_parity_against_the_double_sum_reference(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, J, rho_kind):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, O_mem, O_sh, cots = shape_problem(n, m, N, E, herm, variant)
    ref = shape_reference((n, m, N, E, herm, variant), c, O_mem, O_sh, cots)
    worst = 0.0
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        for r, ((n_obs, pm, which), (yb, xb)) in enumerate(zip(COMBOS, cots)):
            ops = O_mem[:, :n_obs] if pm else O_sh[:n_obs]
            G = eng.observe_vjp(c["x"], ops, ybar=yb, xbar_final=xb, per_member=bool(pm))
            assert G.shape == (c["K"], N)
            worst = max(worst, close(G, ref[r], f"n={n} m={m} N={N} E={E} n_obs={n_obs} per_member={pm} {which}"))
        names = eng.kernel_names()
    print(f"n={n} m={m} N={N} E={E} {kernel}: worst relG over {len(COMBOS)} cotangent sets {worst:.2e}")
    assert "trajectory_vjp_kernel" in names and "vjp_sum_kernel" in names


def index_case():
    c = make_case(4101, 3, 2, 23, 2, hermitian=False)
    rng = np.random.default_rng(4102)
    return c, cplx(rng, 3, 3, 2), rng


def test_ybar_at_s0_contributes_nothing(qoc):
    c, O, rng = index_case()
    ybar = np.zeros((2, 3, 24), complex)
    ybar[:, :, 0] = cplx(rng, 2, 3)
    with engine(qoc, c, slices_per_lane=2) as eng:
        G = eng.observe_vjp(c["x"], O, ybar=ybar)
    assert G.shape == (2, 23) and not G.any()                 # exactly zero


def test_ybar_at_one_interior_slice(qoc):
    c, O, rng = index_case()
    s = 9
    ybar = np.zeros((2, 3, 24), complex)
    ybar[:, :, s] = cplx(rng, 2, 3)
    ref = vr.vjp_ref(c["A"], c["B"], c["Xi"], c["x"], T, O, ybar, None, False, c["variant"])
    with engine(qoc, c, slices_per_lane=2) as eng:
        G = eng.observe_vjp(c["x"], O, ybar=ybar)
    close(G, ref, "ybar at s = 9")
    assert G[:, :s].all() and not G[:, s:].any()              # slices t >= s cannot see the state after s slices


def test_ybar_at_the_last_slice_is_an_xbar(qoc):
    c, O, rng = index_case()
    ybar = np.zeros((2, 3, 24), complex)
    ybar[:, :, 23] = cplx(rng, 2, 3)
    xbar = np.einsum("kj,jab->kab", ybar[:, :, 23], O)
    ref = vr.vjp_ref(c["A"], c["B"], c["Xi"], c["x"], T, O, ybar, None, False, c["variant"])
    with engine(qoc, c, slices_per_lane=2) as eng:
        Gy = eng.observe_vjp(c["x"], O, ybar=ybar)
        Gx = eng.observe_vjp(c["x"], None, xbar_final=xbar)
    close(Gy, ref, "ybar at s = N")
    close(Gx, ref, "the same thing as Xbar")
    close(Gx, Gy, "Xbar against ybar")


# ---- 2: against the shipped running-cost kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,E,herm,kernel", [(4, 4, 65, 3, True, "pair"), (3, 1, 64, 3, False, "lane"), (2, 2, 130, 5, True, "lane")])
def test_reproduces_the_running_cost_kernel(qoc, monkeypatch, n, m, N, E, herm, kernel):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(4200 + 10 * n + m, n, m, N, E, hermitian=herm, J=3, rho_kind="mixed")
    O = np.swapaxes(c["R"], 0, 1)                             # (E, J, n, m)
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        y = eng.observe(c["x"], O, per_member=True)
        ybar = np.zeros_like(y)
        ybar[:, :, 1:] = 2.0 * c["wts"][:, None, None] * c["rho"][None] * y[:, :, 1:]
        G = eng.observe_vjp(c["x"], O, ybar=ybar, per_member=True)
        eng.set_running_cost(c["R"], c["rho"])
        F1, G1 = eng.eval(c["x"])
    GJ = G1 - G0
    assert np.abs(GJ).max() >= 1e-3 * np.abs(G1).max(), (np.abs(GJ).max(), np.abs(G1).max())     # the term is visible
    close(G, GJ, f"n={n} m={m} {kernel}: vjp(2 w rho y) against eval with the running cost minus eval without")


# ---- 3: invariants -------------------------------------------------------------------------------------------------------------
def invariant_case(herm=False, E=10):
    c = make_case(4301 + herm + E, 3, 3, 40, E, hermitian=herm, J=2)
    rng = np.random.default_rng(4303)
    return c, cplx(rng, 4, 3, 3), cplx(rng, E, 4, 41), cplx(rng, E, 3, 3)


def test_bitwise_call_to_call_and_eval_vjp_eval(qoc):
    c, O, yb, xb = invariant_case()
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        Ga = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        assert "trajectory_vjp_kernel" in eng.kernel_names()
        F1, G1 = eng.eval(c["x"])
        assert eng.kernel_names() == names0 and "trajectory_vjp_kernel" not in names0
        Gb = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        Gother = eng.observe_vjp(-c["x"], O, ybar=yb)         # another call in between
        Gc = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
    assert F1 == F0 and np.array_equal(G1, G0)
    assert np.array_equal(Ga, Gb) and np.array_equal(Ga, Gc) and not np.array_equal(Ga, Gother)


# (the members' rows are summed in groups of 32 consecutive members: blocks of 4 of 10 members split one group three ways,
# blocks of 24 of 70 cut through every group)
@pytest.mark.parametrize("herm,E,members", [(False, 10, 4), (True, 10, 4), (True, 70, 24)])
def test_member_chunked_context_is_bitwise_the_unchunked_one(qoc, monkeypatch, herm, E, members):
    c, O, yb, xb = invariant_case(herm, E)
    with engine(qoc, c) as eng:
        G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, herm, members)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < E and eng.info["member_chunk"] % 32 != 0, eng.info["member_chunk"]
        Gc = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
    assert np.array_equal(Gc, G)


@pytest.mark.parametrize("standing", ["running_cost", "penalties", "risk"])
def test_standing_costs_do_not_enter(qoc, standing):
    c, O, yb, xb = invariant_case()
    with engine(qoc, c) as eng:
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
        F2, _ = eng.eval(c["x"])
    assert F1 != F0 and F2 == F1                              # the cost is in force, before and after
    assert np.array_equal(Gs, G)


# ---- 4: coordinates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["basis", "bounds", "both"])
def test_gradient_comes_back_in_the_coordinates_of_x(qoc, mode):
    c = make_case(4401, 4, 2, 50, 3, hermitian=False)
    N, K = c["N"], c["K"]
    rng = np.random.default_rng(4402)
    O, yb, xb = cplx(rng, 2, 4, 2), cplx(rng, 3, 2, N + 1), cplx(rng, 3, 4, 2)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    assert phi.shape == (N, 5)
    x0 = 0.2 * rng.standard_normal((K, N))
    lo, hi = np.array([-0.8, -0.5]), np.array([0.9, 0.6])
    with engine(qoc, c) as eng:
        if mode != "bounds":
            eng.set_basis(phi, x0)
            theta = 0.4 * rng.standard_normal((K, 5))
            a = x0 + theta @ phi.T
        else:
            theta = 0.7 * rng.standard_normal((K, N))
            a = theta
        if mode != "basis":
            eng.set_bounds(lo, hi)
        x = eng.controls(theta)
        G = eng.observe_vjp(theta, O, ybar=yb, xbar_final=xb)
        y_map, X_map = eng.observe(theta, O, final=True)
    with engine(qoc, c) as eng:
        G_plain = eng.observe_vjp(x, O, ybar=yb, xbar_final=xb)
        y_plain, X_plain = eng.observe(x, O, final=True)
    assert np.array_equal(y_map, y_plain) and np.array_equal(X_map, X_plain)      # the pair agrees on the pulse
    want = G_plain
    if mode != "basis":
        mid, half = (0.5 * (lo + hi))[:, None], (0.5 * (hi - lo))[:, None]
        slope = 1.0 - np.tanh((a - mid) / half) ** 2
        want = want * slope
    if mode != "bounds":
        want = want @ phi
    assert G.shape == want.shape == ((K, N) if mode == "bounds" else (K, 5))
    close(G, want, mode)


# ---- 5: refusals and arguments -----------------------------------------------------------------------------------------------
def raw_call(qoc, eng, x, n_obs, per_member, O, ybar, Xbar, G):
    lib = qoc.load_library()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.grape_eval_vjp(eng._h, ptr(x), n_obs, per_member, ptr(O), ptr(ybar), ptr(Xbar), ptr(G))
    return rc, lib.grape_last_error(eng._h).decode()


def test_refusals(qoc):
    c = make_case(4501, 4, 4, 20, 2)
    GE = qoc.GrapeError

    def refused(eng, case, word):
        F0, G0 = eng.eval(case["x"])                          # the bits from before the refusal
        with pytest.raises(GE) as ei:
            eng.observe_vjp(case["x"], None, xbar_final=np.ones_like(case["Xi"]))
        assert ei.value.status == -2 and word in str(ei.value), str(ei.value)
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
        Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
        yb, Xb, G = cplx(rng, E, 2, N + 1), cplx(rng, E, 4, 4), np.empty((N, K))
        bad_args = [
            (None, 2, 0, Of, yb, Xb, G),                      # null x
            (xf, 2, 0, Of, yb, Xb, None),                     # null G
            (xf, 2, 0, Of, None, None, G),                    # ybar and Xbar_final both NULL
            (xf, -1, 0, Of, yb, Xb, G), (xf, 17, 0, Of, yb, Xb, G),       # n_obs outside 0..16
            (xf, 0, 0, Of, yb, Xb, G),                        # n_obs = 0 with a non-NULL ybar
            (xf, 2, 0, None, yb, Xb, G),                      # n_obs > 0 with a NULL O
            (xf, 2, 2, Of, yb, Xb, G), (xf, 2, -1, Of, yb, Xb, G),        # per_member other than 0 or 1
        ]
        for args in bad_args:
            rc, msg = raw_call(qoc, eng, *args)
            assert rc == -1 and "grape_eval_vjp" in msg, (rc, msg)
            same_bits()
        for which in range(3):                                # a non-finite entry of O, ybar, Xbar_final
            arrs = [Of.copy(), yb.copy(), Xb.copy()]
            arrs[which].reshape(-1)[5] = [np.nan, np.inf, complex(0, -np.inf)][which]
            rc, msg = raw_call(qoc, eng, xf, 2, 0, arrs[0], arrs[1], arrs[2], G)
            assert rc == -1 and "not finite" in msg and ["O[", "ybar[", "Xbar_final["][which] in msg, (rc, msg)
            same_bits()
        with pytest.raises(GE) as ei:
            eng.observe_vjp(c["x"], O, ybar=np.where(np.arange(E * 2 * (N + 1)).reshape(E, 2, N + 1) == 0, np.nan, yb))
        assert ei.value.status == -1 and "not finite" in str(ei.value)      # (ybar[0, ., .] is validated although it is unused)
        # valid corners: Xbar_final alone with n_obs = 0; ybar alone
        rc, msg = raw_call(qoc, eng, xf, 0, 0, None, None, Xb, G)
        assert rc == 0, msg
        rc, msg = raw_call(qoc, eng, xf, 2, 0, Of, yb, None, G)
        assert rc == 0, msg
        # the Python layer catches wrong shapes before the library is called
        for kw in (dict(ops=O, ybar=yb[:, :1]), dict(ops=O, xbar_final=Xb[:, :3]), dict(ops=None, ybar=yb), dict(ops=O),
                   dict(ops=np.zeros((17, 4, 4)), ybar=np.zeros((E, 17, N + 1)))):
            with pytest.raises(ValueError):
                eng.observe_vjp(c["x"], **kw)
        with pytest.raises(ValueError):
            eng.observe_vjp(c["x"][:, :5], O, ybar=yb)
        # a NaN in x gives NaN out and no error
        xn = c["x"].copy()
        xn[1, 7] = np.nan
        assert np.isnan(eng.observe_vjp(xn, O, ybar=yb)).any()
        same_bits()
    # before grape_set_operators
    lib = qoc.load_library()
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.grape_eval_vjp(h, p(xf), 2, 0, p(Of), p(yb), None, p(G)) == -5
        assert b"operators not set" in lib.grape_last_error(h)
    finally:
        lib.grape_destroy(h)


# ---- 6: torch, end to end ------------------------------------------------------------------------------------------------------
def test_adam_on_a_log_barrier_leakage_loss_written_in_torch(qoc):
    """A qutrit held as a ket, |0> -> |1>, level 2 to be avoided: l = 1 - |<1|psi_N>|^2 - (mu / N) sum_s log(1 - |<2|psi_s>|^2),
    written in torch on autograd.trajectory's y.  x.grad is observe_vjp of the cotangents computed by hand,
    ybar_0[N] = -2 y_0[N] and ybar_1[s] = (2 mu / N) y_1[s] / (1 - |y_1[s]|^2): torch's own cotangents differ from these in
    the last bits only and G is linear in them, so the two gradients agree to 1e-12 of max |G| (four orders above the
    double-precision rounding of a 40-slice product, two below the parity bar).  Eight Adam steps must lower the loss."""
    import torch
    from quoptimalcontrol_jl_amd import autograd
    N, mu = 40, 0.5
    c = make_case(4701, 3, 1, N, 1)
    c["Xi"] = np.array([[[1.0], [0.0], [0.0]]], complex)
    c["Xt"] = np.array([[[0.0], [1.0], [0.0]]], complex)
    ops = np.array([[[0.0], [1.0], [0.0]], [[0.0], [0.0], [1.0]]], complex)

    def loss_of(y):
        return 1.0 - y[0, 0, N].abs() ** 2 - mu / N * torch.log(1.0 - y[0, 1].abs() ** 2).sum()

    with engine(qoc, c) as eng:
        x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
        opt = torch.optim.Adam([x], lr=0.03)
        losses = []
        for step in range(8):
            opt.zero_grad()
            y, _ = autograd.trajectory(eng, x, ops)
            loss = loss_of(y)
            loss.backward()
            if step == 0:
                assert "trajectory_vjp_kernel" in eng.kernel_names()
                yn = y.detach().numpy()
                ybar = np.zeros_like(yn)
                ybar[0, 0, N] = -2.0 * yn[0, 0, N]
                ybar[0, 1] = 2.0 * mu / N * yn[0, 1] / (1.0 - np.abs(yn[0, 1]) ** 2)
                G = eng.observe_vjp(c["x"], ops, ybar=ybar)
                assert np.abs(x.grad.numpy() - G).max() <= 1e-12 * np.abs(G).max()
            losses.append(float(loss.detach()))
            opt.step()
        y, _ = autograd.trajectory(eng, x.detach(), ops)
        losses.append(float(loss_of(y)))
    print("log-barrier leakage loss over eight Adam steps:", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0]
