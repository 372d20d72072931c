"""grape_set_running_cost_derivative(GRAPE_TRAJ_EXACT) on the GPU: the exact gradient of the running cost against the NumPy /
SciPy reference of tests/rc_exact_reference.py (scipy.linalg.expm_frechet per slice, the O(N^2) double sum) added to the
oracle's ensemble result -- the first-order one on first-order contexts, the exact one on gradient = exact contexts -- at the
project's parity bar; with scaled slices; against central differences of the device's own F + J; bit identities (call to
call, the entry points, member chunks); mode 0 untouched; the trajectory pair under a standing exact cost; the compositions,
the refusals, and one optimisation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixed_norm_cases as mn  # noqa: E402
import rc_exact_reference as rxr  # noqa: E402
import rc_reference as rcr  # noqa: E402
from conftest import assert_parity  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, as_problem, engine, make_case  # noqa: E402
from test_gpu_traj_exact import SCALED, slice_squarings  # noqa: E402
from test_gpu_vjp import cplx, invariant_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5
EXACT_KERNELS = ["running_cost_exact_kernel", "traj_frechet_rows_kernel"]
EXACT_CTX_ROWS = [1, 2, 4, 6, 8, 9, 12, 13]                   # lane and pair kernels, m < n, E = 70 and E = 1


def rc_exact(eng):
    eng.set_running_cost_derivative("exact")
    assert eng.running_cost_derivative == "exact"
    return eng


def with_cost(eng, c):
    rc_exact(eng).set_running_cost(c["R"], c["rho"])
    return eng


def exact_ctx(qoc, c, objective="fom", **kw):
    return engine(qoc, c, gradient="exact", objective=objective, **kw)


# ---- the references, once per case ------------------------------------------------------------------------------------------
_RC, _OR = {}, {}


def rc_ref(key, c, x=None):
    """(J, G_J) of rc_exact_reference"""
    if key not in _RC:
        xx = c["x"] if x is None else x
        J, GJ = rxr.rc_exact_ref(c["A"], c["B"], c["Xi"], c["wts"], xx, c["T"], c["R"], c["rho"], c["variant"])
        GJ.setflags(write=False)
        _RC[key] = (J, GJ)
    return _RC[key]


def oracle_ref(oracle, key, c, kind, x=None):
    """(F, G) of the oracle: kind "first" (ensemble_eval), "fom" / "c1" (ensemble_exact with that objective)"""
    if (key, kind) not in _OR:
        xx = c["x"] if x is None else x
        if kind == "first":
            F, G = oracle.ensemble_eval("UnitaryGate", c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], xx, c["T"], c["variant"])
        else:                                                 # (the oracle's exact path takes n x n states: n x m ones zero-padded,
            E, n, m = c["Xi"].shape                           # which leaves tr(Xt' U Xi) what it is; C1 divides by n^2)
            Xi, Xt = np.zeros((E, n, n), complex), np.zeros((E, n, n), complex)
            Xi[:, :, :m], Xt[:, :, :m] = c["Xi"], c["Xt"]
            F, G = oracle.ensemble_exact("UnitaryGate", c["A"], c["B"], Xi, Xt, c["wts"], xx, c["T"], variant=c["variant"],
                                         objective=0 if kind == "fom" else 1)
        G = np.array(G)
        G.setflags(write=False)
        _OR[(key, kind)] = (float(F), G)
    return _OR[(key, kind)]


def reference(oracle, key, c, kind, x=None):
    """(F + J, G + G_J) with the term visible: its gradient is at least 1e-3 of the whole"""
    (F0, G0), (J, GJ) = oracle_ref(oracle, key, c, kind, x), rc_ref(key, c, x)
    assert np.abs(GJ).max() >= 1e-3 * np.abs(G0 + GJ).max(), (np.abs(GJ).max(), np.abs(G0 + GJ).max())
    return F0 + J, G0 + GJ


def report(what, F, G, ref):
    print(f"{what}: |dF|={abs(F - ref[0]):.2e} relG={np.abs(G - ref[1]).max() / np.abs(ref[1]).max():.2e}")


def shape_case(row):
    n, m, N, E, herm, variant, kernel, S, W, J, rho_kind = SHAPES[row]
    return make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant, J=J, rho_kind=rho_kind)


# ---- 1: parity on first-order contexts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", range(len(SHAPES)))
def test_parity_on_first_order_contexts(qoc, oracle, monkeypatch, row):
    n, m, N, E, herm, variant, kernel, S, W, J, rho_kind = SHAPES[row]
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = shape_case(row)
    ref = reference(oracle, ("shape", row), c, "first")
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        F, G = with_cost(eng, c).eval(c["x"])
        names = eng.kernel_names()
        F2, G2 = eng.eval(c["x"])
    report(f"row {row} n={n} m={m} N={N} E={E} J={J} {kernel}", F, G, ref)
    assert all(k in names for k in EXACT_KERNELS + ["running_cost_fold_kernel"]) and "running_cost_kernel" not in names, names
    assert_parity(F, G, ref[0], ref[1], n, what=f"row {row}")
    assert F2 == F and np.array_equal(G2, G)


# ---- 2: parity on gradient = exact contexts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", ["fom", "c1"])
@pytest.mark.parametrize("row", EXACT_CTX_ROWS)
def test_parity_on_exact_gradient_contexts(qoc, oracle, monkeypatch, row, objective):
    n, m, N, E, herm, variant, kernel, S, W, J, rho_kind = SHAPES[row]
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = shape_case(row)
    ref = reference(oracle, ("shape", row), c, objective)
    with exact_ctx(qoc, c, objective, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        F, G = with_cost(eng, c).eval(c["x"])
        names = eng.kernel_names()
        F2, G2 = eng.eval(c["x"])
    report(f"row {row} n={n} m={m} N={N} E={E} J={J} {kernel} exact context, {objective}", F, G, ref)
    assert all(k in names for k in EXACT_KERNELS + ["running_cost_join_kernel"]), names
    assert "running_cost_kernel" not in names and "running_cost_fold_kernel" not in names, names
    assert_parity(F, G, ref[0], ref[1], n, what=f"row {row} {objective}")
    assert F2 == F and np.array_equal(G2, G)


# ---- 3: scaled slices and mixed squarings ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,Tc,herm,kernel", SCALED)
def test_parity_on_scaled_slices(qoc, oracle, monkeypatch, n, m, N, Tc, herm, kernel):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(8200 + 10 * n + m + N, n, m, N, 2, hermitian=herm, T=Tc, J=2)
    s = slice_squarings(c)
    assert s.min() >= 2, s                                    # a test that never leaves s = 0 proves nothing
    ref = reference(oracle, ("scaled", n, m, N, herm), c, "first")
    with engine(qoc, c) as eng:
        F, G = with_cost(eng, c).eval(c["x"])
    report(f"scaled n={n} m={m} N={N} T={Tc} {kernel} s={s.min()}..{s.max()}", F, G, ref)
    assert_parity(F, G, ref[0], ref[1], n, what=f"scaled n={n} m={m} N={N}")


@pytest.mark.parametrize("n,cols,kernel,herm", [(4, None, "pair", True), (3, 2, "lane", False)])
def test_parity_on_a_pulse_whose_slices_need_different_squarings(qoc, oracle, monkeypatch, n, cols, kernel, herm):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    A, B, Xi, Xt, wts, x, Tc = mn.make_case(n, 2, 23, 3, "UnitaryGate", herm, "shuffled", 4, 8400 + n, cols=cols)
    m = Xi.shape[2]
    rng = np.random.default_rng(9800 + n)
    R = cplx(rng, 2, 3, n, m)
    R[0] = Xt
    c = dict(n=n, m=m, N=23, E=3, K=2, A=A, B=B, Xi=Xi, Xt=Xt, wts=wts, x=x, variant=0, T=Tc, R=R, rho=rng.uniform(0.1, 0.3, (2, 23)))
    s = slice_squarings(c)
    assert 0 in s and len(np.unique(s)) >= 4 and s.max() >= 4, s
    ref = reference(oracle, ("mixed", n), c, "first")
    with engine(qoc, c) as eng:
        F, G = with_cost(eng, c).eval(c["x"])
    report(f"mixed norms n={n} {kernel} s={s.min()}..{s.max()}", F, G, ref)
    assert_parity(F, G, ref[0], ref[1], n, what=f"mixed norms n={n}")


@pytest.mark.parametrize("forced", [0, 3])
@pytest.mark.parametrize("n,m,kernel,herm", [(4, 4, "pair", True), (3, 3, "lane", False), (2, 2, "pair", False)])
def test_parity_with_forced_squarings(qoc, oracle, monkeypatch, forced, n, m, kernel, herm):
    """(N = 64 at T = 0.2: the Taylor polynomial is accurate unscaled, as the sweep evaluates it under expm_squarings = 0, and
    scaled 3 times; the slice weights are of order 1 here so that the term stays visible next to F)"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(8600 + 10 * n + m, n, m, 64, 2, hermitian=herm, T=0.2, J=2)
    c["rho"] = c["rho"] * 16.0
    assert mn.slice_bounds(c["A"], c["B"], c["x"], c["T"] / 64).max() < mn.THETA8
    ref = reference(oracle, ("forced", n, m), c, "first")
    with engine(qoc, c, expm_squarings=forced) as eng:
        F, G = with_cost(eng, c).eval(c["x"])
    report(f"forced s={forced} n={n} m={m} {kernel}", F, G, ref)
    assert_parity(F, G, ref[0], ref[1], n, what=f"forced s={forced} n={n}")


# ---- 4: against central differences of the device's own F + J ----------------------------------------------------------------
def central_differences(eng, x, h=1e-5):
    g = np.empty_like(x)
    for cc in range(x.shape[0]):
        for t in range(x.shape[1]):
            d = np.zeros_like(x)
            d[cc, t] = h
            g[cc, t] = (eng.eval(x + d)[0] - eng.eval(x - d)[0]) / (2 * h)
    return g


@pytest.mark.parametrize("n,m,N,E,objective", [(4, 4, 8, 3, "c1"), (3, 1, 8, 2, "fom")])
def test_against_central_differences_of_the_devices_own_objective(qoc, n, m, N, E, objective):
    """the whole gradient of F + J on a gradient = exact context within 1e-6 of the central differences (h = 1e-5) of the same
    context's F + J; a first-order context with the first-order running cost misses that bar on the same shapes"""
    c = make_case(9900 + n, n, m, N, E, hermitian=(n == 4), J=2)
    with exact_ctx(qoc, c, objective) as eng:
        with_cost(eng, c)
        _, G = eng.eval(c["x"])
        fd = central_differences(eng, c["x"])
    with engine(qoc, c) as eng:
        eng.set_running_cost(c["R"], c["rho"])
        _, G1 = eng.eval(c["x"])
        fd1 = central_differences(eng, c["x"])
    dev_x, dev_1 = np.abs(G - fd).max() / np.abs(fd).max(), np.abs(G1 - fd1).max() / np.abs(fd1).max()
    print(f"n={n} m={m} N={N} E={E}: against central differences: exact context {dev_x:.2e}, first-order context {dev_1:.2e}")
    assert dev_x <= 1e-6, dev_x
    assert dev_1 > 1e-6, dev_1


# ---- 5: bits -------------------------------------------------------------------------------------------------------------------
def eval_on_device(torch, eng, c, x):
    d_x = torch.tensor(np.ascontiguousarray(x.T), device="cuda")
    d_fg = torch.zeros(c["K"] * c["N"] + 1, dtype=torch.float64, device="cuda")
    eng.eval_device(d_x.data_ptr(), d_fg.data_ptr())
    torch.cuda.synchronize()
    fg = d_fg.cpu().numpy()
    return fg[-1], fg[:-1].reshape(c["N"], c["K"]).T


@pytest.mark.parametrize("ctx", ["first", "exact"])
@pytest.mark.parametrize("herm", [False, True])
def test_bits_call_to_call_and_between_the_entry_points(qoc, ctx, herm):
    import torch
    c = invariant_case(herm)[0]
    kw = dict(gradient="exact", objective="c1") if ctx == "exact" else {}
    rng = np.random.default_rng(9910)
    Xs = np.array([c["x"], c["x"] + 0.1 * rng.standard_normal(c["x"].shape), -c["x"]])
    with engine(qoc, c, max_batch=3, **kw) as eng:
        with_cost(eng, c)
        single = [eng.eval(x) for x in Xs]
        F, G = eng.eval(Xs[0])                                # (other pulses in between)
        assert F == single[0][0] and np.array_equal(G, single[0][1])
        Fd, Gd = eval_on_device(torch, eng, c, Xs[1])
        assert Fd == single[1][0] and np.array_equal(Gd, single[1][1])
        F1, G1 = eng.eval_batch(Xs[1:2])                      # the one-array batch
        assert F1[0] == single[1][0] and np.array_equal(G1[0], single[1][1])
        Fb, Gb = eng.eval_batch(Xs)                           # every array its own J
        for b in range(3):
            assert Fb[b] == single[b][0] and np.array_equal(Gb[b], single[b][1]), b
        assert len({s[0] for s in single}) == 3


@pytest.mark.parametrize("ctx", ["first", "exact"])
@pytest.mark.parametrize("herm,E,members", [(False, 10, 4), (True, 10, 4), (False, 70, 24), (True, 70, 24)])
def test_member_chunked_context_is_bitwise_the_unchunked_one(qoc, monkeypatch, ctx, herm, E, members):
    c = invariant_case(herm, E)[0]
    kw = dict(gradient="exact", objective="fom") if ctx == "exact" else {}
    with engine(qoc, c, **kw) as eng:
        F, G = with_cost(eng, c).eval(c["x"])
        info = eng.info
        assert info["member_chunk"] in (0, E), info["member_chunk"]
    # room for `members` and a half members' workspace: a gradient = exact context keeps the states and the costates beside
    # the propagators whatever the generators are (n = 3: the lane kernel's debug flow)
    budget = _chunk_budget(c, info, herm, members) if ctx == "first" else 3 * _chunk_budget(c, info, True, members)
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(budget))
    with engine(qoc, c, **kw) as eng:
        assert 0 < eng.info["member_chunk"] < E, eng.info["member_chunk"]
        Fc, Gc = with_cost(eng, c).eval(c["x"])
        assert "running_cost_exact_kernel" in eng.kernel_names()
    assert Fc == F and np.array_equal(Gc, G)


# ---- 6: mode 0 is untouched ----------------------------------------------------------------------------------------------------
def test_first_order_mode_is_untouched(qoc):
    c = invariant_case()[0]
    with engine(qoc, c) as eng:                               # a context that never calls the setting
        eng.set_running_cost(c["R"], c["rho"])
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        ws0 = eng.info["workspace_bytes"]
    with engine(qoc, c) as eng:
        assert eng.running_cost_derivative == "first_order"
        eng.set_running_cost_derivative("first_order")
        eng.set_running_cost(c["R"], c["rho"])
        F1, G1 = eng.eval(c["x"])
        assert eng.kernel_names() == names0
        rc_exact(eng)
        Fx, Gx = eng.eval(c["x"])
        assert "running_cost_exact_kernel" in eng.kernel_names()
        assert eng.info["workspace_bytes"] > ws0              # the per-slice blocks are counted
        eng.set_running_cost_derivative("first_order")
        assert eng.running_cost_derivative == "first_order"
        F2, G2 = eng.eval(c["x"])
        names2 = eng.kernel_names()
    for F, G in ((F1, G1), (F2, G2)):
        assert F == F0 and np.array_equal(G, G0)
    assert names2 == names0 and "running_cost_kernel" in names0
    assert not any("exact" in k or "frechet" in k or "join" in k for k in names0), names0
    assert Fx == F0 and not np.array_equal(Gx, G0)            # J keeps its bits (F is the same sweep's), its gradient moves


# ---- 7: the trajectory pair under a standing exact running cost --------------------------------------------------------------
@pytest.mark.parametrize("traj_mode", ["first_order", "exact"])
def test_the_trajectory_pair_does_not_see_a_standing_exact_cost(qoc, traj_mode):
    c, O, yb, xb = invariant_case()
    xdot = np.random.default_rng(9920).standard_normal((c["K"], c["N"]))
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(traj_mode)
        G = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        yd, Xd = eng.observe_jvp(c["x"], xdot, O, final=True)
        F0, _ = eng.eval(c["x"])
        with_cost(eng, c)
        F1, G1 = eng.eval(c["x"])
        Gs = eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb)
        assert "running_cost_exact_kernel" in eng.kernel_names()
        yds, Xds = eng.observe_jvp(c["x"], xdot, O, final=True)
        F2, G2 = eng.eval(c["x"])
    assert F1 != F0 and F2 == F1 and np.array_equal(G2, G1)   # the cost is in force, before and after
    assert np.array_equal(Gs, G) and np.array_equal(yds, yd) and np.array_equal(Xds, Xd)


# ---- 8: composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", ["first", "c1"])
@pytest.mark.parametrize("mode", ["basis", "bounds", "both", "penalties"])
def test_results_come_back_in_the_coordinates_of_x(qoc, oracle, mode, ctx):
    from test_penalties_host import penalty_ref
    c = make_case(4401, 4, 2, 50, 3, hermitian=False, J=3, rho_kind="mixed")
    N, K = c["N"], c["K"]
    rng = np.random.default_rng(9930)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    x0 = 0.2 * rng.standard_normal((K, N))
    lo, hi = np.array([-0.8, -0.5]), np.array([0.9, 0.6])
    amp, var = np.array([0.3, 0.0]), np.array([0.1, 0.2])
    kw = dict(gradient="exact", objective="c1") if ctx == "c1" else {}
    with engine(qoc, c, **kw) as eng:
        with_cost(eng, c)
        if mode in ("basis", "both"):
            eng.set_basis(phi, x0)
            theta = 0.4 * rng.standard_normal((K, 5))
            a = x0 + theta @ phi.T
        else:
            theta = 0.7 * rng.standard_normal((K, N))
            a = theta
        if mode in ("bounds", "both"):
            eng.set_bounds(lo, hi)
        if mode == "penalties":
            eng.set_penalties(amp, var)
        x = eng.controls(theta)
        F, G = eng.eval(theta)
    slope = np.ones((K, N))
    if mode in ("bounds", "both"):
        mid, half = (0.5 * (lo + hi))[:, None], (0.5 * (hi - lo))[:, None]
        slope = 1.0 - np.tanh((a - mid) / half) ** 2
        assert np.abs(x - (mid + half * np.tanh((a - mid) / half))).max() <= 1e-14
    else:
        assert np.abs(x - a).max() <= 1e-14
    F_ref, G_ref = reference(oracle, ("compose", mode), c, ctx, x=x)
    if mode == "penalties":
        Fp, Gp = penalty_ref(x, amp, var)
        F_ref, G_ref = F_ref + Fp, G_ref + Gp
    want = G_ref * slope
    if mode in ("basis", "both"):
        want = want @ phi
    report(f"{mode} on a {ctx} context", F, G, (F_ref, want))
    assert G.shape == want.shape
    assert_parity(F, G, F_ref, want, c["n"], what=f"{mode} {ctx}")


def test_member_results_stay_without_the_cost_on_an_exact_context(qoc):
    c = make_case(9940, 4, 4, 33, 3, J=2)
    with exact_ctx(qoc, c, "c1", member_results=True) as eng:
        F0, G0 = eng.eval(c["x"])
        mem0 = eng.member_results()
        with_cost(eng, c)
        F1, G1 = eng.eval(c["x"])
        mem1 = eng.member_results()
        assert F1 != F0 and "running_cost_join_kernel" in eng.kernel_names()
        eng.set_running_cost(None)
        F2, G2 = eng.eval(c["x"])
    assert np.array_equal(mem0[0], mem1[0]) and np.array_equal(mem0[1], mem1[1])
    assert F2 == F0 and np.array_equal(G2, G0)


@pytest.mark.parametrize("ctx", ["first", "fom"])
def test_an_ensemble_with_a_zero_weight(qoc, oracle, ctx):
    c = make_case(9950, 3, 2, 20, 4, hermitian=False, J=2)
    c["wts"] = c["wts"].copy()
    c["wts"][1] = 0.0
    ref = reference(oracle, ("zero weight",), c, ctx)
    kw = dict(gradient="exact", objective="fom") if ctx == "fom" else {}
    with engine(qoc, c, **kw) as eng:
        F, G = with_cost(eng, c).eval(c["x"])
    assert np.isfinite(F) and np.isfinite(G).all()
    assert_parity(F, G, ref[0], ref[1], c["n"], what=f"zero weight, {ctx}")


# ---- 9: refusals and arguments -------------------------------------------------------------------------------------------------
def test_refusals_and_invalid_arguments(qoc):
    c = make_case(4501, 4, 4, 20, 2)
    GE = qoc.GrapeError
    lib = qoc.load_library()

    def refused(eng, case, word):
        F0, G0 = eng.eval(case["x"])
        with pytest.raises(GE) as ei:
            eng.set_running_cost_derivative("exact")
        assert ei.value.status == -2 and word in str(ei.value) and "grape_set_running_cost_derivative" in str(ei.value), str(ei.value)
        assert eng.running_cost_derivative == "first_order"
        eng.set_running_cost_derivative("first_order")        # (switching off what can never be on)
        F, G = eng.eval(case["x"])
        assert F == F0 and np.array_equal(G, G0)

    big = make_case(4507, 5, 5, 8, 1)
    with engine(qoc, big) as eng:
        refused(eng, big, "dimension")
    with qoc.GrapeEngine("StateTransfer", c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], T, 20) as eng:
        refused(eng, c, "StateTransfer")
    with engine(qoc, c, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM) as eng:
        refused(eng, c, "multi-device")
    with engine(qoc, c, force_collective=True) as eng:
        refused(eng, c, "communicator")

    def cost_refused(eng, word):
        with pytest.raises(GE) as ei:
            eng.set_running_cost(c["R"], c["rho"])
        assert ei.value.status == -2 and word in str(ei.value), str(ei.value)

    for objective in ("fom", "c1"):
        with exact_ctx(qoc, c, objective) as eng:
            F0, G0 = eng.eval(c["x"])
            cost_refused(eng, "exact")                        # before the mode is set: refused as ever
            rc_exact(eng)
            eng.set_running_cost(c["R"], c["rho"])            # ... and accepted after
            F1, G1 = eng.eval(c["x"])
            assert F1 != F0
            with pytest.raises(GE) as ei:                     # back to first order under the standing cost
                eng.set_running_cost_derivative("first_order")
            assert ei.value.status == -2 and "grape_set_running_cost_derivative" in str(ei.value)
            assert eng.running_cost_derivative == "exact"
            F2, G2 = eng.eval(c["x"])
            assert F2 == F1 and np.array_equal(G2, G1)        # the setting stayed
            for bad in (2, -1, 7):                            # mode outside {0, 1}
                assert lib.grape_set_running_cost_derivative(eng._h, bad) == -1
                assert b"grape_set_running_cost_derivative" in lib.grape_last_error(eng._h)
            eng.set_operators(c["A"], c["B"], c["Xi"], c["Xt"], c["wts"])   # both settings persist
            F3, G3 = eng.eval(c["x"])
            assert F3 == F1 and np.array_equal(G3, G1) and "running_cost_exact_kernel" in eng.kernel_names()
            eng.set_running_cost(None)                        # the cost off: the mode may go back, and the cost is refused again
            eng.set_running_cost_derivative("first_order")
            cost_refused(eng, "exact")
            F4, G4 = eng.eval(c["x"])
            assert F4 == F0 and np.array_equal(G4, G0)

    with engine(qoc, c) as eng:                               # a risk and an attached exchange are refused as before
        rc_exact(eng)
        eng.set_risk(2.0)
        cost_refused(eng, "risk")
        eng.set_risk(0.0)
        eng.set_running_cost(c["R"], c["rho"])
        with pytest.raises(GE) as ei:
            eng.set_risk(2.0)
        assert ei.value.status == -2 and "running cost" in str(ei.value)
        with pytest.raises(GE) as ei:
            eng.ipc_attach([eng.ipc_export(1)], 0, 1)
        assert ei.value.status == -2 and "running cost" in str(ei.value)
        with pytest.raises(GE) as ei:
            eng.comm_attach(bytes(128), 0, 1)
        assert ei.value.status == -2 and "running cost" in str(ei.value)
    assert lib.grape_set_running_cost_derivative(None, 1) == -1


# ---- 10: one optimisation ------------------------------------------------------------------------------------------------------
def optimisation_case():
    """a qutrit held as a ket, two members: level 2 forbidden (C5) and the evolution-time cost towards the target ket (C7)"""
    c = make_case(9960, 3, 1, 12, 2, J=2)
    e = np.eye(3, dtype=complex)
    c["Xi"] = np.array([e[:, :1]] * 2)
    c["Xt"] = np.array([e[:, 1:2]] * 2)
    c["wts"] = np.array([0.5, 0.5])
    return c


OPT_COSTS = dict(forbidden=([0, 0, 1.0], 0.8), time=0.6)


def test_lbfgs_reaches_a_stationary_point_of_the_objective_with_running_costs(qoc):
    """grape_lbfgs on (n, m, N, E) = (3, 1, 12, 2) with a C5 and a C7 term.  On the ADGRAPE-type context (gradient = exact,
    objective = c1, the running cost exact) it stops where the central-difference gradient (h = 1e-5) of the device's own
    F + J is <= 1e-6; from the same start on a first-order context with the first-order running cost it ends at a point whose
    central-difference gradient is at least 100 times larger.  solve(prob, ADGRAPE(..., running_costs=...)) runs the same
    optimisation and returns the same minimum (plus the constant of C7)."""
    c = optimisation_case()
    costs = [qoc.ForbiddenStates([OPT_COSTS["forbidden"][0]], OPT_COSTS["forbidden"][1]), qoc.EvolutionTime(OPT_COSTS["time"])]
    prob = as_problem(qoc, c)
    members = qoc.init_ensemble(prob)
    R, rho, const = qoc.api.running_cost_terms(members, costs, c["N"], c["wts"])
    opts = dict(iterations=2000, g_tol=1e-10)
    out = {}
    for kind in ("exact", "first"):
        kw = dict(gradient="exact", objective="c1", variant=1) if kind == "exact" else dict(variant=c["variant"])
        with qoc.GrapeEngine("UnitaryGate", c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], c["T"], c["N"], **kw) as eng:
            if kind == "exact":
                rc_exact(eng)
            eng.set_running_cost(R, rho)
            x_min, info = eng.lbfgs(c["x"], iterations=opts["iterations"], g_tol=opts["g_tol"])
            own = np.abs(eng.eval(x_min)[1]).max()
            fd = np.abs(central_differences(eng, x_min)).max()
        out[kind] = (fd, own, info["minimum"], info["iterations"])
        print(f"{kind}: grape_lbfgs {info['iterations']} iterations ({info['message']}), minimum {info['minimum']:.12f}, "
              f"own |g|_inf {own:.2e}, central-difference |g|_inf {fd:.2e}")
    assert out["exact"][0] <= 1e-6, out
    assert out["first"][0] >= 100.0 * out["exact"][0], out
    res = qoc.solve(prob, qoc.ADGRAPE(n_slices=c["N"], optimizer="device", optim_options=opts, running_costs=costs))
    print(f"solve(ADGRAPE): minimum {res.fidelity:.12f} (the raw run: {out['exact'][2] + const:.12f})")
    assert res.fidelity == pytest.approx(out["exact"][2] + const, abs=1e-9)
