"""grape_gn_step on the GPU: the loss, its gradient and the damped Gauss-Newton step of one call against the NumPy / SciPy reference
of tests/gn_step_reference.py (dense H, numpy.linalg.solve) and against the shipped host forms -- bit for bit where the
arithmetic is the same (unit weights), through gauss_newton._cg where it is a restatement; reproducibility, independence of the
block size, coordinates, refusals, and the Levenberg-Marquardt loop with solver="device".

Bounds: 1e-10 is the project's parity bar.  The converged solves run at cg_rtol = 1e-13 on systems of condition <= 26 (about
50 where |H|_2 is a power-iteration estimate), so the solution moves by cond * rtol < 5e-12 of its norm; one CG iteration is a
single quotient of dot products, continuous in the operator.  Longer TRUNCATED runs are not compared: see
test_fit_trajectory_tracks_the_curve_of_a_known_pulse in test_gpu_gnvp.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_step_cases as gsc  # noqa: E402
import gn_step_reference as gsr  # noqa: E402
import gnvp_cases as gc  # noqa: E402
import gnvp_reference as gr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_traj_device import dev, ptr  # noqa: E402
from test_gpu_vjp import invariant_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5
cplx = gc.cplx
FIELDS = ("loss", "predicted", "iterations", "status", "residual", "g_norm", "g_inf", "p_norm")


def step(eng, c, a, x=None, **kw):
    return eng.gn_step(c["x"] if x is None else x, a["ops"], y_target=a["y_target"], w=a["w"], xf_target=a["xf_target"], wf=a["wf"],
                       per_member=a["per_member"], **kw)


def same_bits(s1, s2):
    return np.array_equal(s1["p"], s2["p"]) and np.array_equal(s1["g"], s2["g"]) and all(
        s1[f] == s2[f] or (s1[f] != s1[f] and s2[f] != s2[f]) for f in FIELDS)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---- 1: loss and gradient --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W,J,rho_kind", SHAPES)
def test_loss_and_gradient_against_the_reference(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, J, rho_kind):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    row = (n, m, N, E, herm, variant)
    ref = gsc.loss_and_gradient(row)
    with engine(qoc, gc.shape_problem(*row)[0], slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        for call, (L, g) in ref.items():
            c, a = gsc.call_arguments(row, *call)
            s = step(eng, c, a, lam=0.3, cg_iter=0)
            gmax = np.abs(g).max()
            eL, eg = abs(s["loss"] - L), np.abs(s["g"] - g).max()
            print(f"n={n} m={m} N={N} E={E} {kernel} {call}: L={L:.6e} |dL|={eL:.3e} |g|_inf={gmax:.3e} |dg|_inf={eg:.3e}")
            assert L > 0 and eL <= PARITY_RTOL * L
            assert s["g"].shape == (c["K"], N) and gmax > 0 and eg <= PARITY_RTOL * gmax
            assert s["status"] == 1 and s["iterations"] == 0 and not s["p"].any() and s["predicted"] == 0.0
            assert abs(s["g_inf"] - gmax) <= PARITY_RTOL * gmax and abs(s["g_norm"] - np.linalg.norm(g)) <= PARITY_RTOL * s["g_norm"]


# ---- 2: bit for bit under unit weights ----------------------------------------------------------------------------------------------
CASES3 = [(3, 2, 23, 2, False, "lane", 2, 0), (4, 4, 65, 3, True, "pair", 1, 3), (2, 2, 130, 5, True, "lane", 0, 0)]


def small_problem(n, m, N, E, herm):
    c = make_case(8300 + n, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(8301)
    return c, dict(ops=cplx(rng, 3, n, m), y_target=cplx(rng, E, 3, N + 1), w=None, xf_target=cplx(rng, E, n, m), wf=None,
                   per_member=False)


@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", CASES3)
def test_unit_weights_give_the_bits_of_the_host_forms(qoc, monkeypatch, n, m, N, E, herm, kernel, S, W):
    """rr = ii = 1, ri = 0, wf = 1: any evaluation order of the cotangent gives the same bits, so g is observe_vjp of
    observe() - target bit for bit; cg_iter = 0 leaves p = 0 with status 1; at target = own read-out g = 0, status 3"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, a = small_problem(n, m, N, E, herm)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        y, Xf = eng.observe(c["x"], a["ops"], final=True)
        for has_y, has_x in ((True, True), (True, False), (False, True)):
            b = dict(a, y_target=a["y_target"] if has_y else None, xf_target=a["xf_target"] if has_x else None,
                     ops=a["ops"] if has_y else None)
            g_host = eng.observe_vjp(c["x"], b["ops"], ybar=y - a["y_target"] if has_y else None,
                                     xbar_final=Xf - a["xf_target"] if has_x else None)
            s = step(eng, c, b, lam=0.1, cg_iter=0)
            assert g_host.any() and np.array_equal(s["g"], g_host), (has_y, has_x)
            assert s["status"] == 1 and s["iterations"] == 0 and not s["p"].any()
            assert np.array_equal(step(eng, c, b, lam=0.1, cg_iter=5)["g"], g_host)
        own = dict(a, y_target=y, xf_target=Xf)
        for iters in (0, 5):
            s = step(eng, c, own, lam=0.1, cg_iter=iters)
            assert s["status"] == 3 and s["iterations"] == 0 and s["loss"] == 0.0 and not s["g"].any() and not s["p"].any()


# ---- 3: one iteration through the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [2, 6, 8, 10, "Q1", "Q65", "Q1200"])
def test_one_iteration_is_cg_on_the_engines_own_operator(qoc, monkeypatch, which):
    from quoptimalcontrol_jl_amd.gauss_newton import _cg
    sc = gsc.solve_case(which)
    c, a, lam = sc["c"], sc["args"], sc["lam"]
    kw = {}
    if not isinstance(which, str):
        monkeypatch.setenv("GRAPE_SMALL_KERNEL", SHAPES[which][6])
        kw = dict(slices_per_lane=SHAPES[which][7], waves_per_member=SHAPES[which][8])
    with engine(qoc, c, **kw) as eng:
        s = step(eng, c, a, lam=lam, cg_iter=1, cg_rtol=0.0)
        H = lambda v: eng.observe_gnvp(c["x"], v, a["ops"], w=a["w"], wf=a["wf"], per_member=a["per_member"])
        p, Ap = _cg(lambda v: H(v) + lam * v, -s["g"], 1, 0.0)
    err, size = np.linalg.norm(s["p"] - p), np.linalg.norm(p)
    print(f"{which}: Q={sc['Q']} |p - p_cg| = {err:.3e} of {size:.3e}")
    assert s["iterations"] == 1 and s["status"] == 1
    assert size > 0 and err <= 1e-10 * size
    model = -float(np.vdot(s["g"], p)) - 0.5 * (float(np.vdot(p, Ap)) - lam * float(np.vdot(p, p)))
    assert abs(s["predicted"] - model) <= 1e-10 * abs(model)


# ---- 4: converged solves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", gsc.SOLVES)
def test_converged_solve_against_the_dense_reference(qoc, monkeypatch, which):
    sc = gsc.solve_case(which)
    c, a, lam, Q = sc["c"], sc["args"], sc["lam"], sc["Q"]
    kw = {}
    if not isinstance(which, str):
        monkeypatch.setenv("GRAPE_SMALL_KERNEL", SHAPES[which][6])
        kw = dict(slices_per_lane=SHAPES[which][7], waves_per_member=SHAPES[which][8])
    rtol, iters = 1e-13, min(4 * Q, 400)
    with engine(qoc, c, **kw) as eng:
        s = step(eng, c, a, lam=lam, cg_iter=iters, cg_rtol=rtol)
        names = eng.kernel_names()
        Hp = eng.observe_gnvp(c["x"], s["p"], a["ops"], w=a["w"], wf=a["wf"], per_member=a["per_member"])
    g, p = s["g"], s["p"]
    print(f"{which}: Q={Q} lam={lam:.3e} cond={sc['cond']} iterations={s['iterations']} of {iters} residual={s['residual']:.3e} "
          f"|g|={s['g_norm']:.3e} |p|={s['p_norm']:.3e} predicted={s['predicted']:.6e}")
    assert s["status"] == 0 and 0 < s["iterations"] < iters
    assert s["residual"] <= rtol * s["g_norm"]
    assert "gn_residual_kernel" in names and "trajectory_gnvp_kernel" in names and "gn_cg_step_kernel" in names, names
    if sc["p_star"] is not None:
        assert sc["cond"] <= 26.0
        err, size = np.linalg.norm(p - sc["p_star"]), np.linalg.norm(sc["p_star"])
        print(f"{which}: |p - p*| = {err:.3e} of {size:.3e}")
        assert size > 0 and err <= 1e-10 * size
    else:
        res = np.linalg.norm(Hp + lam * p + g)
        print(f"{which}: true residual {res:.3e} of |g| = {np.linalg.norm(g):.3e}")
        assert res <= 1e-10 * np.linalg.norm(g)
    want = gsr.predicted_ref(g, p, Hp)
    assert want > 0 and abs(s["predicted"] - want) <= 1e-10 * want
    assert abs(s["p_norm"] - np.linalg.norm(p)) <= 1e-12 * s["p_norm"]


# ---- 5: reproducibility and independence -------------------------------------------------------------------------------------------
def gn_case(herm=False, E=10):
    c, O, _, _ = invariant_case(herm, E)
    rng = np.random.default_rng(8401)
    a = dict(ops=O, y_target=cplx(rng, E, O.shape[0], c["N"] + 1), w=gc.psd_blocks(rng, E, O.shape[0], c["N"] + 1),
             xf_target=cplx(rng, E, c["n"], c["m"]), wf=rng.uniform(0.2, 1.5, E), per_member=False)
    return c, a


def swept(names):
    return [k for k in names if k.startswith("sweep_")]


def test_bitwise_call_to_call_block_size_and_eval_gn_step_eval(qoc, torch, monkeypatch):
    c, a = gn_case()
    kw = dict(lam=5.0, cg_iter=300, cg_rtol=1e-9)
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        s1 = step(eng, c, a, **kw)
        names = eng.kernel_names()
        F1, G1 = eng.eval(c["x"])
        assert eng.kernel_names() == names0
        s2 = step(eng, c, a, **kw)
        other = step(eng, c, a, x=-c["x"], **kw)               # another call in between
        s3 = step(eng, c, a, **kw)
        monkeypatch.setenv("GRAPE_GN_CG_BLOCK", "1")
        b1 = step(eng, c, a, **kw)
        monkeypatch.setenv("GRAPE_GN_CG_BLOCK", "8")
        b8 = step(eng, c, a, **kw)
        monkeypatch.delenv("GRAPE_GN_CG_BLOCK")
        # the call leaves no trajectory for the reuse forms
        G = torch.zeros((eng._cols, eng.K), dtype=torch.float64, device="cuda")
        xb = dev(torch, np.zeros((c["E"], c["m"], c["n"]), complex))
        with pytest.raises(qoc.GrapeError) as ei:
            eng.observe_vjp_device(0, 0, False, 0, 0, ptr(xb), ptr(G))
        assert ei.value.status == -5 and "reuse" in str(ei.value), str(ei.value)
    assert F1 == F0 and np.array_equal(G1, G0)
    print(f"iterations: {s1['iterations']}")
    assert s1["status"] == 0 and 4 < s1["iterations"] < 300 and s1["p"].any()      # (an early exit: no-op launches behind it)
    assert same_bits(s1, s2) and same_bits(s1, s3) and not same_bits(s1, other)
    assert same_bits(s1, b1) and same_bits(s1, b8)
    assert len(swept(names)) == 1, names
    for k in ("gn_residual_kernel", "vjp_sum_kernel", "gn_cg_init_kernel", "trajectory_gnvp_kernel", "gn_cg_step_kernel"):
        assert k in names, names
    assert any(k.startswith("trajectory_vjp_") for k in names), names          # (the direct or the staged instance)
    assert names.count("gn_cg_step_kernel") == 1, names                           # (the names of ONE iteration)


@pytest.mark.parametrize("standing", ["running_cost", "penalties", "risk"])
def test_standing_costs_do_not_enter(qoc, standing):
    c, a = gn_case()
    kw = dict(lam=0.5, cg_iter=6, cg_rtol=0.0)
    with engine(qoc, c) as eng:
        s0 = step(eng, c, a, **kw)
        F0, _ = eng.eval(c["x"])
        if standing == "running_cost":
            eng.set_running_cost(c["R"], c["rho"])
        elif standing == "penalties":
            eng.set_penalties(np.array([0.3, 0.1]), np.array([0.05, 0.2]))
        else:
            eng.set_risk(2.0)
        F1, _ = eng.eval(c["x"])
        s1 = step(eng, c, a, **kw)
        F2, _ = eng.eval(c["x"])
    assert F1 != F0 and F2 == F1
    assert s0["iterations"] == 6 and same_bits(s0, s1)


def test_scratch_is_counted_in_workspace_bytes(qoc):
    c, a = gn_case()
    with engine(qoc, c) as eng:
        eng.observe_gnvp(c["x"], np.ones_like(c["x"]), a["ops"], w=a["w"], wf=a["wf"])
        eng.observe_vjp(c["x"], a["ops"], ybar=a["y_target"], xbar_final=a["xf_target"])
        before = eng.info["workspace_bytes"]
        step(eng, c, a, lam=0.5, cg_iter=3)
        grown = eng.info["workspace_bytes"] - before
        step(eng, c, a, lam=0.5, cg_iter=3)
        assert eng.info["workspace_bytes"] - before == grown
    # at least the targets and the seven vectors
    assert grown >= 16 * c["E"] * (a["ops"].shape[0] * (c["N"] + 1) + c["n"] * c["m"]) + 7 * 8 * c["K"] * c["N"], grown


# ---- 6: coordinates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["basis", "bounds", "both"])
def test_step_and_gradient_live_in_the_coordinates_of_x(qoc, mode):
    """under a pulse map g = Phi' s g_phys and the operator is Phi' s (J' W J) s Phi: the reference on the physical pulse through
    the slope and the projection, its dense matrix in the coordinates of theta, numpy.linalg.solve"""
    c = make_case(8501, 4, 2, 50, 3, hermitian=False)
    N, K, E = c["N"], c["K"], c["E"]
    rng = np.random.default_rng(8502)
    a = dict(ops=cplx(rng, 2, 4, 2), y_target=cplx(rng, E, 2, N + 1), w=gc.psd_blocks(rng, E, 2, N + 1),
             xf_target=cplx(rng, E, 4, 2), wf=rng.uniform(0.2, 1.5, E), per_member=False)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    x0 = 0.2 * rng.standard_normal((K, N))
    lo, hi = np.array([-0.8, -0.5]), np.array([0.9, 0.6])
    with engine(qoc, c) as eng:
        if mode != "bounds":
            eng.set_basis(phi, x0)
            theta = 0.4 * rng.standard_normal((K, 5))
            acc = x0 + theta @ phi.T
        else:
            theta = 0.7 * rng.standard_normal((K, N))
            acc = theta
        if mode != "basis":
            eng.set_bounds(lo, hi)
        x = eng.controls(theta)
        slope = np.ones_like(acc)
        if mode != "basis":
            mid, half = (0.5 * (lo + hi))[:, None], (0.5 * (hi - lo))[:, None]
            slope = 1.0 - np.tanh((acc - mid) / half) ** 2
        pr = gsc.problem_of(dict(c, x=x), a)
        down = (lambda v: v @ phi.T) if mode != "bounds" else (lambda v: v)        # theta -> the accumulated pulse
        up = (lambda G: G @ phi) if mode != "bounds" else (lambda G: G)
        g_ref = up(slope * pr.g)
        Q = theta.size
        H = np.empty((Q, Q))
        for q in range(Q):
            e = np.zeros(Q)
            e[q] = 1.0
            H[:, q] = up(slope * pr.apply(slope * down(e.reshape(theta.shape)))).reshape(-1)
        H = 0.5 * (H + H.T)
        ev = np.linalg.eigvalsh(H)
        lam = ev[-1] / 25.0
        p_star = -np.linalg.solve(H + lam * np.eye(Q), g_ref.reshape(-1)).reshape(theta.shape)
        s = step(eng, c, a, x=theta, lam=lam, cg_iter=min(4 * Q, 400), cg_rtol=1e-13)
        names = eng.kernel_names()
    assert s["p"].shape == theta.shape and s["g"].shape == theta.shape
    assert ("bounds_tangent_kernel" if mode == "bounds" else "basis_expand_kernel") in names, names
    eL, eg, gmax = abs(s["loss"] - pr.L), np.abs(s["g"] - g_ref).max(), np.abs(g_ref).max()
    err, size = np.linalg.norm(s["p"] - p_star), np.linalg.norm(p_star)
    print(f"{mode}: Q={Q} |dL|={eL:.3e} of {pr.L:.3e} |dg|_inf={eg:.3e} of {gmax:.3e} |p - p*|={err:.3e} of {size:.3e} "
          f"iterations={s['iterations']}")
    assert eL <= PARITY_RTOL * pr.L and eg <= PARITY_RTOL * gmax
    assert s["status"] == 0 and (ev[-1] + lam) / (max(ev[0], 0.0) + lam) <= 26.0
    assert size > 0 and err <= 1e-10 * size


# ---- 7: refusals and arguments --------------------------------------------------------------------------------------------------
def raw_call(qoc, eng_h, x, n_obs, pm, O, yt, wpm, wy, xt, wf, opts, p, g, res):
    lib = qoc.load_library()
    q = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    rc = lib.grape_gn_step(eng_h, q(x), n_obs, pm, q(O), q(yt), wpm, q(wy), q(xt), q(wf),
                           None if opts is None else C.byref(opts), q(p), q(g), None if res is None else C.byref(res))
    return rc, lib.grape_last_error(eng_h).decode()


def test_refusals(qoc, monkeypatch):
    c = make_case(8701, 4, 4, 20, 2)
    GE = qoc.GrapeError

    def refused(eng, case, word, x=None):
        x = case["x"] if x is None else x
        F0, G0 = eng.eval(x)
        with pytest.raises(GE) as ei:
            eng.gn_step(x, None, xf_target=np.zeros((case["E"], case["n"], case["m"]), complex), wf=np.ones(case["E"]))
        assert ei.value.status == -2 and word in str(ei.value) and "grape_gn_step" in str(ei.value), str(ei.value)
        F, G = eng.eval(x)
        assert F == F0 and np.array_equal(G, G0)

    big = make_case(8707, 5, 5, 8, 1)
    with engine(qoc, big) as eng:
        refused(eng, big, "dimension")
    for sys_type in ("StateTransfer", "CoherenceTransfer"):
        with qoc.GrapeEngine(sys_type, c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], T, 20) as eng:
            refused(eng, c, "StateTransfer")
    with engine(qoc, c, gradient="exact") as eng:
        refused(eng, c, "exact")
    with engine(qoc, c, force_collective=True) as eng:
        refused(eng, c, "communicator")
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative("exact")
        refused(eng, c, "trajectory_derivative")
        eng.set_trajectory_derivative("first_order")
        eng.set_bounds(np.array([-0.8, -0.5]), np.array([0.9, 0.6]))              # bounds are served
        s = eng.gn_step(0.3 * c["x"], None, xf_target=np.zeros((2, 4, 4), complex), wf=np.ones(2), lam=0.1, cg_iter=2)
        assert s["p"].any() and s["iterations"] == 2
    # a member-chunked context: this call's own refusal, behind grape_eval_gnvp's
    cc, a = gn_case()
    with engine(qoc, cc) as eng:
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(cc, info, False, 4)))
    with engine(qoc, cc) as eng:
        assert 0 < eng.info["member_chunk"] < cc["E"]
        refused(eng, cc, "member_chunk")


def test_invalid_arguments_and_nan(qoc):
    c = make_case(8801, 4, 4, 20, 2)
    E, N, K = c["E"], c["N"], c["K"]
    rng = np.random.default_rng(8802)
    O = cplx(rng, 2, 4, 4)
    Opt, Res = qoc.engine.GrapeGnOptions, qoc.engine.GrapeGnResult
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])

        def unchanged():
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)

        xf = np.ascontiguousarray(c["x"].T)
        Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
        wy, wym, wf = gc.psd_blocks(rng, 2, N + 1), gc.psd_blocks(rng, E, 2, N + 1), rng.uniform(0.2, 1.5, E)
        yt, xt = cplx(rng, E, 2, N + 1), cplx(rng, E, 4, 4)
        p, g, res, ok = np.empty((N, K)), np.empty((N, K)), Res(), Opt(0.1, 1e-10, 3, 0)
        bad_args = [
            (None, 2, 0, Of, yt, 0, wy, xt, wf, ok, p, g, res),                   # null x
            (xf, 2, 0, Of, yt, 0, wy, xt, wf, ok, None, g, res),                  # null p
            (xf, 2, 0, Of, yt, 0, wy, xt, wf, ok, p, g, None),                    # null result
            (xf, 2, 0, Of, yt, 0, wy, xt, wf, None, p, g, res),                   # null opts
            (xf, 2, 0, Of, None, 0, None, None, None, ok, p, g, res),             # no pair at all
            (xf, 2, 0, Of, None, 0, wy, xt, wf, ok, p, g, res), (xf, 2, 0, Of, yt, 0, None, xt, wf, ok, p, g, res),   # wy / y_target apart
            (xf, 2, 0, Of, yt, 0, wy, None, wf, ok, p, g, res), (xf, 2, 0, Of, yt, 0, wy, xt, None, ok, p, g, res),   # wf / Xf_target apart
            (xf, 2, 0, Of, yt, 0, wy, xt, wf, Opt(-0.1, 1e-10, 3, 0), p, g, res), (xf, 2, 0, Of, yt, 0, wy, xt, wf, Opt(np.nan, 1e-10, 3, 0), p, g, res),
            (xf, 2, 0, Of, yt, 0, wy, xt, wf, Opt(np.inf, 1e-10, 3, 0), p, g, res),                                   # lambda
            (xf, 2, 0, Of, yt, 0, wy, xt, wf, Opt(0.1, np.nan, 3, 0), p, g, res), (xf, 2, 0, Of, yt, 0, wy, xt, wf, Opt(0.1, np.inf, 3, 0), p, g, res),
            (xf, 2, 0, Of, yt, 0, wy, xt, wf, Opt(0.1, 1e-10, -1, 0), p, g, res),                                     # cg_max_iter < 0
            (xf, 2, 0, Of, yt, 0, wy, xt, wf, Opt(0.1, 1e-10, 3, 1), p, g, res),                                      # reserved
            (xf, 2, 0, Of, yt, 2, wy, xt, wf, ok, p, g, res), (xf, 2, 0, Of, yt, -1, wy, xt, wf, ok, p, g, res),      # w_per_member
            (xf, 0, 0, Of, yt, 0, wy, xt, wf, ok, p, g, res),                     # n_obs = 0 with a non-NULL wy
            (xf, -1, 0, Of, yt, 0, wy, xt, wf, ok, p, g, res), (xf, 17, 0, Of, yt, 0, wy, xt, wf, ok, p, g, res),     # n_obs outside 0..16
            (xf, 2, 0, None, yt, 0, wy, xt, wf, ok, p, g, res),                   # n_obs > 0 with a NULL O
            (xf, 2, 2, Of, yt, 0, wy, xt, wf, ok, p, g, res),                     # per_member other than 0 or 1
        ]
        for args in bad_args:
            rc, msg = raw_call(qoc, eng._h, *args)
            assert rc == -1 and "grape_gn_step" in msg, (rc, msg)
            unchanged()
        names = ["O[", "y_target[", "wy[", "Xf_target[", "wf["]
        for which in range(5):                                # NaN, then inf, in every host array but x
            for bad in (np.nan, np.inf):
                arrs = [Of.copy(), yt.copy(), wy.copy(), xt.copy(), wf.copy()]
                arrs[which].reshape(-1)[1] = bad
                rc, msg = raw_call(qoc, eng._h, xf, 2, 0, arrs[0], arrs[1], 0, arrs[2], arrs[3], arrs[4], ok, p, g, res)
                assert rc == -1 and "not finite" in msg and names[which] in msg, (rc, msg)
            unchanged()
        for args in ((2, 0, Of, yt, 0, wy, xt, wf, ok, p, g), (2, 0, Of, yt, 0, wy, None, None, ok, p, None),
                     (2, 0, Of, yt, 1, wym, xt, wf, ok, p, g), (2, 0, Of, None, 0, None, xt, wf, ok, p, g),
                     (0, 0, None, None, 0, None, xt, wf, Opt(0.1, -1.0, 3, 0), p, g)):       # every valid NULL combination
            rc, msg = raw_call(qoc, eng._h, xf, *args, res)
            assert rc == 0 and res.cg_iterations == 3, msg
        unchanged()
        # a non-finite x is not refused: the call comes back with NaN in the loss and no step
        xb = c["x"].copy()
        xb[1, 3] = np.nan
        s = eng.gn_step(xb, O, y_target=yt, w=wy, xf_target=xt, wf=wf, lam=0.1, cg_iter=5)
        assert s["status"] == 2 and s["loss"] != s["loss"] and not s["p"].any() and s["iterations"] == 0
        unchanged()
    # before grape_set_operators
    lib = qoc.load_library()
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        rc, msg = raw_call(qoc, h, xf, 2, 0, Of, yt, 0, wy, xt, wf, ok, p, g, res)
        assert rc == -5 and "operators not set" in msg
    finally:
        lib.grape_destroy(h)


# ---- 8: the Levenberg-Marquardt loop with the step solved on the device ---------------------------------------------------------------
def test_fit_trajectory_on_the_device_tracks_the_curve_of_a_known_pulse(qoc):
    """the case of test_gpu_gnvp.py's loop test (seed 7901, 24 unknowns, lam0 = 0.1, cg_rtol = 1e-12, cg_iter = 60): the first
    step is a CONVERGED solve of a system of condition <= 1e3, so the two loops' first steps agree to cond * cg_rtol, inside
    1e-8 of the step; the final loss is held to the factor that test measures against the reference-driven loop"""
    from quoptimalcontrol_jl_amd import gauss_newton as gn
    c = make_case(7901, 2, 1, 12, 2, K=2, hermitian=True)
    rng = np.random.default_rng(7902)
    O = cplx(rng, 3, 2, 1)
    w = rng.uniform(0.5, 1.5, (3, 13))
    x_star = c["x"]
    x0 = x_star + 0.1 * rng.standard_normal(x_star.shape)
    kw = dict(max_iter=10, cg_iter=60, lam0=0.1, cg_rtol=1e-12)
    with engine(qoc, c) as eng:
        y_target = eng.observe(x_star, O)
        on_device = gn.fit_trajectory(eng, x0, O, y_target, w=w, solver="device", **kw)
        fused = gn.fit_trajectory(eng, x0, O, y_target, w=w, operator="fused", **kw)
        by_ref = gn.fit_trajectory(eng, x0, O, y_target, w=w, **kw, operator=lambda x: (
            lambda v: gr.gnvp_ref(c["A"], c["B"], c["Xi"], x, v, c["T"], O, w, None, False, c["variant"])))
        with pytest.raises(ValueError):
            gn.fit_trajectory(eng, x0, O, y_target, w=w, solver="device", operator=lambda x: (lambda v: v))
    res = on_device
    assert res["accepted"] >= 1 and all(b < a for a, b in zip(res["losses"], res["losses"][1:])), res["losses"]
    step0 = fused["steps"][0]
    dstep = np.linalg.norm(res["steps"][0] - step0)
    print(f"losses: start {res['losses'][0]:.3e}; device {res['loss']:.3e} fused {fused['loss']:.3e} reference-driven "
          f"{by_ref['loss']:.3e}; first steps differ by {dstep:.3e} of {np.linalg.norm(step0):.3e}")
    assert res["losses"][0] == fused["losses"][0] or abs(res["losses"][0] - fused["losses"][0]) <= 1e-10 * fused["losses"][0]
    assert dstep <= 1e-8 * np.linalg.norm(step0)
    assert res["loss"] < res["losses"][0] and res["loss"] <= 10.0 * by_ref["loss"]
