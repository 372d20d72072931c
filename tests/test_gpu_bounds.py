"""GPU: smooth amplitude bounds on the device (grape_set_bounds).

The entry points take a raw pulse u (theta with a basis); the device saturates it, x = mid + half tanh((u - mid) / half),
evaluates the physical pulse and returns G_u = G_tot s with s = 1 - tanh^2.  Every device result is held to a reference no
device result enters -- the oracle on the NumPy-saturated pulse, plus penalty_ref and running_cost_ref, times the NumPy
slope, projected in NumPy (bounds_sequences.bounded_reference) -- through conftest.assert_parity at the project's 1e-10 bar.
The bitwise checks compare device results with each other."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_parity
import bounds_sequences as bs
import settings_sequences as ss
from test_gpu_basis import draw, engine, sized

pytestmark = pytest.mark.gpu
INF = np.inf


def small_ctx(n, K, N, E=3, variant=0, kernel="lane", m=None, T=0.9):
    return dict(full=True, sys_type="UnitaryGate", n=n, m=m or n, K=K, E=E, N=N, T=T, scale=0.8, variant=variant,
                max_batch=1, kernel=kernel)


def small_engine(qoc, ctx, ops, **kw):
    return qoc.GrapeEngine("UnitaryGate", ops["A"], ops["B"], ops["Xi"], ops["Xt"], ops["wts"], ctx["T"], ctx["N"],
                           variant=ctx["variant"], **kw)


def mixed_bounds(K):
    """K = 1: one bounded control; K = 3: bounded, free, bounded and not symmetric about 0"""
    return (np.array([-0.6]), np.array([0.8])) if K == 1 else (np.array([-0.6, -INF, -0.2]), np.array([0.8, INF, 1.1]))


def reference(oracle, ctx, ops, u, lo, hi, penalties=None, rc=None):
    x, s = bs.sat(u, lo, hi)
    F, G, _ = ss.composed_reference(oracle, ops, x, ctx["T"], ctx["variant"], penalties, rc, ctx["sys_type"])
    return F, G * s, x, s


# ---- 1. parity of F and G_u -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 83, 130])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("herm", [True, False])
@pytest.mark.parametrize("n,kernel", [(2, "lane"), (2, "pair"), (3, "lane"), (4, "lane"), (4, "pair")])
def test_parity_on_the_small_kernels(qoc, oracle, monkeypatch, n, kernel, herm, variant, N):
    K = 1 if (variant + herm) % 2 == 0 else 3             # (every (n, kernel, N) sees both, with either variant)
    E = 7 if N <= 5 else 3
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    ctx = small_ctx(n, K, N, E, variant, kernel)
    rng = np.random.default_rng(1000 * n + 10 * N + 2 * variant + herm)
    ops = ss._full_operators(rng, ctx, herm, False)
    lo, hi = mixed_bounds(K)
    u = rng.uniform(-1.5, 1.5, (K, N))
    F_ref, G_ref, x_ref, s = reference(oracle, ctx, ops, u, lo, hi)
    with small_engine(qoc, ctx, ops) as eng:
        eng.set_bounds(lo, hi)
        F, G = eng.eval(u)
        names, info = eng.kernel_names(), eng.info
        x = eng.controls(u)
    print(f"n={n} {kernel} herm={herm} v{variant} N={N} K={K}: |dF| = {abs(F - F_ref):.2e}, max |dG| / max |G_ref| = "
          f"{np.abs(G - G_ref).max() / np.abs(G_ref).max():.2e}, min slope {s.min():.2e}")
    assert info["lane_pair"] == (1 if kernel == "pair" else 0) and info["unitary_flow"] == (1 if herm else 0)
    assert names[0] == "bounds_saturate_kernel" and names[-1] == "bounds_slope_kernel", names
    assert np.abs(x - x_ref).max() <= 1e-10
    assert_parity(F, G, F_ref, G_ref, n, what="bounds only")


@pytest.mark.parametrize("n,sys_type", [(8, "StateTransfer"), (40, "UnitaryGate")])
def test_parity_in_the_tile_and_grid_families(qoc, oracle, n, sys_type):
    w = sized(qoc, n, sys_type, 700 + n)
    lo, hi = mixed_bounds(w.K)
    u = np.random.default_rng(n).uniform(-1.5, 1.5, (w.K, w.N))
    x, s = bs.sat(u, lo, hi)
    F_ref, G_x = oracle.ensemble_eval(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, x, w.T, 0)
    with engine(qoc, w) as eng:
        eng.set_bounds(lo, hi)
        F, G = eng.eval(u)
        names = eng.kernel_names()
    print(f"n={n}: {names}")
    assert names[0] == "bounds_saturate_kernel" and names[-1] == "bounds_slope_kernel", names
    assert_parity(F, G, F_ref, G_x * s, n, what=f"n={n}")


# ---- 2. saturation in both directions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_basis", [False, True])
def test_deep_saturation_in_both_directions(qoc, oracle, with_basis):
    """u 60 half-widths outside either bound: tanh has rounded to +-1, the slope is 0 -- x stays strictly inside, G is finite
    (exactly 0 there), F and the rest of G at parity"""
    ctx = small_ctx(4, 3, 20)
    rng = np.random.default_rng(77)
    ops = ss._full_operators(rng, ctx, True, False)
    lo, hi = mixed_bounds(3)
    half = (hi - lo) / 2
    u = rng.uniform(-0.5, 0.5, (3, 20))
    u[0, 3], u[0, 4], u[2, 0], u[2, 19] = hi[0] + 60 * half[0], lo[0] - 60 * half[0], lo[2] - 1e6, hi[2] + 1e300
    u[1, 5] = 40.0                                           # the free control takes anything
    with small_engine(qoc, ctx, ops) as eng:
        eng.set_bounds(lo, hi)
        if with_basis:                                       # the identity basis: theta IS the raw pulse, the fused kernels run
            eng.set_basis(np.eye(20))
        F, G = eng.eval(u)
        x = eng.controls(u)
        names = eng.kernel_names()
    assert names[0] == ("basis_expand_kernel" if with_basis else "bounds_saturate_kernel"), names
    F_ref, G_ref, x_ref, s = reference(oracle, ctx, ops, u, lo, hi)
    assert s[0, 3] == 0 and s[0, 4] == 0 and s[2, 0] == 0 and s[2, 19] == 0
    for c in (0, 2):
        assert np.all(x[c] > lo[c]) and np.all(x[c] < hi[c]), (c, x[c])
    assert x[0, 3] == np.nextafter(hi[0], lo[0]) and x[0, 4] == np.nextafter(lo[0], hi[0])
    assert x[1, 5] == 40.0
    assert np.all(np.isfinite(G)) and np.isfinite(F)
    assert G[0, 3] == 0 and G[0, 4] == 0 and G[2, 0] == 0 and G[2, 19] == 0
    assert np.abs(x - x_ref).max() <= 1e-10
    assert_parity(F, G, F_ref, G_ref, 4, what="deep saturation")


# ---- 3. penalties and a running cost act on the physical pulse ------------------------------------------------------------
@pytest.mark.parametrize("n,kernel,herm", [(2, "pair", True), (3, "lane", False), (4, "pair", False)])
def test_penalties_and_running_cost_on_the_physical_pulse(qoc, oracle, monkeypatch, n, kernel, herm):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    ctx = small_ctx(n, 3, 20)
    rng = np.random.default_rng(90 + n)
    ops = ss._full_operators(rng, ctx, herm, False)
    lo, hi = mixed_bounds(3)
    u = rng.uniform(-1.5, 1.5, (3, 20))
    pen = dict(amp=np.array([0.3, 0.5, 0.2]), var=np.array([0.1, 0.05, 0.25]))
    rc = ss._draw_rc(rng, ctx, ops["Xt"], 2)
    F_ref, G_ref, x, s = reference(oracle, ctx, ops, u, lo, hi, pen, rc)
    F_raw = ss.composed_reference(oracle, ops, u, ctx["T"], ctx["variant"], pen, rc)[0]      # the terms on u instead
    with small_engine(qoc, ctx, ops) as eng:
        eng.set_penalties(pen["amp"], pen["var"])
        eng.set_running_cost(rc["R"], rc["rho"])
        eng.set_bounds(lo, hi)
        F, G = eng.eval(u)
        f = eng.fom(u)
    assert abs(F_raw - F_ref) > 1e-3                         # (evaluating a term on the raw pulse would show)
    assert_parity(F, G, F_ref, G_ref, n, what="penalties + running cost + bounds")
    assert f == F                                            # a running cost sends fom through the full evaluation


# ---- 4. with a basis ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("per_control", [False, True])
@pytest.mark.parametrize("n,kernel", [(2, "lane"), (4, "pair")])
def test_bounded_pulse_in_a_basis(qoc, oracle, monkeypatch, n, kernel, per_control, M):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    ctx = small_ctx(n, 3, 83, variant=1)
    rng = np.random.default_rng(200 + n + M)
    ops = ss._full_operators(rng, ctx, True, False)
    st = bs.BState(dict(ctx, ops=ops, pool=None))
    st.apply(dict(op="basis_per_control" if per_control else "basis_on", phi=rng.standard_normal((3, 83, M) if per_control
                  else (83, M)), x0=0.3 * rng.standard_normal((3, 83)), thetas=None))
    st.apply(dict(op="bounds_on", lo=mixed_bounds(3)[0], hi=mixed_bounds(3)[1]))
    st.apply(dict(op="pen_on", amp=np.array([0.3, 0.5, 0.2]), var=None))
    theta = rng.uniform(-1, 1, (3, M)) / np.sqrt(M)
    F_ref, G_ref, x_ref = bs.bounded_reference(oracle, st, theta)
    with small_engine(qoc, ctx, ops) as eng:
        eng.set_penalties(st.pen["amp"], None)
        eng.set_basis(st.basis["phi"], st.basis["x0"])
        eng.set_bounds(*st.bounds)
        F, G = eng.eval(theta)
        names = eng.kernel_names()
        x = eng.controls(theta)
    assert names[0] == "basis_expand_kernel" and names[-1] == "basis_project_kernel", names
    assert not any(k.startswith("bounds_") for k in names), names      # fused: no second pass
    assert G.shape == (3, M) and np.abs(x - x_ref).max() <= 1e-10
    _, s = st.physical(theta)
    assert np.abs(s - 1).max() > 1e-2                        # the saturation bites at this pulse
    assert_parity(F, G, F_ref, G_ref, n, what="basis + bounds")


# ---- 5. bitwise -----------------------------------------------------------------------------------------------------------
def _device_eval(eng, arr, K, cols):
    import torch
    xd = torch.as_tensor(np.ascontiguousarray(arr.T), device="cuda:0")
    fg = torch.zeros(K * cols + 1, dtype=torch.float64, device="cuda:0")
    eng.eval_device(xd.data_ptr(), fg.data_ptr(), torch.cuda.current_stream(0).cuda_stream)
    torch.cuda.synchronize(0)
    h = fg.cpu().numpy()
    return h[-1], h[:-1].reshape(cols, K).T


@pytest.mark.parametrize("case", ["n4", "n8", "n4_basis"])
def test_entry_points_agree_bit_for_bit(qoc, case):
    """F is the F a context without bounds returns from eval_device for the pulse controls(u) returned; eval, F-only,
    eval_batch, the device-pointer form and (on a context whose fom is the full evaluation: n = 8) fom return the same bits;
    two identical calls agree."""
    if case == "n8":
        w = sized(qoc, 8, "StateTransfer", 31)
    else:
        w = qoc.workloads.config("C3", E=6, N=50)
    lo, hi = (np.full(w.K, -0.7), np.full(w.K, 0.5))
    lo[1], hi[1] = -INF, INF
    rng = np.random.default_rng(32)
    phi = rng.standard_normal((w.N, 6)) if case == "n4_basis" else None
    cols = 6 if phi is not None else w.N
    us = rng.uniform(-1.2, 1.2, (3, w.K, cols))
    with engine(qoc, w, max_batch=3) as eng:
        eng.set_bounds(lo, hi)
        if phi is not None:
            eng.set_basis(phi, 0.2 * w.x)
        single = [eng.eval(u) for u in us]
        again = eng.eval(us[0])
        F_only = eng.eval(us[1], want_G=False)[0]
        Fb, Gb = eng.eval_batch(us)
        Fd, Gd = _device_eval(eng, us[2], w.K, cols)
        foms = [eng.fom(u) for u in us]
        xs = [eng.controls(u) for u in us]
    assert again[0] == single[0][0] and np.array_equal(again[1], single[0][1])
    assert F_only == single[1][0]
    for b in range(3):
        assert Fb[b] == single[b][0] and np.array_equal(Gb[b], single[b][1]), b
    assert Fd == single[2][0] and np.array_equal(Gd, single[2][1])
    if case == "n8":
        assert foms == [s[0] for s in single]
    else:                                                    # the forward-only kernel: its own arithmetic, close
        for b in range(3):
            assert abs(foms[b] - single[b][0]) <= 1e-10 * max(1.0, abs(single[b][0]))
    with engine(qoc, w) as plain:
        for b in range(3):
            assert np.all(xs[b][0] > lo[0]) and np.all(xs[b][0] < hi[0])
            Fx, _ = _device_eval(plain, xs[b], w.K, w.N)
            assert Fx == single[b][0], (b, Fx, single[b][0])


def test_member_chunked_context_is_the_unchunked_one(qoc, monkeypatch):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", "lane")
    ctx = small_ctx(4, 2, 65, E=7)
    rng = np.random.default_rng(5)
    ops = ss._full_operators(rng, ctx, False, False)
    lo, hi = np.array([-0.6, -0.3]), np.array([0.8, 0.9])
    u = rng.uniform(-1.5, 1.5, (2, 65))
    res = []
    for budget in (None, int(2.5 * 2 * 16 * 1 * 16 * 64 * 2)):     # two and a half members' propagators and states
        if budget:
            monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(budget))
        with small_engine(qoc, ctx, ops, waves_per_member=2) as eng:
            eng.set_bounds(lo, hi)
            res.append((eng.eval(u), eng.info["member_chunk"]))
    (r0, c0), (r1, c1) = res
    assert 0 < c1 < 7 and not 0 < c0 < 7, (c0, c1)
    assert r1[0] == r0[0] and np.array_equal(r1[1], r0[1])


# ---- 6. off means off -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C3", "C4"])
def test_off_means_off(qoc, cfg):
    """After set -> off, on a context that never called grape_set_bounds, and with bounds that leave every control free (the
    header: the same as switching them off, i.e. as a context that never called it): the same kernels, the same bits."""
    w = qoc.workloads.config("C3", E=8, N=100) if cfg == "C3" else qoc.workloads.config("C4", E=3, N=12)
    X = np.array([w.x, 0.5 * w.x])

    def observe(eng):
        F, G = eng.eval(w.x)
        names = eng.kernel_names()
        f = eng.fom(w.x)
        fnames = eng.kernel_names()
        Fb, Gb = eng.eval_batch(X)
        return F, G, names, f, fnames, Fb, Gb, eng.controls(w.x)

    def same(a, b):
        return all(np.array_equal(p, q) if isinstance(p, np.ndarray) else p == q for p, q in zip(a, b))

    with engine(qoc, w, max_batch=2) as never:
        base = observe(never)
    assert not any(k.startswith("bounds_") or k.startswith("basis_") for k in base[2] + base[4]), base[2]
    with engine(qoc, w, max_batch=2) as eng:
        eng.set_bounds(-0.4, 0.6)
        on = observe(eng)
        assert on[2][0] == "bounds_saturate_kernel" and on[0] != base[0] and eng.bounds is not None
        eng.set_bounds(None)
        assert eng.bounds is None
        assert same(observe(eng), base), "set -> off"
        eng.set_bounds(-0.4, 0.6)
        eng.set_bounds(-INF, INF)                            # every control free: off
        assert eng.bounds is None
        assert same(observe(eng), base), "all-infinite bounds"
        eng.set_bounds(np.full(w.K, -INF), np.full(w.K, INF))
        assert same(observe(eng), base), "all-infinite bounds, vectors"
        assert np.array_equal(base[7], w.x)


def test_bounds_persist_across_set_operators(qoc):
    w = qoc.workloads.config("C3", E=8, N=60)
    u = 1.5 * w.x
    with engine(qoc, w) as eng:
        eng.set_bounds(-0.4, 0.6)
        F0, G0 = eng.eval(u)
        eng.set_operators(w.A, w.B, w.Xi, w.Xt, w.wts)
        F1, G1 = eng.eval(u)
    assert F1 == F0 and np.array_equal(G1, G0)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_keep_the_previous_setting(qoc):
    w = qoc.workloads.config("C3", E=8, N=60)
    K = w.K
    u = 1.5 * w.x
    with engine(qoc, w) as eng:
        eng.set_bounds(-0.4, 0.6)
        F0, G0 = eng.eval(u)
        lib, h, p = eng._lib, eng._h, lambda a: a.ctypes.data
        good_lo, good_hi = np.full(K, -1.0), np.full(K, 1.0)

        def with_one(lo_v, hi_v):
            lo, hi = good_lo.copy(), good_hi.copy()
            lo[2], hi[2] = lo_v, hi_v
            return lo, hi
        for lo_v, hi_v in ((-1.0, INF), (-INF, 1.0), (1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (-1.0, np.nan), (INF, INF),
                           (INF, -INF)):
            lo, hi = with_one(lo_v, hi_v)
            assert lib.grape_set_bounds(h, p(lo), p(hi)) == -1, (lo_v, hi_v)
            assert "control 2" in lib.grape_last_error(h).decode()
            F1, G1 = eng.eval(u)
            assert F1 == F0 and np.array_equal(G1, G0), (lo_v, hi_v)
        assert lib.grape_set_bounds(h, p(good_lo), None) == -1 and lib.grape_set_bounds(h, None, p(good_hi)) == -1
        for bad in ((np.full(K + 1, -1.0), np.full(K + 1, 1.0)), (np.full(K - 1, -1.0), 1.0), (-1.0, INF), (0.5, 0.5)):
            with pytest.raises(ValueError):
                eng.set_bounds(*bad)
        with pytest.raises(ValueError):
            eng.set_bounds(-1.0)                             # hi missing
        F1, G1 = eng.eval(u)
        assert F1 == F0 and np.array_equal(G1, G0) and np.array_equal(eng.bounds[0], np.full(K, -0.4))


# ---- 8. grape_lbfgs -------------------------------------------------------------------------------------------------------
def _lbfgs_case(qoc, n):
    if n == 4:
        w = qoc.workloads.config("C3", E=8, N=20)
        rho0 = np.zeros((4, 4), complex)
        rho0[0, 0] = 1
        psi = np.array([1, 1j, -1, 0.5]) / np.linalg.norm([1, 1j, -1, 0.5])
        Xi = np.broadcast_to(rho0, (w.E, 4, 4)).copy()
        Xt = np.broadcast_to(np.outer(psi, psi.conj()), (w.E, 4, 4)).copy()
        return ("StateTransfer", w.A, w.B, Xi, Xt, w.wts, w.T, w.N), w
    w = qoc.workloads.reference_ensemble("StateTransfer", 5, 20, 5.0)
    return (w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N), w


@pytest.mark.parametrize("n", [2, 4])
def test_lbfgs_iterates_match_the_host_restatement_with_bounds(qoc, n):
    """grape_lbfgs(line_search = 1) over the raw pulse against oracle/optim_lbfgs.py driven with the NumPy-wrapped objective
    -- a context without bounds, saturation and slope in NumPy -- with the comparison and the bars of
    tests/test_gpu_lbfgs.py::test_iterates_match_the_host_restatement (settings_sequences.compare_lbfgs_iterates): accepted
    step length to 1e-6, iterate to 1e-9, evaluations per iteration equal.  The returned physical pulse lies strictly inside.
    The bounds: n = 4 (-1.1, 1.3) around a guess in (0, 1); n = 2 (-3, 3.5) around an unbounded optimum that peaks at 3.5 --
    the slope at the ninth iterate is below 0.6 on the CPU oracle, yet the reference's own line search stays regular for the
    nine iterations (with (-1.1, 1.3) the optimum sits in saturation, where the first-order StateTransfer gradient is no longer
    the derivative of F to the digits the approximate Wolfe test needs, and from its fourth iteration on the reference
    bisects ~55 times per iteration: the helper ends its comparison at such an iteration)."""
    from oracle import optim_lbfgs
    args, w = _lbfgs_case(qoc, n)
    lo, hi = (np.full(w.K, -1.1), np.full(w.K, 1.3)) if n == 4 else (np.full(w.K, -3.0), np.full(w.K, 3.5))
    u0 = qoc.bounds.bounds_start(w.x, lo, hi)
    n_it = 9

    def wrapped(u):
        x, s = bs.sat(u, lo, hi)
        F, Gx = ref_eng.eval(x)
        return F, Gx * s

    with qoc.GrapeEngine(*args) as ref_eng:
        ref = optim_lbfgs.lbfgs(wrapped, u0, iterations=n_it)
    with qoc.GrapeEngine(*args) as eng:
        eng.set_bounds(lo, hi)
        ss.compare_lbfgs_iterates(eng, ref, u0, n_it, f"n={n} with bounds", min_compared=8)
        u_min, info = eng.lbfgs(u0, iterations=30)
        x_min = eng.controls(u_min)
        F0 = eng.eval(u0)[0]
    assert info["minimum"] < F0
    assert np.all(x_min > lo[:, None]) and np.all(x_min < hi[:, None])
    assert bs.sat(ref["trace"][-1]["x"].reshape(u0.shape), lo, hi)[1].min() < 0.9      # the bounds shaped the iterates compared


# ---- 9. solve(prob, GRAPE(bounds=...)) ------------------------------------------------------------------------------------
def test_solve_keeps_the_pulse_inside_where_the_unbounded_solve_leaves(qoc, oracle):
    """The reference's n_ens = 5 StateTransfer ensemble (N = 25, T = 5).  The bound is 0.6 x the peak amplitude of the
    UNBOUNDED optimum, found here with the host optimiser on the CPU oracle: the unbounded solve exceeds it by construction,
    and on the device too; the bounded solves -- host and device optimiser -- must stay strictly below it."""
    wl = qoc.workloads
    N, T = 25, 5.0
    w = wl.reference_ensemble("StateTransfer", 5, N, T)
    free = qoc.api._lbfgs(lambda x: oracle.ensemble_eval(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, x, w.T, 0), w.x, {})
    peak = np.abs(free.minimizer).max()
    bound = 0.6 * peak
    assert peak > bound > np.abs(w.x).max() * 1.001          # the guess starts inside: no clipping in this test
    prob = qoc.Problem(B=[wl.Sx, wl.Sy], A=wl.Sz, Xi=wl.rho_init, Xt=wl.rho_fin, T=T, n_controls=2, guess=wl.controls(2, N),
                       sys_type=qoc.StateTransfer())
    ens = qoc.EnsembleProblem(prob=prob, n_ens=5, A_g=lambda k: (k - 2.5) / 2.5 * wl.Sz * 5, B_g=lambda k: [wl.Sx, wl.Sy],
                              XiG=lambda k: wl.rho_init, XtG=lambda k: wl.rho_fin if k % 2 else wl.rho_init,
                              wts=np.ones(5) / 5)
    guess = np.array(prob.guess, dtype=np.float64)
    unb = qoc.solve(ens, qoc.GRAPE(n_slices=N))
    print(f"unbounded: CPU oracle peak {peak!r}, device peak {np.abs(unb.opti_pulses).max()!r}; bound {bound!r}")
    assert np.abs(unb.opti_pulses).max() > bound
    with qoc.api.make_engine(ens, qoc.GRAPE(n_slices=N)) as eng:
        F_guess = eng.eval(guess)[0]
        for optimizer in ("host", "device"):
            sol = qoc.solve(ens, qoc.GRAPE(n_slices=N, bounds=(-bound, bound), optimizer=optimizer))
            top = np.abs(sol.opti_pulses).max()
            print(f"{optimizer}: minimum {sol.result.minimum!r}, max |opti_pulses| {top!r}")
            assert isinstance(sol, qoc.EnsembleSolutionResult) and sol.opti_pulses.shape == (2, N)
            assert top < bound
            assert sol.parameters.shape == (2, N)            # the raw variables; opti_pulses is their physical pulse
            assert np.abs(bs.sat(sol.parameters, [-bound] * 2, [bound] * 2)[0] - sol.opti_pulses).max() <= 1e-10
            assert eng.eval(sol.opti_pulses)[0] == pytest.approx(sol.result.minimum, abs=1e-10)
            assert sol.result.minimum < F_guess
    assert np.array_equal(np.asarray(prob.guess, dtype=np.float64), guess)


# ---- 10. groups and mailbox ranks -----------------------------------------------------------------------------------------
def test_two_shard_group_is_the_single_device_result_bit_for_bit(qoc):
    """A device_ids = [0, 0] peer-sum group against one device.  Two members with the weight 1/2 each: every product w_k g_k
    is exact, so one device's multiply-add chain over the members and the group's sum of its two shards' rows round the same
    exact sum once -- the same bits in, the same bits out, and the slope multiplies the same row.  (Larger ensembles are summed
    in another order by a group; they are held to parity below.)"""
    ctx = small_ctx(4, 3, 60, E=2)
    rng = np.random.default_rng(8)
    ops = ss._full_operators(rng, ctx, True, False)
    ops["wts"] = np.array([0.5, 0.5])
    lo, hi = mixed_bounds(3)
    phi = rng.standard_normal((60, 5))
    us, thetas = rng.uniform(-1.5, 1.5, (2, 3, 60)), rng.uniform(-0.5, 0.5, (2, 3, 5))
    out = []
    for kw in (dict(), dict(devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM)):
        with small_engine(qoc, ctx, ops, slices_per_lane=1, waves_per_member=1, **kw) as eng:
            eng.set_bounds(lo, hi)
            r = [eng.eval(u) for u in us]
            names = eng.kernel_names()
            eng.set_basis(phi)
            r += [eng.eval(th) for th in thetas]
            r.append((eng.eval(thetas[1], want_G=False)[0], eng.controls(thetas[0])))
        out.append(r)
        assert names[0] == "bounds_saturate_kernel" and names[-1] == "bounds_slope_kernel", names
    for i, ((F1, G1), (Fg, Gg)) in enumerate(zip(*out)):
        print(f"{i}: one device F {F1!r}, group F {Fg!r}, max |dG| {np.abs(np.asarray(G1) - np.asarray(Gg)).max():.3e}")
    for (F1, G1), (Fg, Gg) in zip(*out):
        assert F1 == Fg and np.array_equal(G1, Gg)


def _run_ranks(tmp_path, E, N, data):
    out, inp = str(tmp_path / "bounds"), str(tmp_path / "bounds_in.npz")
    np.savez(inp, **data)
    port = 29600 + (os.getpid() + 57) % 300
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "workers", "ipc_bounds_rank.py"), out, str(E), str(N), inp]
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return [np.load(f"{out}.rank{r}.npz") for r in range(2)]


def test_groups_and_mailbox_ranks_apply_the_slope_to_the_summed_row(qoc, oracle, tmp_path):
    """Two processes exchanging through mailboxes on the one GPU and the in-process two-shard group: the same shards, the same
    rows, the same order of summation, one slope on the complete row -- both ranks return the same bits, and they are the
    group's.  The group itself is held to the reference (penalties set everywhere, counted once)."""
    w = qoc.workloads.config("C3", E=10, N=60)
    rng = np.random.default_rng(54)
    lo, hi = np.full(w.K, -0.5), np.full(w.K, 0.7)
    lo[1], hi[1] = -INF, INF
    us = rng.uniform(-1.5, 1.5, (3, w.K, w.N))
    phi, x0, _ = draw(w, 8, 53)
    thetas = rng.uniform(-0.5, 0.5, (3, w.K, 8))
    amp, var = np.linspace(0.3, 0.9, w.K), np.linspace(0.8, 0.2, w.K)
    ops = dict(A=w.A, B=w.B, Xi=w.Xi, Xt=w.Xt, wts=w.wts)
    with engine(qoc, w, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM, max_batch=3) as eng:
        eng.set_penalties(amp, var)
        eng.set_bounds(lo, hi)
        group = [eng.eval(u) for u in us]
        names = eng.kernel_names()
        xg = eng.controls(us[0])
        Fb, Gb = eng.eval_batch(us)
        u_min, info = eng.lbfgs(us[0], iterations=3)
        eng.set_basis(phi, x0)
        group_basis = [eng.eval(th) for th in thetas]
    assert names[0] == "bounds_saturate_kernel" and names[-1] == "bounds_slope_kernel", names
    assert u_min.shape == (w.K, w.N) and info["minimum"] < group[0][0]
    for b in range(3):
        assert Fb[b] == group[b][0] and np.array_equal(Gb[b], group[b][1])
        x, s = bs.sat(us[b], lo, hi)
        F_ref, G_ref, _ = ss.composed_reference(oracle, ops, x, w.T, 0, dict(amp=amp, var=var), None, w.sys_type)
        assert_parity(group[b][0], group[b][1], F_ref, G_ref * s, w.n, what=f"group, pulse {b}")
    res = _run_ranks(tmp_path, w.E, w.N, dict(lo=lo, hi=hi, us=us, phi=phi, x0=x0, thetas=thetas, amp=amp, var=var))
    assert all(str(r["collective"]) == "ipc" for r in res), [str(r["error"]) for r in res]
    for r in res:
        assert np.array_equal(r["x"], xg)
        assert str(r["names"]).startswith("bounds_saturate_kernel") and str(r["names"]).endswith("ipc_allreduce_kernel;bounds_slope_kernel")
        assert str(r["names_basis"]).startswith("basis_expand_kernel") and str(r["names_basis"]).endswith("basis_project_kernel")
        for i in range(3):
            assert float(r["F"][i]) == group[i][0] and np.array_equal(r["G"][i], group[i][1]), i
            assert float(r["F_basis"][i]) == group_basis[i][0] and np.array_equal(r["G_basis"][i], group_basis[i][1]), i
    assert np.array_equal(res[0]["F"], res[1]["F"]) and np.array_equal(res[0]["G"], res[1]["G"])
