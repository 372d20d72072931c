"""grape_eval_vjp_multi on the GPU: several cotangent sets per trajectory call.  The defining property is that block r of the
result is bit for bit grape_eval_vjp's for set r alone -- over the 15 decomposition shapes, set counts with ragged blocks, both
derivative modes, the multi kernel forced on and the default dispatch; then the single kernel per set beyond 256 chunks,
parity against the NumPy references on its own, the transpose identity against observe_jvp_multi, linearity, member chunks,
pulse maps, standing settings, forced decompositions, the device form and its reuse, sequences, argument errors and
refusals, and trajectory_jacobian_rows against trajectory_jacobian."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import traj_exact_reference as xr  # noqa: E402
import vjp_reference as vr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_jvp_device import swept  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_traj_device import vjp_dev  # noqa: E402
from test_gpu_vjp import cplx, invariant_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5
ROWS = [r[:9] for r in SHAPES]                                # (n, m, N, E, hermitian, variant, kernel, S, W)
COUNTS = (1, 2, 3, 5, 8)                                      # 3 and 5: ragged blocks at every block size 2, 3, 6, 8
MODES = ("first_order", "exact")
MULTI = "trajectory_vjp_multi_kernel"
SINGLE = {"first_order": "trajectory_vjp_kernel", "exact": "trajectory_vjp_exact_kernel"}


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def force(monkeypatch, dispatch):
    """GRAPE_VJP_MULTI: "1" the multi kernel, "0" the single kernel per set, None the library's dispatch table"""
    if dispatch is None:
        monkeypatch.delenv("GRAPE_VJP_MULTI", raising=False)
    else:
        monkeypatch.setenv("GRAPE_VJP_MULTI", dispatch)


def singles(eng, x, O, ybars, xbars, per_member=False):
    """observe_vjp per set, stacked set-slowest: what every multi call has to reproduce bit for bit"""
    n_set = len(ybars) if ybars is not None else len(xbars)
    return np.stack([eng.observe_vjp(x, O, ybar=None if ybars is None else ybars[r], xbar_final=None if xbars is None else xbars[r],
                                     per_member=per_member) for r in range(n_set)])


def same_bits(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape)
    assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{what}: G differs in its bits"


def close(got, ref, what):
    scale = np.abs(ref).max()
    err = np.abs(np.asarray(got) - ref).max()
    print(f"{what}: |got-ref|_inf={err:.3e} |ref|_inf={scale:.3e}")
    assert scale > 0 and err <= PARITY_RTOL * scale, f"{what}: |got-ref|_inf={err:.3e} > {PARITY_RTOL * scale:.3e}"


def shape_problem(n, m, N, E, herm, variant):
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    rng = np.random.default_rng(9100 + 100 * n + 10 * m + N + E)
    return c, cplx(rng, 3, n, m), cplx(rng, 8, E, 3, N + 1), cplx(rng, 8, E, n, m)


# ---- 1: bits ---------------------------------------------------------------------------------------------------------------------
_SINGLE = {}                                                  # the single calls' results, once per (shape, mode)


@pytest.mark.parametrize("dispatch", ["1", None])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W", ROWS)
def test_block_r_is_bitwise_the_single_call(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, mode, dispatch):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, dispatch)
    c, O, ybars, xbars = shape_problem(n, m, N, E, herm, variant)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        eng.set_trajectory_derivative(mode)
        key = (n, m, N, E, herm, variant, kernel, S, W, mode)
        if key not in _SINGLE:
            _SINGLE[key] = (singles(eng, c["x"], O, ybars, xbars), singles(eng, c["x"], O, ybars[:3], None),
                            singles(eng, c["x"], None, None, xbars[:3]))
            assert SINGLE[mode] in eng.kernel_names()
            for a in _SINGLE[key]:
                a.setflags(write=False)
        want, want_y, want_x = _SINGLE[key]
        assert np.abs(want).max() > 0
        eng.observe_vjp(c["x"], None, xbar_final=xbars[0])
        one_sweep = sum(k.startswith("sweep_") for k in eng.kernel_names())      # the sweep kernels of ONE evaluation
        for n_set in COUNTS:
            got = eng.observe_vjp_multi(c["x"], O, ybars[:n_set], xbars[:n_set])
            names = eng.kernel_names()
            assert got.shape == (n_set, c["K"], N)
            same_bits(got, want[:n_set], f"n={n} m={m} N={N} E={E} {kernel} {mode} n_set={n_set}")
            assert swept(names) and (MULTI in names or SINGLE[mode] in names), names
            if mode == "first_order" and dispatch == "1":
                assert MULTI in names and SINGLE[mode] not in names, names
            if mode == "exact":
                assert names.count("traj_frechet_rows_kernel") == n_set and MULTI not in names, names
                assert sum(k.startswith("sweep_") for k in names) == one_sweep >= 1, names      # behind ONE sweep
        # the expectation values' cotangents alone and the final states' alone (n_obs = 0)
        same_bits(eng.observe_vjp_multi(c["x"], O, ybars=ybars[:3]), want_y, "ybars alone")
        same_bits(eng.observe_vjp_multi(c["x"], None, xbars_final=xbars[:3]), want_x, "xbars_final alone")


# ---- 2: more than 256 chunks per member ------------------------------------------------------------------------------------------
def test_more_than_256_chunks_take_the_single_kernel_per_set(qoc, monkeypatch):
    """n = 2, N = 300 with one slice per lane: 300 chunks on five waves, beyond the multi instance's 256 threads"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", "lane")
    force(monkeypatch, "1")
    c = make_case(9150, 2, 2, 300, 2, hermitian=False)
    rng = np.random.default_rng(9151)
    O, ybars, xbars = cplx(rng, 3, 2, 2), cplx(rng, 5, 2, 3, 301), cplx(rng, 5, 2, 2, 2)
    with engine(qoc, c, slices_per_lane=1, waves_per_member=5) as eng:
        info = eng.info
        assert info["slices_per_lane"] == 1 and 64 * info["waves_per_member"] // (2 if info["lane_pair"] else 1) > 256, info
        want = singles(eng, c["x"], O, ybars, xbars)
        one_sweep = sum(k.startswith("sweep_") for k in eng.kernel_names())
        got = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        names = eng.kernel_names()
    assert names.count("trajectory_vjp_kernel") == 5 and MULTI not in names, names
    assert sum(k.startswith("sweep_") for k in names) == one_sweep >= 1, names
    same_bits(got, want, "300 chunks")


# ---- 3: parity, on its own ---------------------------------------------------------------------------------------------------------
_REF = {}


def parity_reference(key, c, O, ybars, xbars, mode):
    if key not in _REF:
        if mode == "exact":
            PL = xr.slice_derivatives(c["A"], c["B"], c["x"], c["T"], c["variant"])
            per = [xr.exact_vjp_ref(c["A"], c["B"], c["Xi"], c["x"], c["T"], O, yb, xb, False, c["variant"], PL)
                   for yb, xb in zip(ybars, xbars)]
        else:
            per = [vr.vjp_ref(c["A"], c["B"], c["Xi"], c["x"], c["T"], O, yb, xb, False, c["variant"]) for yb, xb in zip(ybars, xbars)]
        _REF[key] = np.stack(per)
        _REF[key].setflags(write=False)
    return _REF[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W", ROWS)
def test_parity_against_the_numpy_references(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, mode):
    """three sets (one ragged block at block size 2, one whole block at 3) against the double sum / expm_frechet"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, "1")
    c, O, ybars, xbars = shape_problem(n, m, N, E, herm, variant)
    ref = parity_reference((n, m, N, E, herm, variant, mode), c, O, ybars[:3], xbars[:3], mode)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        eng.set_trajectory_derivative(mode)
        G = eng.observe_vjp_multi(c["x"], O, ybars[:3], xbars[:3])
        assert (MULTI if mode == "first_order" else SINGLE[mode]) in eng.kernel_names()
    for r in range(3):
        close(G[r], ref[r], f"n={n} m={m} N={N} E={E} {kernel} {mode} set {r}")


# ---- 4: the transpose identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,m,N,E,herm,kernel", [(4, 4, 65, 3, True, "pair"), (3, 1, 64, 3, False, "lane"), (2, 2, 130, 5, True, "lane")])
def test_transpose_identity_against_the_push_forward(qoc, monkeypatch, n, m, N, E, herm, kernel, mode):
    """sum Re(conj(ybar_r) ydot_d) + sum Re(conj(xbar_r) Xdot_d) = sum(G_r xdot_d) for every pair (set r, direction d), at
    the bar of the transpose test of test_gpu_jvp_multi.py"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, "1")
    c = make_case(5200 + 10 * n + m, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(9311 + n)
    O, xdots = cplx(rng, 3, n, m), rng.standard_normal((3, c["K"], N))
    ybars, xbars = cplx(rng, 5, E, 3, N + 1), cplx(rng, 5, E, n, m)
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        G = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        if mode == "first_order":
            assert MULTI in eng.kernel_names()
        yd, Xd = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
    for r in range(5):
        for d in range(3):
            lhs, mag = jr.pairing(ybars[r], yd[d], xbars[r], Xd[d])
            rhs, scale = float(np.sum(G[r] * xdots[d])), float(np.sum(np.abs(G[r] * xdots[d]))) + mag
            print(f"n={n} m={m} {mode} set {r} direction {d}: |lhs - rhs| / scale = {abs(lhs - rhs) / scale:.2e}")
            assert abs(lhs) > 0 and abs(lhs - rhs) <= 1e-12 * scale


# ---- 5: linearity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", [(3, 2, 23, 2, False, "lane", 2, 0), (4, 4, 65, 3, True, "pair", 1, 3),
                                                     (2, 2, 130, 5, True, "lane", 0, 0)])
def test_scaling_and_zero_sets_are_exact(qoc, monkeypatch, n, m, N, E, herm, kernel, S, W, mode):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, "1")
    c = make_case(5300 + n, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(9411)
    O, ybars, xbars = cplx(rng, 3, n, m), cplx(rng, 5, E, 3, N + 1), cplx(rng, 5, E, n, m)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        eng.set_trajectory_derivative(mode)
        base = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        ys, xs = ybars.copy(), xbars.copy()
        ys[1] *= 2.0
        xs[1] *= 2.0
        ys[4] *= -1.0
        xs[4] *= -1.0
        ys[2] = 0.0                                           # a zero set inside a block
        xs[2] = 0.0
        got = eng.observe_vjp_multi(c["x"], O, ys, xs)
        if mode == "first_order":
            assert MULTI in eng.kernel_names()
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[3], base[3])     # the neighbours are not disturbed
    assert np.array_equal(got[1], 2.0 * base[1]) and np.array_equal(got[4], -base[4])
    assert not got[2].any() and not np.isnan(got[2]).any() and base[2].any()       # exactly zero


# ---- 6: other forms and sequences ------------------------------------------------------------------------------------------------
def invariant_sets(herm=False, E=10, n_set=5):
    c, O, _, _ = invariant_case(herm, E)
    rng = np.random.default_rng(9501 + E)
    return c, O, cplx(rng, n_set, E, 4, 41), cplx(rng, n_set, E, 3, 3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("herm,E,members", [(False, 10, 4), (True, 70, 24)])
def test_member_chunked_context_returns_the_unchunked_bits(qoc, monkeypatch, herm, E, members, mode):
    """the groups' partial sums are kept per set across the member blocks (blocks of 4 of 10 split one group three ways,
    blocks of 24 of 70 cut through every group)"""
    force(monkeypatch, "1")
    c, O, ybars, xbars = invariant_sets(herm, E)
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        want = singles(eng, c["x"], O, ybars, xbars)
        whole = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        info = eng.info
    same_bits(whole, want, "unchunked")
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, herm, members)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < E and eng.info["member_chunk"] % 32 != 0, eng.info["member_chunk"]
        eng.set_trajectory_derivative(mode)
        got = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        if mode == "first_order":
            assert MULTI in eng.kernel_names()
    same_bits(got, want, f"member-chunked, {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pulse_map", ["basis", "bounds", "both"])
def test_block_r_is_the_single_call_under_a_pulse_map(qoc, monkeypatch, pulse_map, mode):
    force(monkeypatch, "1")
    c = make_case(4401, 4, 2, 50, 3, hermitian=False)
    N, K = c["N"], c["K"]
    rng = np.random.default_rng(9611)
    O, ybars, xbars = cplx(rng, 2, 4, 2), cplx(rng, 5, 3, 2, N + 1), cplx(rng, 5, 3, 4, 2)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        cols = N
        if pulse_map != "bounds":
            eng.set_basis(phi, 0.2 * rng.standard_normal((K, N)))
            cols = 5
        if pulse_map != "basis":
            eng.set_bounds(np.array([-0.8, -0.5]), np.array([0.9, 0.6]))
        theta = 0.5 * rng.standard_normal((K, cols))
        want = singles(eng, theta, O, ybars, xbars)
        got = eng.observe_vjp_multi(theta, O, ybars, xbars)
        names = eng.kernel_names()
    assert got.shape == (5, K, cols) and (MULTI in names if mode == "first_order" else SINGLE[mode] in names), names
    same_bits(got, want, f"{pulse_map}, {mode}")


@pytest.mark.parametrize("standing", ["running_cost", "penalties", "risk"])
def test_standing_costs_do_not_enter(qoc, monkeypatch, standing):
    force(monkeypatch, "1")
    c, O, ybars, xbars = invariant_sets(n_set=3)
    with engine(qoc, c) as eng:
        want = singles(eng, c["x"], O, ybars, xbars)
        F0, _ = eng.eval(c["x"])
        if standing == "running_cost":
            eng.set_running_cost(c["R"], c["rho"])
        elif standing == "penalties":
            eng.set_penalties(np.array([0.3, 0.1]), np.array([0.05, 0.2]))
        else:
            eng.set_risk(2.0)
        F1, _ = eng.eval(c["x"])
        got = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        also = singles(eng, c["x"], O, ybars, xbars)
        F2, _ = eng.eval(c["x"])
    assert F1 != F0 and F2 == F1                              # the cost is in force, before and after
    same_bits(got, want, standing)
    same_bits(also, want, standing + ", single calls")


@pytest.mark.parametrize("n,m,kernel,S,W", [(2, 2, "lane", 5, 2), (3, 3, "lane", 1, 4), (4, 4, "pair", 7, 1), (4, 2, "lane", 2, 3)])
def test_forced_slices_per_lane_and_waves_per_member(qoc, monkeypatch, n, m, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, "1")
    c = make_case(9800 + n, n, m, 97, 2, hermitian=False)
    rng = np.random.default_rng(9811)
    O, ybars, xbars = cplx(rng, 2, n, m), cplx(rng, 5, 2, 2, 98), cplx(rng, 5, 2, n, m)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["slices_per_lane"] == S and eng.info["waves_per_member"] == W
        want = singles(eng, c["x"], O, ybars, xbars)
        got = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        assert MULTI in eng.kernel_names()
    same_bits(got, want, f"S={S} W={W}")


def multi_dev(torch, eng, x, O, ybars, xbars):
    """observe_vjp_multi_device -> numpy after a synchronise; x=None: reuse"""
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    G = eng.observe_vjp_multi_device(d(x), d(O), d(ybars), d(xbars))
    torch.cuda.synchronize()
    return G.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("herm", [False, True])
def test_device_form_host_form_and_reuse_agree_bitwise(qoc, torch, monkeypatch, herm, mode):
    force(monkeypatch, "1")
    c, O, ybars, xbars = invariant_sets(herm, n_set=11)       # 11: a block of 8 and a ragged one by reuse
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        host = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        same_bits(host, singles(eng, c["x"], O, ybars, xbars), "host = single calls")
        got = multi_dev(torch, eng, c["x"], O, ybars[:5], xbars[:5])
        names = eng.kernel_names()
        assert swept(names) and (MULTI in names if mode == "first_order" else SINGLE[mode] in names), names
        same_bits(got, host[:5], "device = host")
        again = multi_dev(torch, eng, None, O, ybars[:5], xbars[:5])          # d_x = NULL: along the stored trajectory
        names = eng.kernel_names()
        assert not swept(names) and (MULTI in names if mode == "first_order" else SINGLE[mode] in names), names
        same_bits(again, got, "reuse = the call with d_x")
        G1 = vjp_dev(torch, eng, None, O, ybars[0], xbars[0], False, reuse=True)  # the flag is still set
        assert np.array_equal(G1, host[0])
        long = multi_dev(torch, eng, c["x"], O, ybars, xbars)  # more than 8: the second block reuses
        same_bits(long, host, "11 sets")
        assert not swept(eng.kernel_names())                  # (the names of the last call: the reuse block)
        same_bits(multi_dev(torch, eng, None, O, ybars[:3], None), singles(eng, c["x"], O, ybars[:3], None), "ybars alone, reuse")


def test_any_setting_clears_the_flag_and_chunked_contexts_answer_not_ready(qoc, torch, monkeypatch):
    force(monkeypatch, "1")
    c, O, ybars, xbars = invariant_sets(n_set=3)

    def reuse_refused(eng, word):
        with pytest.raises(qoc.GrapeError) as ei:
            multi_dev(torch, eng, None, O, ybars, xbars)
        assert ei.value.status == -5 and "reuse" in str(ei.value) and "grape_eval_vjp_multi_device" in str(ei.value), str(ei.value)
        assert word in str(ei.value), str(ei.value)

    with engine(qoc, c) as eng:
        reuse_refused(eng, "trajectory")                      # a fresh context
        want = multi_dev(torch, eng, c["x"], O, ybars, xbars)
        for touch in (lambda: eng.set_penalties(0.1, 0.2), lambda: eng.set_trajectory_derivative("exact"),
                      lambda: eng.set_trajectory_derivative("first_order"), lambda: eng.set_risk(1.0), lambda: eng.eval(c["x"])):
            multi_dev(torch, eng, c["x"], O, ybars, xbars)
            touch()
            reuse_refused(eng, "trajectory")
            reuse_refused(eng, "trajectory")                  # (a refused call leaves the flag clear)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, False, 4)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < c["E"]
        F0, G0 = eng.eval(c["x"])
        same_bits(multi_dev(torch, eng, c["x"], O, ybars, xbars), want, "member-chunked device form")
        reuse_refused(eng, "member_chunk")
        F, G = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G, G0)


def test_workspace_bytes_count_the_scratch(qoc, torch, monkeypatch):
    """five sets against one: four more images of the members' rows ((K N + 1) doubles per member), of the groups' sums (K N
    per group of 32 members) and, under a pulse map, of the summed and the projected rows (K N + 1 doubles each)"""
    force(monkeypatch, "1")
    c = make_case(4401, 4, 4, 50, 3, hermitian=False)
    rng = np.random.default_rng(9913)
    O, K, N, E = cplx(rng, 2, 4, 4), c["K"], c["N"], c["E"]
    ybars, xbars = cplx(rng, 5, E, 2, N + 1), cplx(rng, 5, E, 4, 4)
    with engine(qoc, c) as eng:
        assert eng.info["member_chunk"] >= E
        u = 0.5 * rng.standard_normal((K, N))
        multi_dev(torch, eng, u, O, ybars[:1], xbars[:1])
        one = eng.info["workspace_bytes"]
        multi_dev(torch, eng, u, O, ybars, xbars)
        five = eng.info["workspace_bytes"]
        assert five - one == 4 * 8 * (E * (K * N + 1) + K * N), (one, five)
        eng.set_bounds(np.array([-0.8, -0.5]), np.array([0.9, 0.6]))
        multi_dev(torch, eng, u, O, ybars[:1], xbars[:1])
        b1 = eng.info["workspace_bytes"]
        multi_dev(torch, eng, u, O, ybars, xbars)
        b5 = eng.info["workspace_bytes"]
        assert b5 - b1 == 4 * 8 * 2 * (K * N + 1), (b1, b5)


@pytest.mark.parametrize("mode", MODES)
def test_eval_multi_eval_and_the_kernel_names(qoc, monkeypatch, mode):
    c, O, ybars, xbars = invariant_sets()
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        force(monkeypatch, "1")
        on = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        names_on = eng.kernel_names()
        F1, G1 = eng.eval(c["x"])
        assert eng.kernel_names() == names0
        force(monkeypatch, "0")
        off = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
        names_off = eng.kernel_names()
        F2, G2 = eng.eval(c["x"])
        again = eng.observe_vjp_multi(c["x"], O, ybars, xbars)
    assert F1 == F0 and F2 == F0 and np.array_equal(G1, G0) and np.array_equal(G2, G0)
    if mode == "first_order":
        assert MULTI in names_on and SINGLE[mode] not in names_on, names_on
    assert names_off.count(SINGLE[mode]) == 5 and MULTI not in names_off, names_off
    assert sum(k.startswith("sweep_") for k in names_off) == sum(k.startswith("sweep_") for k in names0)        # ONE sweep
    assert not any("vjp" in k for k in names0)
    same_bits(on, off, "forced on = forced off")
    same_bits(again, off, "call to call")


# ---- 7: arguments and refusals -----------------------------------------------------------------------------------------------------
def raw_call(qoc, eng, x, n_set, n_obs, per_member, O, ybar, Xbar, G):
    lib = qoc.load_library()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.grape_eval_vjp_multi(eng._h, ptr(x), n_set, n_obs, per_member, ptr(O), ptr(ybar), ptr(Xbar), ptr(G))
    return rc, lib.grape_last_error(eng._h).decode()


def test_invalid_arguments(qoc):
    c = make_case(4601, 4, 4, 20, 2)
    E, N, K = c["E"], c["N"], c["K"]
    rng = np.random.default_rng(9915)
    O = cplx(rng, 2, 4, 4)
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])

        def evaluates_as_before():
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)

        xf = np.ascontiguousarray(c["x"].T)
        Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
        yb, Xb, G = cplx(rng, 3, E, 2, N + 1), cplx(rng, 3, E, 4, 4), np.empty((3, N, K))
        for n_set in (0, 9, -1):
            rc, msg = raw_call(qoc, eng, xf, n_set, 2, 0, Of, yb, Xb, G)
            assert rc == -1 and "grape_eval_vjp_multi" in msg and f"n_set = {n_set}" in msg, (rc, msg)
            evaluates_as_before()
        bad_args = [
            (None, 3, 2, 0, Of, yb, Xb, G),                   # null x
            (xf, 3, 2, 0, Of, yb, Xb, None),                  # null G
            (xf, 3, 2, 0, Of, None, None, G),                 # ybar and Xbar_final both NULL
            (xf, 3, -1, 0, Of, yb, Xb, G), (xf, 3, 17, 0, Of, yb, Xb, G),         # n_obs outside 0..16
            (xf, 3, 0, 0, Of, yb, Xb, G),                     # n_obs = 0 with a non-NULL ybar
            (xf, 3, 2, 0, None, yb, Xb, G),                   # n_obs > 0 with a NULL O
            (xf, 3, 2, 2, Of, yb, Xb, G), (xf, 3, 2, -1, Of, yb, Xb, G),          # per_member other than 0 or 1
        ]
        for args in bad_args:
            rc, msg = raw_call(qoc, eng, *args)
            assert rc == -1 and "grape_eval_vjp_multi" in msg, (rc, msg)
            evaluates_as_before()
        for which in range(3):                                # a non-finite entry of O, and of the LAST set of ybar, Xbar_final
            arrs = [Of.copy(), yb.copy(), Xb.copy()]
            arrs[which].reshape(-1)[-5] = [np.nan, np.inf, complex(0, -np.inf)][which]
            rc, msg = raw_call(qoc, eng, xf, 3, 2, 0, arrs[0], arrs[1], arrs[2], G)
            assert rc == -1 and "not finite" in msg and ["O[", "ybar[", "Xbar_final["][which] in msg, (rc, msg)
            evaluates_as_before()
        rc, msg = raw_call(qoc, eng, xf, 3, 0, 0, None, None, Xb, G)            # valid corners
        assert rc == 0, msg
        rc, msg = raw_call(qoc, eng, xf, 3, 2, 0, Of, yb, None, G)
        assert rc == 0, msg
        Xs = np.swapaxes(Xb, -1, -2)
        for kw in (dict(ops=O, ybars=yb[:, :, :1]), dict(ops=O, xbars_final=Xs[:, :, :3]), dict(ops=None, ybars=yb), dict(ops=O),
                   dict(ops=O, ybars=yb, xbars_final=Xs[:2]), dict(ops=O, ybars=yb[0]), dict(ops=O, ybars=yb[:0])):
            with pytest.raises(ValueError):
                eng.observe_vjp_multi(c["x"], **kw)
        evaluates_as_before()
    lib = qoc.load_library()                                  # before grape_set_operators
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.grape_eval_vjp_multi(h, p(xf), 3, 2, 0, p(Of), p(yb), None, p(G)) == -5
        assert b"operators not set" in lib.grape_last_error(h)
        assert lib.grape_eval_vjp_multi_device(h, None, 3, 2, 0, p(Of), p(yb), None, p(G), None) == -5
    finally:
        lib.grape_destroy(h)
    assert lib.grape_eval_vjp_multi(None, None, 1, 0, 0, None, None, None, None) == -1
    assert lib.grape_eval_vjp_multi_device(None, None, 1, 0, 0, None, None, None, None, None) == -1


def test_refusals(qoc):
    c = make_case(4501, 4, 4, 20, 2)
    GE = qoc.GrapeError

    def refused(eng, case, word):
        F0, G0 = eng.eval(case["x"])                          # the bits from before the refusal
        with pytest.raises(GE) as ei:
            eng.observe_vjp_multi(case["x"], None, xbars_final=np.ones((2,) + case["Xi"].shape))
        assert ei.value.status == -2 and word in str(ei.value) and "grape_eval_vjp_multi" in str(ei.value), str(ei.value)
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


# ---- 8: Jacobian rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_jacobian_rows_against_the_columns(qoc, torch, mode):
    """(n, m, N, E) = (4, 4, 12, 2): five rows (two blocks of cotangent sets, the second by reuse) against the matching entries
    of trajectory_jacobian, the forward mode's columns of the same linearisation -- the transpose identity entry by entry, at
    the parity bar"""
    c = make_case(9916, 4, 4, 12, 2, hermitian=False)
    O = cplx(np.random.default_rng(9917), 3, 4, 4)
    rows = [(0, 0, 12), (1, 2, 5), (0, 1, 1), (1, 0, 0), (1, 1, 12)]
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        Jr = eng.trajectory_jacobian_rows(c["x"], O, rows)
        Jc = eng.trajectory_jacobian(c["x"], O)                # (K N, E, n_obs, N+1)
    assert Jr.shape == (5, c["K"], 12) and Jr.dtype == np.complex128
    want = np.stack([Jc[:, k, j, s].reshape(c["K"], 12) for k, j, s in rows])
    assert not Jr[3].any()                                    # y at s = 0 does not depend on x
    close(Jr, want, f"trajectory_jacobian_rows against trajectory_jacobian, {mode}")
