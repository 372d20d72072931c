"""grape_eval_jvp_multi on the GPU: several tangent directions per trajectory call.  The defining property is that block d of
the result is bit for bit grape_eval_jvp's for direction d alone -- over the 15 decomposition shapes, direction counts with
ragged blocks, both derivative modes, the multi kernel forced on and the default dispatch; then parity against the NumPy
references on its own, the transpose identity, linearity, member chunks, pulse maps, standing settings, the device form and
its reuse, sequences, argument errors and refusals, and trajectory_jacobian against central differences."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import traj_exact_reference as xr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_jvp_device import swept  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_traj_device import vjp_dev  # noqa: E402
from test_gpu_vjp import cplx, invariant_case  # noqa: E402
from test_jvp_multi_host import stack_directions  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5
ROWS = [r[:9] for r in SHAPES]                                # (n, m, N, E, hermitian, variant, kernel, S, W)
COUNTS = (1, 2, 3, 5, 8)                                      # 3 and 5: ragged blocks at every block size 2, 3, 4, 8
MODES = ("first_order", "exact")
MULTI = {"first_order": "trajectory_jvp_multi_kernel", "exact": "trajectory_jvp_multi_exact_kernel"}
SINGLE = {"first_order": "trajectory_jvp_kernel", "exact": "trajectory_jvp_exact_kernel"}


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def force(monkeypatch, dispatch):
    """GRAPE_JVP_MULTI: "1" the multi kernel, "0" the single kernel per direction, None the library's dispatch table"""
    if dispatch is None:
        monkeypatch.delenv("GRAPE_JVP_MULTI", raising=False)
    else:
        monkeypatch.setenv("GRAPE_JVP_MULTI", dispatch)


def singles(eng, x, xdots, O, per_member=False):
    """observe_jvp per direction, stacked direction-slowest: what every multi call has to reproduce bit for bit"""
    return stack_directions([eng.observe_jvp(x, xd, O, per_member=per_member, final=True) for xd in xdots])


def same_bits(got, want, what):
    for g, w, name in zip(got, want, ("ydot", "Xdot_final")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{what}: {name} differs in its bits"


def close(got, ref, what):
    scale = np.abs(ref).max()
    err = np.abs(np.asarray(got) - ref).max()
    print(f"{what}: |got-ref|_inf={err:.3e} |ref|_inf={scale:.3e}")
    assert scale > 0 and err <= PARITY_RTOL * scale, f"{what}: |got-ref|_inf={err:.3e} > {PARITY_RTOL * scale:.3e}"


def shape_problem(n, m, N, E, herm, variant):
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    rng = np.random.default_rng(9000 + 100 * n + 10 * m + N + E)
    return c, cplx(rng, 3, n, m), rng.standard_normal((8, c["K"], N))


# ---- 1: bits ---------------------------------------------------------------------------------------------------------------------
_SINGLE = {}                                                  # the single calls' results, once per (shape, mode)


@pytest.mark.parametrize("dispatch", ["1", None])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W", ROWS)
def test_block_d_is_bitwise_the_single_call(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, mode, dispatch):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, dispatch)
    c, O, xdots = shape_problem(n, m, N, E, herm, variant)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        eng.set_trajectory_derivative(mode)
        key = (n, m, N, E, herm, variant, kernel, S, W, mode)
        if key not in _SINGLE:
            _SINGLE[key] = singles(eng, c["x"], xdots, O)
            assert SINGLE[mode] in eng.kernel_names()
            for a in _SINGLE[key]:
                a.setflags(write=False)
        want = _SINGLE[key]
        assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0
        for n_dir in COUNTS:
            got = eng.observe_jvp_multi(c["x"], xdots[:n_dir], O, final=True)
            names = eng.kernel_names()
            assert got[0].shape == (n_dir, E, 3, N + 1) and got[1].shape == (n_dir, E, n, m)
            same_bits(got, (want[0][:n_dir], want[1][:n_dir]), f"n={n} m={m} N={N} E={E} {kernel} {mode} n_dir={n_dir}")
            assert swept(names) and (MULTI[mode] in names or SINGLE[mode] in names), names
            if dispatch == "1":
                assert MULTI[mode] in names and SINGLE[mode] not in names, names
            if mode == "exact":
                assert names.count("traj_frechet_dir_kernel") == n_dir, names
        # the final tangents alone (n_obs = 0) and the traces alone
        Xonly = eng.observe_jvp_multi(c["x"], xdots[:3], None, final=True)[1]
        yonly = eng.observe_jvp_multi(c["x"], xdots[:3], O)
        same_bits((yonly, Xonly), (want[0][:3], want[1][:3]), "one output at a time")


# ---- 2: parity, on its own ---------------------------------------------------------------------------------------------------------
_REF = {}


def parity_reference(key, c, O, xdots, mode):
    if key not in _REF:
        if mode == "exact":
            PL = xr.slice_derivatives(c["A"], c["B"], c["x"], c["T"], c["variant"])
            per = [xr.exact_jvp_ref(c["A"], c["B"], c["Xi"], c["x"], xd, c["T"], O, False, c["variant"], PL) for xd in xdots]
        else:
            per = [jr.jvp_ref(c["A"], c["B"], c["Xi"], c["x"], xd, c["T"], O, False, c["variant"]) for xd in xdots]
        _REF[key] = stack_directions(per)
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W", ROWS)
def test_parity_against_the_numpy_references(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, mode):
    """three directions (one ragged block at block size 2, one whole block at 3) against the double sum / expm_frechet"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, "1")
    c, O, xdots = shape_problem(n, m, N, E, herm, variant)
    y_ref, X_ref = parity_reference((n, m, N, E, herm, variant, mode), c, O, xdots[:3], mode)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        eng.set_trajectory_derivative(mode)
        yd, Xd = eng.observe_jvp_multi(c["x"], xdots[:3], O, final=True)
        assert MULTI[mode] in eng.kernel_names()
    for d in range(3):
        what = f"n={n} m={m} N={N} E={E} {kernel} {mode} direction {d}"
        close(yd[d], y_ref[d], what + " ydot")
        close(Xd[d], X_ref[d], what + " Xdot_final")
    assert not yd[:, :, :, 0].any()                           # row 0 is zero and written


# ---- 3: the transpose identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,m,N,E,herm,kernel", [(4, 4, 65, 3, True, "pair"), (3, 1, 64, 3, False, "lane"), (2, 2, 130, 5, True, "lane")])
def test_transpose_identity_against_the_pull_back(qoc, monkeypatch, n, m, N, E, herm, kernel, mode):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, "1")
    c = make_case(5200 + 10 * n + m, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(9301 + n)
    O, xdots = cplx(rng, 3, n, m), rng.standard_normal((5, c["K"], N))
    ybar, xbar = cplx(rng, E, 3, N + 1), cplx(rng, E, n, m)
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        yd, Xd = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        assert MULTI[mode] in eng.kernel_names()
        G = eng.observe_vjp(c["x"], O, ybar=ybar, xbar_final=xbar)
    for d in range(5):
        lhs, mag = jr.pairing(ybar, yd[d], xbar, Xd[d])
        rhs, scale = float(np.sum(G * xdots[d])), float(np.sum(np.abs(G * xdots[d]))) + mag
        print(f"n={n} m={m} {mode} direction {d}: |lhs - rhs| / scale = {abs(lhs - rhs) / scale:.2e}")
        assert abs(lhs) > 0 and abs(lhs - rhs) <= 1e-12 * scale


# ---- 4: linearity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,m,N,E,herm,kernel,S,W", [(3, 2, 23, 2, False, "lane", 2, 0), (4, 4, 65, 3, True, "pair", 1, 3),
                                                     (2, 2, 130, 5, True, "lane", 0, 0)])
def test_scaling_and_zero_directions_are_exact(qoc, monkeypatch, n, m, N, E, herm, kernel, S, W, mode):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, "1")
    c = make_case(5300 + n, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(9401)
    O, xdots = cplx(rng, 3, n, m), rng.standard_normal((5, c["K"], N))
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        eng.set_trajectory_derivative(mode)
        base = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        scaled = xdots.copy()
        scaled[1] *= 2.0
        scaled[4] *= -1.0
        scaled[2] = 0.0                                       # a zero direction inside a block
        got = eng.observe_jvp_multi(c["x"], scaled, O, final=True)
        assert MULTI[mode] in eng.kernel_names()
    assert np.abs(base[0]).min(initial=1.0, where=np.abs(base[0]) > 0) > 0
    for b, g in zip(base, got):
        assert np.array_equal(g[0], b[0]) and np.array_equal(g[3], b[3])          # the neighbours are not disturbed
        assert np.array_equal(g[1], 2.0 * b[1]) and np.array_equal(g[4], -b[4])
        assert not g[2].any() and not np.isnan(g[2]).any() and b[2].any()          # exactly zero


# ---- 5: member chunks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("herm,E,members", [(False, 10, 4), (True, 70, 24)])
def test_member_chunked_context_returns_the_unchunked_bits(qoc, monkeypatch, herm, E, members, mode):
    force(monkeypatch, "1")
    c, O, _, _ = invariant_case(herm, E)
    xdots = np.random.default_rng(9501).standard_normal((5, c["K"], c["N"]))
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        want = singles(eng, c["x"], xdots, O)
        whole = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        info = eng.info
    same_bits(whole, want, "unchunked")
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, herm, members)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < E and eng.info["member_chunk"] % 32 != 0, eng.info["member_chunk"]
        eng.set_trajectory_derivative(mode)
        got = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        assert MULTI[mode] in eng.kernel_names()
    same_bits(got, want, f"member-chunked, {mode}")


# ---- 6: basis, bounds, both --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pulse_map", ["basis", "bounds", "both"])
def test_block_d_is_the_single_call_under_a_pulse_map(qoc, monkeypatch, pulse_map, mode):
    force(monkeypatch, "1")
    c = make_case(4401, 4, 2, 50, 3, hermitian=False)
    N, K = c["N"], c["K"]
    rng = np.random.default_rng(9601)
    O = cplx(rng, 2, 4, 2)
    phi = np.concatenate([np.ones((N, 1)), qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0]))], axis=1)
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        cols = N
        if pulse_map != "bounds":
            eng.set_basis(phi, 0.2 * rng.standard_normal((K, N)))
            cols = 5
        if pulse_map != "basis":
            eng.set_bounds(np.array([-0.8, -0.5]), np.array([0.9, 0.6]))
        theta, thetadots = 0.5 * rng.standard_normal((K, cols)), rng.standard_normal((5, K, cols))
        want = singles(eng, theta, thetadots, O)
        got = eng.observe_jvp_multi(theta, thetadots, O, final=True)
        names = eng.kernel_names()
    tangent = "bounds_tangent_kernel" if pulse_map == "bounds" else "basis_expand_kernel"
    assert names.count(tangent) >= 5 and MULTI[mode] in names, names          # the tangent map runs per direction
    same_bits(got, want, f"{pulse_map}, {mode}")


# ---- 7: standing settings ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("standing", ["running_cost", "penalties", "risk"])
def test_standing_costs_do_not_enter(qoc, monkeypatch, standing):
    force(monkeypatch, "1")
    c, O, _, _ = invariant_case()
    xdots = np.random.default_rng(9701).standard_normal((3, c["K"], c["N"]))
    with engine(qoc, c) as eng:
        want = singles(eng, c["x"], xdots, O)
        F0, _ = eng.eval(c["x"])
        if standing == "running_cost":
            eng.set_running_cost(c["R"], c["rho"])
        elif standing == "penalties":
            eng.set_penalties(np.array([0.3, 0.1]), np.array([0.05, 0.2]))
        else:
            eng.set_risk(2.0)
        F1, _ = eng.eval(c["x"])
        got = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        also = singles(eng, c["x"], xdots, O)
        F2, _ = eng.eval(c["x"])
    assert F1 != F0 and F2 == F1                              # the cost is in force, before and after
    same_bits(got, want, standing)
    same_bits(also, want, standing + ", single calls")


@pytest.mark.parametrize("n,m,kernel,S,W", [(2, 2, "lane", 5, 2), (3, 3, "lane", 1, 4), (4, 4, "pair", 7, 1), (4, 2, "lane", 2, 3)])
def test_forced_slices_per_lane_and_waves_per_member(qoc, monkeypatch, n, m, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    force(monkeypatch, "1")
    c = make_case(9800 + n, n, m, 97, 2, hermitian=False)
    rng = np.random.default_rng(9801)
    O, xdots = cplx(rng, 2, n, m), rng.standard_normal((5, c["K"], 97))
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["slices_per_lane"] == S and eng.info["waves_per_member"] == W
        want = singles(eng, c["x"], xdots, O)
        got = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        assert MULTI["first_order"] in eng.kernel_names()
    same_bits(got, want, f"S={S} W={W}")


# ---- 8: the device form ------------------------------------------------------------------------------------------------------------
def multi_dev(torch, eng, x, xdots, O, final=True):
    """observe_jvp_multi_device -> numpy after a synchronise; x=None: reuse"""
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = eng.observe_jvp_multi_device(d(x), d(xdots), d(O), final=final)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out) if final else out.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("herm", [False, True])
def test_device_form_host_form_and_reuse_agree_bitwise(qoc, torch, monkeypatch, herm, mode):
    force(monkeypatch, "1")
    c, O, yb, xb = invariant_case(herm)
    xdots = np.random.default_rng(9901).standard_normal((11, c["K"], c["N"]))      # 11: a block of 8 and a ragged one by reuse
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        host = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        got = multi_dev(torch, eng, c["x"], xdots[:5], O)
        names = eng.kernel_names()
        assert swept(names) and MULTI[mode] in names, names
        same_bits(got, (host[0][:5], host[1][:5]), "device = host")
        again = multi_dev(torch, eng, None, xdots[:5], O)     # d_x = NULL: along the stored trajectory
        names = eng.kernel_names()
        assert not swept(names) and MULTI[mode] in names, names
        same_bits(again, got, "reuse = the call with d_x")
        G = vjp_dev(torch, eng, None, O, yb, xb, False, reuse=True)              # the flag is still set
        assert np.array_equal(G, eng.observe_vjp(c["x"], O, ybar=yb, xbar_final=xb))
        long = multi_dev(torch, eng, c["x"], xdots, O)        # more than 8: the second block reuses
        same_bits(long, host, "11 directions")
        assert not swept(eng.kernel_names())                  # (the names of the last call: the reuse block)
        yonly = multi_dev(torch, eng, None, xdots[:3], O, final=False)
        assert np.array_equal(yonly, host[0][:3])


def test_any_setting_clears_the_flag_and_chunked_contexts_answer_not_ready(qoc, torch, monkeypatch):
    force(monkeypatch, "1")
    c, O, _, _ = invariant_case()
    xdots = np.random.default_rng(9902).standard_normal((3, c["K"], c["N"]))

    def reuse_refused(eng, word):
        with pytest.raises(qoc.GrapeError) as ei:
            multi_dev(torch, eng, None, xdots, O)
        assert ei.value.status == -5 and "reuse" in str(ei.value) and "grape_eval_jvp_multi_device" in str(ei.value), str(ei.value)
        assert word in str(ei.value), str(ei.value)

    with engine(qoc, c) as eng:
        reuse_refused(eng, "trajectory")                      # a fresh context
        want = multi_dev(torch, eng, c["x"], xdots, O)
        for touch in (lambda: eng.set_penalties(0.1, 0.2), lambda: eng.set_trajectory_derivative("exact"),
                      lambda: eng.set_trajectory_derivative("first_order"), lambda: eng.set_risk(1.0), lambda: eng.eval(c["x"])):
            multi_dev(torch, eng, c["x"], xdots, O)
            touch()
            reuse_refused(eng, "trajectory")
            reuse_refused(eng, "trajectory")                  # (a refused call leaves the flag clear)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, False, 4)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < c["E"]
        F0, G0 = eng.eval(c["x"])
        same_bits(multi_dev(torch, eng, c["x"], xdots, O), want, "member-chunked device form")
        reuse_refused(eng, "member_chunk")
        F, G = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G, G0)


def test_workspace_bytes_count_the_scratch(qoc, torch, monkeypatch):
    """the physical directions under a pulse map and the further E_t images of the exact mode are counted"""
    force(monkeypatch, "1")
    c = make_case(4401, 4, 4, 50, 3, hermitian=False)
    rng = np.random.default_rng(9903)
    O, K, N = cplx(rng, 2, 4, 4), c["K"], c["N"]
    with engine(qoc, c) as eng:
        eng.set_bounds(np.array([-0.8, -0.5]), np.array([0.9, 0.6]))
        u, udots = 0.5 * rng.standard_normal((K, N)), rng.standard_normal((5, K, N))
        multi_dev(torch, eng, u, udots[:1], O)
        one = eng.info["workspace_bytes"]
        multi_dev(torch, eng, u, udots, O)
        five = eng.info["workspace_bytes"]
        assert five - one == 4 * K * N * 8, (one, five)
        eng.set_trajectory_derivative("exact")
        multi_dev(torch, eng, u, udots[:1], O)
        e1 = eng.info["workspace_bytes"]
        multi_dev(torch, eng, u, udots, O)
        e5 = eng.info["workspace_bytes"]
        info = eng.info
        chunks = 64 * info["waves_per_member"] // (2 if info["lane_pair"] else 1)
        image = c["E"] * info["slices_per_lane"] * chunks * 16 * 16
        assert e5 - e1 == image, (e1, e5, image)              # <4,4>: blocks of two directions, one further image


# ---- 9: sequences ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_eval_multi_eval_and_the_kernel_names(qoc, monkeypatch, mode):
    c, O, _, _ = invariant_case()
    xdots = np.random.default_rng(9904).standard_normal((5, c["K"], c["N"]))
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative(mode)
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        force(monkeypatch, "1")
        on = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        names_on = eng.kernel_names()
        F1, G1 = eng.eval(c["x"])
        assert eng.kernel_names() == names0
        force(monkeypatch, "0")
        off = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        names_off = eng.kernel_names()
        F2, G2 = eng.eval(c["x"])
        again = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
    assert F1 == F0 and F2 == F0 and np.array_equal(G1, G0) and np.array_equal(G2, G0)
    assert MULTI[mode] in names_on and SINGLE[mode] not in names_on, names_on
    assert names_off.count(SINGLE[mode]) == 5 and MULTI[mode] not in names_off, names_off
    assert sum(k.startswith("sweep_") for k in names_off) == sum(k.startswith("sweep_") for k in names0)        # ONE sweep
    assert not any("jvp" in k for k in names0)
    same_bits(on, off, "forced on = forced off")
    same_bits(again, off, "call to call")


def test_default_dispatch_leaves_a_lone_direction_to_the_single_kernel(qoc, monkeypatch):
    """<3,3> carries four directions per launch: by default five are one multi launch and one single launch, one direction
    alone is the single kernel (where the multi kernel measured slower); forced on, every block is the multi kernel's"""
    c, O, _, _ = invariant_case()
    xdots = np.random.default_rng(9908).standard_normal((5, c["K"], c["N"]))
    with engine(qoc, c) as eng:
        want = singles(eng, c["x"], xdots, O)
        force(monkeypatch, None)
        five = eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        names5 = eng.kernel_names()
        eng.observe_jvp_multi(c["x"], xdots[:1], O, final=True)
        names1 = eng.kernel_names()
        force(monkeypatch, "1")
        eng.observe_jvp_multi(c["x"], xdots, O, final=True)
        forced = eng.kernel_names()
    same_bits(five, want, "default dispatch")
    assert names5.count(MULTI["first_order"]) == 1 and names5.count(SINGLE["first_order"]) == 1, names5
    assert names1.count(SINGLE["first_order"]) == 1 and MULTI["first_order"] not in names1, names1
    assert forced.count(MULTI["first_order"]) == 2 and SINGLE["first_order"] not in forced, forced


# ---- 10: arguments and refusals ----------------------------------------------------------------------------------------------------
def raw_call(qoc, eng, x, n_dir, xdot, n_obs, per_member, O, ydot, Xdot):
    lib = qoc.load_library()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.grape_eval_jvp_multi(eng._h, ptr(x), n_dir, ptr(xdot), n_obs, per_member, ptr(O), ptr(ydot), ptr(Xdot))
    return rc, lib.grape_last_error(eng._h).decode()


def test_invalid_arguments(qoc):
    c = make_case(4601, 4, 4, 20, 2)
    E, N, K = c["E"], c["N"], c["K"]
    rng = np.random.default_rng(9905)
    O = cplx(rng, 2, 4, 4)
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])

        def evaluates_as_before():
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)

        xf = np.ascontiguousarray(c["x"].T)
        xdf = np.ascontiguousarray(rng.standard_normal((3, N, K)))
        Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
        yd, Xd = np.empty((3, E, 2, N + 1), complex), np.empty((3, E, 4, 4), complex)
        for n_dir in (0, 9, -1):
            rc, msg = raw_call(qoc, eng, xf, n_dir, xdf, 2, 0, Of, yd, Xd)
            assert rc == -1 and "grape_eval_jvp_multi" in msg and f"n_dir = {n_dir}" in msg, (rc, msg)
            evaluates_as_before()
        bad_args = [
            (None, 3, xdf, 2, 0, Of, yd, Xd),                 # null x
            (xf, 3, None, 2, 0, Of, yd, Xd),                  # null xdot
            (xf, 3, xdf, 2, 0, Of, None, None),               # ydot and Xdot_final both NULL
            (xf, 3, xdf, -1, 0, Of, yd, Xd), (xf, 3, xdf, 17, 0, Of, yd, Xd),
            (xf, 3, xdf, 0, 0, Of, yd, Xd),                   # n_obs = 0 with a non-NULL ydot
            (xf, 3, xdf, 2, 0, None, yd, Xd),                 # n_obs > 0 with a NULL O
            (xf, 3, xdf, 2, 2, Of, yd, Xd), (xf, 3, xdf, 2, -1, Of, yd, Xd),
        ]
        for args in bad_args:
            rc, msg = raw_call(qoc, eng, *args)
            assert rc == -1 and "grape_eval_jvp_multi" in msg, (rc, msg)
            evaluates_as_before()
        bad = xdf.copy()
        bad[1].reshape(-1)[7] = np.inf                        # a non-finite entry in direction 2 of 3
        rc, msg = raw_call(qoc, eng, xf, 3, bad, 2, 0, Of, yd, Xd)
        assert rc == -1 and "not finite" in msg and "xdot[" in msg, (rc, msg)
        bad_O = Of.copy()
        bad_O.reshape(-1)[5] = np.nan
        rc, msg = raw_call(qoc, eng, xf, 3, xdf, 2, 0, bad_O, yd, Xd)
        assert rc == -1 and "not finite" in msg and "O[" in msg, (rc, msg)
        evaluates_as_before()
        rc, msg = raw_call(qoc, eng, xf, 3, xdf, 0, 0, None, None, Xd)           # valid corners
        assert rc == 0, msg
        rc, msg = raw_call(qoc, eng, xf, 3, xdf, 2, 0, Of, yd, None)
        assert rc == 0, msg
        for call in (lambda: eng.observe_jvp_multi(c["x"], xdf[0].T, O), lambda: eng.observe_jvp_multi(c["x"], xdf[:, :5], O),
                     lambda: eng.observe_jvp_multi(c["x"], np.swapaxes(xdf, 1, 2), None),
                     lambda: eng.observe_jvp_multi(c["x"], np.zeros((0, K, N)), O)):
            with pytest.raises(ValueError):
                call()
        evaluates_as_before()
    lib = qoc.load_library()                                  # before grape_set_operators
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.grape_eval_jvp_multi(h, p(xf), 3, p(xdf), 2, 0, p(Of), p(yd), None) == -5
        assert b"operators not set" in lib.grape_last_error(h)
        assert lib.grape_eval_jvp_multi_device(h, None, 3, p(xdf), 2, 0, p(Of), p(yd), None, None) == -5
    finally:
        lib.grape_destroy(h)
    assert lib.grape_eval_jvp_multi(None, None, 1, None, 0, 0, None, None, None) == -1
    assert lib.grape_eval_jvp_multi_device(None, None, 1, None, 0, 0, None, None, None, None) == -1


def test_refusals(qoc):
    c = make_case(4501, 4, 4, 20, 2)
    GE = qoc.GrapeError

    def refused(eng, case, word):
        F0, G0 = eng.eval(case["x"])                          # the bits from before the refusal
        with pytest.raises(GE) as ei:
            eng.observe_jvp_multi(case["x"], np.ones((2,) + case["x"].shape), None, final=True)
        assert ei.value.status == -2 and word in str(ei.value) and "grape_eval_jvp_multi" in str(ei.value), str(ei.value)
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


# ---- 11: the Jacobian --------------------------------------------------------------------------------------------------------------
def test_trajectory_jacobian_against_central_differences(qoc, torch):
    """(n, m, N, E) = (2, 2, 6, 2) in the exact mode against central differences of observe with h = 1e-5, to 1e-6 of the
    largest entry (the bar of test_gpu_rc_exact.py for the same kind of comparison); 12 columns: a block of 8 and one of 4"""
    c = make_case(9906, 2, 2, 6, 2, hermitian=False)
    O = cplx(np.random.default_rng(9907), 3, 2, 2)
    h = 1e-5
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative("exact")
        J = eng.trajectory_jacobian(c["x"], O)
        some = eng.trajectory_jacobian(c["x"], O, columns=[11, 2])
        fd = np.empty_like(J)
        for i in range(c["x"].size):
            e = np.zeros(c["x"].size)
            e[i] = h
            e = e.reshape(c["x"].shape)
            fd[i] = (eng.observe(c["x"] + e, O) - eng.observe(c["x"] - e, O)) / (2 * h)
    assert J.shape == (12, 2, 3, 7) and np.array_equal(some, J[[11, 2]])
    err, scale = np.abs(J - fd).max(), np.abs(fd).max()
    print(f"trajectory_jacobian against central differences: |J - fd|_inf = {err:.3e}, |fd|_inf = {scale:.3e}")
    assert scale > 0 and err <= 1e-6 * scale
