"""The ensemble-averaged trajectory calls on the GPU (grape_eval_observables_mean / _vjp_mean / _jvp_mean): the member reduction
against the math.fsum reference of the per-member read-out of the same context, within the a-priori bound of ANY summation
order (tests/traj_mean_reference.py: E 2^-52 sum_k |v_k| |component_k| per component -- derived, not measured); the bit
identities the fixed tree promises; the pull-back bit for bit against grape_eval_vjp on the explicit broadcast cotangents;
the push-forward; torch.autograd; refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import rc_reference as rcr  # noqa: E402
import traj_mean_reference as tm  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402
from test_gpu_observe import engine as engine_of_type, sandwich_case  # noqa: E402
from test_gpu_running_cost import _chunk_budget, engine  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5


def cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def mean_case(seed, n, m, N, E, hermitian=True, K=2):
    """operators of norm ~1, Xi = m columns of a unitary, a target of the same kind (no propagation on the CPU: E goes to 257)"""
    rng = np.random.default_rng(seed)
    A, B, Xi, wts = rcr.random_problem(rng, n, m, K, E, hermitian=hermitian)
    Q = np.linalg.qr(cplx(rng, n, n))[0]
    Xt = np.array([Q[:, :m] for _ in range(E)])
    return dict(n=n, m=m, N=N, E=E, K=K, A=A, B=B, Xi=Xi, Xt=Xt, wts=wts, x=rng.standard_normal((K, N)), variant=0, T=T)


def check_fsum(got, v, members, what):
    """got against the fsum of v_k members[k], every component within E 2^-52 sum_k |v_k| |component_k|"""
    ref, mag = tm.fsum_mean(v, members)
    tol = tm.fsum_tolerance(len(v), mag)
    d = got - ref
    worst = max(np.max(np.abs(d.real) / np.maximum(tol.real, 1e-300)), np.max(np.abs(d.imag) / np.maximum(tol.imag, 1e-300)))
    print(f"{what}: worst |got - fsum| / tolerance = {worst:.3f}")
    assert got.shape == ref.shape and tm.within(got, ref, tol), f"{what}: {worst:.3f} of the tolerance"


# ---- 1: value ----------------------------------------------------------------------------------------------------------------
# N + 1 = 6 and 68: below and above one wave, no multiple of 64.  E: one member, no power of two, more than one wave of
# members, more than one reduction segment (17 of them at 257, the last one ragged)
VALUE = [(n, m, N, E) for n in (2, 3, 4) for m in sorted({1, n}) for N in (5, 67) for E in (1, 3, 70, 257)]


@pytest.mark.parametrize("n,m,N,E", VALUE)
def test_value_against_the_fsum_of_the_per_member_read_out(qoc, n, m, N, E):
    c = mean_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=bool((n + E) % 2))
    rng = np.random.default_rng(11000 + 100 * n + 10 * m + N + E)
    v = rng.standard_normal(E)
    with engine(qoc, c) as eng:
        F0 = eng.eval(c["x"])[0]
        for n_obs in (1, 3, 16):
            per_member = n_obs == 3
            O = cplx(rng, E, n_obs, n, m) if per_member else cplx(rng, n_obs, n, m)
            y, Xf = eng.observe(c["x"], O, per_member=per_member, final=True)
            ym, Xm, F = eng.observe_mean(c["x"], O, v=v, per_member=per_member, final=True, want_F=True)
            names = eng.kernel_names()
            assert ym.shape == (n_obs, N + 1) and Xm.shape == (n, m)
            assert F == F0
            assert "traj_mean_reduce_kernel" in names and ("traj_mean_combine_kernel" in names) == (E > 16)
            what = f"n={n} m={m} N={N} E={E} n_obs={n_obs} per_member={per_member}"
            check_fsum(ym, v, y, what + " y_mean")
            check_fsum(Xm, v, Xf, what + " X_mean")
        # each output alone: the same bits
        y_only = eng.observe_mean(c["x"], O, v=v)
        X_only = eng.observe_mean(c["x"], None, v=v, final=True)[1]
        assert np.array_equal(y_only, ym) and np.array_equal(X_only, Xm)


@pytest.mark.parametrize("sys_type,xi_kind,n,N,E", [("StateTransfer", "density", 3, 67, 70), ("CoherenceTransfer", "general", 4, 5, 3)])
def test_value_on_the_sandwich_types(qoc, sys_type, xi_kind, n, N, E):
    c = sandwich_case(11500 + n, n, N, E, True, xi_kind)
    rng = np.random.default_rng(11501 + n)
    v, O = rng.standard_normal(E), cplx(rng, 3, n, n)
    with engine_of_type(qoc, c, sys_type) as eng:
        F0 = eng.eval(c["x"])[0]
        y, Xf = eng.observe(c["x"], O, final=True)
        ym, Xm, F = eng.observe_mean(c["x"], O, v=v, final=True, want_F=True)
    assert F == F0
    check_fsum(ym, v, y, f"{sys_type} y_mean")
    check_fsum(Xm, v, Xf, f"{sys_type} X_mean")


def test_value_against_the_numpy_reference(qoc):
    """one case against tests/observe_reference.py (expm per slice, states by a loop), at the project's parity bar"""
    c = mean_case(11601, 3, 3, 67, 70, hermitian=False)
    rng = np.random.default_rng(11602)
    O = cplx(rng, 3, 3, 3)
    O[0] = c["Xi"][0]                                         # (|y_0| of order 1)
    with engine(qoc, c) as eng:
        ym, Xm = eng.observe_mean(c["x"], O, final=True)      # the ensemble weights
    ym_ref, Xm_ref = tm.observables_mean_ref("UnitaryGate", c["A"], c["B"], c["Xi"], c["x"], c["T"], O, c["wts"])
    assert np.abs(ym_ref).max() >= 0.1
    assert np.abs(ym - ym_ref).max() <= PARITY_RTOL * np.abs(ym_ref).max()
    assert np.abs(Xm - Xm_ref).max() <= PARITY_RTOL * np.abs(Xm_ref).max()


# ---- 2: weights --------------------------------------------------------------------------------------------------------------
def test_weights(qoc):
    c = mean_case(12001, 4, 4, 67, 70)
    rng = np.random.default_rng(12002)
    O = cplx(rng, 3, 4, 4)
    with engine(qoc, c) as eng:
        y, Xf = eng.observe(c["x"], O, final=True)
        a = eng.observe_mean(c["x"], O, final=True)
        b = eng.observe_mean(c["x"], O, v=c["wts"], final=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])       # v = None is v = wts, bit for bit
        eng.set_risk(3.0)                                     # the risk does not enter
        r = eng.observe_mean(c["x"], O, final=True)
        eng.set_risk(0.0)
        assert np.array_equal(r[0], a[0]) and np.array_equal(r[1], a[1])
        v = rng.standard_normal(70)
        v[::3] = 0.0
        v[1::3] = -np.abs(v[1::3])
        ym, Xm = eng.observe_mean(c["x"], O, v=v, final=True)
        check_fsum(ym, v, y, "zero and negative weights y_mean")
        check_fsum(Xm, v, Xf, "zero and negative weights X_mean")
        zero = eng.observe_mean(c["x"], O, v=np.zeros(70))
        assert not zero.any()
    c1 = mean_case(12003, 3, 1, 67, 1)
    with engine(qoc, c1) as eng:
        y, Xf = eng.observe(c1["x"], O[:, :3, :1], final=True)
        ym, Xm = eng.observe_mean(c1["x"], O[:, :3, :1], v=[1.0], final=True)
    assert np.array_equal(ym, y[0]) and np.array_equal(Xm, Xf[0])             # one member, weight 1: the member, bit for bit


# ---- 3: order ----------------------------------------------------------------------------------------------------------------
def test_repeated_calls_and_probe_columns_give_equal_bits(qoc):
    c = mean_case(13001, 2, 2, 67, 257, hermitian=False)
    rng = np.random.default_rng(13002)
    O, v = cplx(rng, 16, 2, 2), rng.standard_normal(257)
    with engine(qoc, c) as eng:
        ym = eng.observe_mean(c["x"], O, v=v)
        assert np.array_equal(eng.observe_mean(c["x"], O, v=v), ym)
        for j in range(16):                                   # column j of the 16-probe call = the 1-probe call with probe j
            assert np.array_equal(eng.observe_mean(c["x"], O[j], v=v)[0], ym[j]), j
        xdot = rng.standard_normal(c["x"].shape)
        yd = eng.observe_jvp_mean(c["x"], xdot, O, v=v)
        assert np.array_equal(eng.observe_jvp_mean(c["x"], xdot, O, v=v), yd)
        assert np.array_equal(eng.observe_jvp_mean(c["x"], xdot, O[5], v=v)[0], yd[5])


@pytest.mark.parametrize("hermitian", [True, False])
def test_member_chunked_context_is_bitwise_the_unchunked_one(qoc, monkeypatch, hermitian):
    c = mean_case(13101 + hermitian, 3, 3, 40, 7, hermitian=hermitian)
    rng = np.random.default_rng(13102)
    O, v, xdot = cplx(rng, 7, 3, 3, 3), rng.standard_normal(7), rng.standard_normal((2, 40))
    with engine(qoc, c) as eng:
        ref = eng.observe_mean(c["x"], O, v=v, per_member=True, final=True, want_F=True)
        refd = eng.observe_jvp_mean(c["x"], xdot, O, v=v, per_member=True, final=True)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, hermitian, 4)))
    with engine(qoc, c) as eng:
        assert eng.info["member_chunk"] == 4                  # a block of 4 and a ragged last one of 3
        got = eng.observe_mean(c["x"], O, v=v, per_member=True, final=True, want_F=True)
        names = eng.kernel_names()
        assert names.count("observe_kernel") == 2 and names.count("traj_mean_reduce_kernel") == 1      # once, behind the last block
        gotd = eng.observe_jvp_mean(c["x"], xdot, O, v=v, per_member=True, final=True)
        assert eng.kernel_names().count("traj_mean_reduce_kernel") == 1
    assert got[2] == ref[2] and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(gotd[0], refd[0]) and np.array_equal(gotd[1], refd[1])


# ---- 4: the pull-back, bit for bit the per-member call on the explicit cotangents -----------------------------------------------
def explicit(v, cot):
    """(E, ...) with .real = v_k Re cot, .imag = v_k Im cot, component-wise"""
    if cot is None:
        return None
    out = np.empty((len(v),) + cot.shape, complex)
    w = v.reshape((len(v),) + (1,) * cot.ndim)
    out.real = w * cot.real
    out.imag = w * cot.imag
    return out


@pytest.mark.parametrize("setting", ["first_order", "exact", "basis", "bounds", "basis+bounds+exact", "chunked"])
def test_pull_back_is_bitwise_the_per_member_call(qoc, monkeypatch, setting):
    E, N = (7, 40) if setting == "chunked" else (70, 67)
    c = mean_case(14001 + len(setting), 3, 3, N, E, hermitian=(setting != "chunked"))
    rng = np.random.default_rng(14002)
    O_sh, O_mem = cplx(rng, 3, 3, 3), cplx(rng, E, 3, 3, 3)
    ybar, xbar, v = cplx(rng, 3, N + 1), cplx(rng, 3, 3), rng.standard_normal(E)
    v[2] = 0.0
    if setting == "chunked":
        with engine(qoc, c) as eng:
            info = eng.info
        monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, False, 4)))
    with engine(qoc, c) as eng:
        x = c["x"]
        if setting == "chunked":
            assert eng.info["member_chunk"] == 4              # a block of 4 and a ragged last one of 3
        if "exact" in setting:
            eng.set_trajectory_derivative("exact")
        if "basis" in setting:
            M = 9
            eng.set_basis(np.cos(np.outer(np.arange(N) + 0.5, np.arange(M)) * np.pi / N), x0=0.1 * c["x"])
            x = 0.3 * rng.standard_normal((2, M))
        if "bounds" in setting:
            eng.set_bounds([-1.0, -np.inf], [1.5, np.inf])
        for per_member in (False, True):
            O = O_mem if per_member else O_sh
            for yb, xb in ((ybar, None), (None, xbar), (ybar, xbar)):
                for vv in (v, None):
                    w = c["wts"] if vv is None else vv
                    G = eng.observe_vjp_mean(x, O, ybar_mean=yb, xbar_mean=xb, v=vv, per_member=per_member)
                    names = eng.kernel_names()
                    G_ref = eng.observe_vjp(x, O, ybar=explicit(w, yb), xbar_final=explicit(w, xb), per_member=per_member)
                    assert G.shape == x.shape and G_ref.any()
                    assert np.array_equal(G, G_ref), (setting, per_member, yb is None, xb is None, vv is None)
                    assert names.count("traj_mean_broadcast_kernel") == 1 and names.index("traj_mean_broadcast_kernel") < names.index("vjp_sum_kernel")


# ---- 5: the push-forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,N,E,herm", [(4, 4, 67, 70, True), (3, 1, 5, 3, False), (2, 2, 67, 257, True)])
def test_push_forward(qoc, n, m, N, E, herm):
    c = mean_case(15001 + 10 * n + m, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(15002 + n)
    O, xdot, v = cplx(rng, 3, n, m), rng.standard_normal((2, N)), rng.standard_normal(E)
    ybar, xbar = cplx(rng, 3, N + 1), cplx(rng, n, m)
    with engine(qoc, c) as eng:
        yd, Xd = eng.observe_jvp(c["x"], xdot, O, final=True)
        ydm, Xdm = eng.observe_jvp_mean(c["x"], xdot, O, v=v, final=True)
        names = eng.kernel_names()
        y2, X2 = eng.observe_jvp_mean(c["x"], 2.0 * xdot, O, v=v, final=True)
        yn, Xn = eng.observe_jvp_mean(c["x"], -xdot, O, v=v, final=True)
        y0, X0 = eng.observe_jvp_mean(c["x"], 0.0 * xdot, O, v=v, final=True)
        G = eng.observe_vjp_mean(c["x"], O, ybar_mean=ybar, xbar_mean=xbar, v=v)
    assert "trajectory_jvp_kernel" in names and "traj_mean_reduce_kernel" in names
    check_fsum(ydm, v, yd, f"n={n} m={m} N={N} E={E} ydot_mean")
    check_fsum(Xdm, v, Xd, f"n={n} m={m} N={N} E={E} Xdot_mean")
    # exactly linear in xdot
    assert np.array_equal(y2, 2.0 * ydm) and np.array_equal(X2, 2.0 * Xdm)
    assert np.array_equal(yn, -ydm) and np.array_equal(Xn, -Xdm)
    assert not y0.any() and not X0.any()
    # the transpose pair, to the relative size tests/test_gpu_jvp.py asks of the unaveraged pair
    lhs, mag = jr.pairing(ybar, ydm, xbar, Xdm)
    rhs, scale = float(np.sum(G * xdot)), float(np.sum(np.abs(G * xdot))) + mag
    print(f"n={n} m={m} N={N} E={E}: lhs={lhs:.15e} rhs={rhs:.15e} |lhs - rhs| / scale = {abs(lhs - rhs) / scale:.2e}")
    assert abs(lhs) > 0 and abs(lhs - rhs) <= PARITY_RTOL * scale


# ---- 6: torch.autograd ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def test_gradcheck_passes_in_exact_mode(qoc, torch):
    from quoptimalcontrol_jl_amd import autograd
    c = mean_case(16001, 2, 2, 6, 3)
    rng = np.random.default_rng(16002)
    O, v = cplx(rng, 2, 2, 2), rng.standard_normal(3)
    with engine(qoc, c) as eng:
        eng.set_trajectory_derivative("exact")
        x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
        assert torch.autograd.gradcheck(lambda xx: autograd.trajectory_mean(eng, xx, O, v=v), (x,))
        assert torch.autograd.gradcheck(lambda xx: autograd.trajectory_mean(eng, xx, O, final=False), (x,))


def test_autograd_backward_and_forward_ad(qoc, torch):
    import torch.autograd.forward_ad as fwad
    from quoptimalcontrol_jl_amd import autograd
    c = mean_case(16101, 3, 3, 21, 5)
    rng = np.random.default_rng(16102)
    O, v, xdot = cplx(rng, 2, 3, 3), rng.uniform(0.1, 0.3, 5), rng.standard_normal((2, 21))
    with engine(qoc, c) as eng:
        x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
        ym, Xm = autograd.trajectory_mean(eng, x, O, v=v)
        assert tuple(ym.shape) == (2, 22) and tuple(Xm.shape) == (3, 3)
        loss = -torch.log(1e3 - ym[0].abs() ** 2).sum() + (Xm.abs() ** 2).sum()
        loss.backward()
        # the same loss through the per-member function and a torch sum: the gradient to rounding
        x2 = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
        y, Xf = autograd.trajectory(eng, x2, O)
        vt = torch.tensor(v)
        ym2, Xm2 = torch.einsum("k,kjs->js", vt.to(y.dtype), y), torch.einsum("k,kab->ab", vt.to(Xf.dtype), Xf)
        loss2 = -torch.log(1e3 - ym2[0].abs() ** 2).sum() + (Xm2.abs() ** 2).sum()
        loss2.backward()
        assert abs(loss.item() - loss2.item()) <= 1e-12 * abs(loss2.item())
        gmax = x2.grad.abs().max().item()
        assert gmax > 0 and (x.grad - x2.grad).abs().max().item() <= 1e-12 * gmax
        # forward mode: the dual's tangent is observe_jvp_mean's output
        with fwad.dual_level():
            xd = fwad.make_dual(torch.tensor(c["x"], dtype=torch.float64), torch.tensor(xdot))
            yd, Xd = autograd.trajectory_mean(eng, xd, O, v=v)
            ty, tX = fwad.unpack_dual(yd).tangent, fwad.unpack_dual(Xd).tangent
        ydm, Xdm = eng.observe_jvp_mean(c["x"], xdot, O, v=v, final=True)
        assert np.array_equal(ty.numpy(), ydm) and np.array_equal(tX.numpy(), Xdm)


def test_expectation_values_mean(qoc):
    from test_gpu_running_cost import as_problem, make_case
    c = make_case(16201, 2, 2, 30, 3)
    prob = as_problem(qoc, c)
    O = np.array([[[1.0, 0.0], [0.0, 0.0]]], complex)
    times, y = qoc.api.expectation_values(prob, c["x"], O)
    times_m, ym = qoc.api.expectation_values(prob, c["x"], O, mean=True)
    assert np.array_equal(times, times_m) and y.shape == (3, 1, 31) and ym.shape == (1, 31)
    check_fsum(ym, c["wts"], y, "expectation_values(mean=True)")


# ---- 7: refusals and arguments -----------------------------------------------------------------------------------------------
def three_calls(eng, case, O):
    x = case["x"]
    n, m, N = eng.n, eng.m, eng.N
    return [("grape_eval_observables_mean", lambda: eng.observe_mean(x, O)),
            ("grape_eval_vjp_mean", lambda: eng.observe_vjp_mean(x, O, ybar_mean=np.ones((O.shape[0], N + 1), complex))),
            ("grape_eval_jvp_mean", lambda: eng.observe_jvp_mean(x, np.ones_like(x), O))]


def refused(qoc, eng, case, word, only=None):
    O = np.ones((1, eng.n, eng.m), complex)
    F0, G0 = eng.eval(case["x"])                              # the bits from before the refusal
    for name, call in three_calls(eng, case, O):
        if only and name not in only:
            continue
        with pytest.raises(qoc.GrapeError) as ei:
            call()
        assert ei.value.status == -2 and word in str(ei.value) and name + ":" in str(ei.value), str(ei.value)
        F, G = eng.eval(case["x"])
        assert F == F0 and np.array_equal(G, G0)


def test_refusals_of_the_underlying_calls_carry_the_new_names(qoc):
    c = mean_case(17001, 4, 4, 20, 2)
    for nbad in (5, 1):
        big = mean_case(17002 + nbad, nbad, nbad, 8, 1)
        with engine(qoc, big) as eng:
            refused(qoc, eng, big, "dimension")
    s = sandwich_case(17010, 3, 9, 2, True, "density")
    with engine_of_type(qoc, s, "StateTransfer") as eng:
        refused(qoc, eng, s, "StateTransfer", only=("grape_eval_vjp_mean", "grape_eval_jvp_mean"))
        assert eng.observe_mean(s["x"], np.ones((1, 3, 3), complex)).shape == (1, 10)      # the read-out serves the sandwich
    with engine(qoc, c, gradient="exact") as eng:
        refused(qoc, eng, c, "exact")
    with engine(qoc, c, gradient="exact", objective="c1") as eng:
        refused(qoc, eng, c, "c1", only=("grape_eval_observables_mean",))
        refused(qoc, eng, c, "exact", only=("grape_eval_vjp_mean", "grape_eval_jvp_mean"))       # (as their underlying calls say)
    with engine(qoc, c, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM) as eng:
        refused(qoc, eng, c, "multi-device")
    with engine(qoc, c, force_collective=True) as eng:
        refused(qoc, eng, c, "communicator")


def test_arguments(qoc):
    c = mean_case(17101, 4, 4, 20, 2)
    rng = np.random.default_rng(17102)
    O = cplx(rng, 2, 4, 4)
    lib = qoc.load_library()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        xf = np.ascontiguousarray(c["x"].T)
        Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
        v = np.array([0.25, 0.75])
        ym, Xm, yb, G = np.empty((2, 21), complex), np.empty((4, 4), complex), np.ones((2, 21), complex), np.empty((20, 2))

        def same_bits():
            F, Gn = eng.eval(c["x"])
            assert F == F0 and np.array_equal(Gn, G0)

        obs = lambda *a: lib.grape_eval_observables_mean(eng._h, *a)
        vjp = lambda *a: lib.grape_eval_vjp_mean(eng._h, *a)
        jvp = lambda *a: lib.grape_eval_jvp_mean(eng._h, *a)
        bad = [
            (obs, "grape_eval_observables_mean", (ptr(xf), 2, 0, ptr(Of), ptr(v), None, None, None), "both null"),
            (obs, "grape_eval_observables_mean", (ptr(xf), 17, 0, ptr(Of), ptr(v), ptr(ym), ptr(Xm), None), "n_obs"),
            (obs, "grape_eval_observables_mean", (ptr(xf), 0, 0, ptr(Of), ptr(v), ptr(ym), ptr(Xm), None), "n_obs = 0"),
            (obs, "grape_eval_observables_mean", (None, 2, 0, ptr(Of), ptr(v), ptr(ym), ptr(Xm), None), "x is null"),
            (vjp, "grape_eval_vjp_mean", (ptr(xf), 2, 0, ptr(Of), ptr(v), None, None, ptr(G)), "both null"),
            (vjp, "grape_eval_vjp_mean", (ptr(xf), 17, 0, ptr(Of), ptr(v), ptr(yb), None, ptr(G)), "n_obs"),
            (vjp, "grape_eval_vjp_mean", (ptr(xf), 2, 0, ptr(Of), ptr(v), ptr(yb), None, None), "G is null"),
            (jvp, "grape_eval_jvp_mean", (ptr(xf), ptr(xf), 2, 0, ptr(Of), ptr(v), None, None), "both null"),
            (jvp, "grape_eval_jvp_mean", (ptr(xf), ptr(xf), 17, 0, ptr(Of), ptr(v), ptr(ym), ptr(Xm)), "n_obs"),
            (jvp, "grape_eval_jvp_mean", (ptr(xf), None, 2, 0, ptr(Of), ptr(v), ptr(ym), ptr(Xm)), "xdot is null"),
        ]
        for fn, name, args, words in bad:
            rc = fn(*args)
            msg = lib.grape_last_error(eng._h).decode()
            assert rc == -1 and name + ":" in msg and words in msg, (rc, msg)
            same_bits()
        # a NaN among the weights
        vn = np.array([0.25, np.nan])
        for fn, args in ((obs, (ptr(xf), 2, 0, ptr(Of), ptr(vn), ptr(ym), ptr(Xm), None)),
                         (vjp, (ptr(xf), 2, 0, ptr(Of), ptr(vn), ptr(yb), None, ptr(G))),
                         (jvp, (ptr(xf), ptr(xf), 2, 0, ptr(Of), ptr(vn), ptr(ym), ptr(Xm)))):
            assert fn(*args) == -1
            msg = lib.grape_last_error(eng._h).decode()
            assert "not finite" in msg and "v[1]" in msg, msg
            same_bits()
        with pytest.raises(qoc.GrapeError) as ei:
            eng.observe_vjp_mean(c["x"], O, ybar_mean=np.where(np.arange(42).reshape(2, 21) == 5, np.inf, 1.0 + 0j))
        assert ei.value.status == -1 and "not finite" in str(ei.value)
        with pytest.raises(qoc.GrapeError) as ei:                # finite factors, an overflowing product
            eng.observe_vjp_mean(c["x"], O, ybar_mean=np.full((2, 21), 1e200 + 0j), v=[1e200, 1.0])
        assert ei.value.status == -1 and "not finite" in str(ei.value)
        same_bits()
        # the Python layer catches wrong shapes before the library is called
        for call in (lambda: eng.observe_mean(c["x"], O, v=np.ones(3)), lambda: eng.observe_mean(c["x"], None),
                     lambda: eng.observe_mean(c["x"], np.zeros((17, 4, 4))),
                     lambda: eng.observe_vjp_mean(c["x"], O, ybar_mean=np.ones((2, 2, 21))),
                     lambda: eng.observe_vjp_mean(c["x"], O), lambda: eng.observe_vjp_mean(c["x"], None, ybar_mean=np.ones((2, 21))),
                     lambda: eng.observe_vjp_mean(c["x"], O, xbar_mean=np.ones((2, 4, 4))),
                     lambda: eng.observe_jvp_mean(c["x"], c["x"][:, :5], O), lambda: eng.observe_jvp_mean(c["x"], c["x"], None)):
            with pytest.raises(ValueError):
                call()
        same_bits()


def test_eval_mean_eval_keeps_the_bits_and_the_kernel_names(qoc):
    c = mean_case(17201, 4, 4, 67, 70)
    rng = np.random.default_rng(17202)
    O = cplx(rng, 3, 4, 4)
    new = ("traj_mean_reduce_kernel", "traj_mean_combine_kernel", "traj_mean_broadcast_kernel")
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        base = eng.kernel_names()
        eng.observe(c["x"], O)
        plain = eng.kernel_names()
        assert not any(k in plain for k in new) and not any(k in base for k in new)
        eng.observe_mean(c["x"], O, final=True)
        names = eng.kernel_names()
        assert "traj_mean_reduce_kernel" in names and "traj_mean_combine_kernel" in names
        assert [k for k in names if not k.startswith("traj_mean_")] == plain                  # and nothing else moved
        F1, G1 = eng.eval(c["x"])
        assert F1 == F0 and np.array_equal(G1, G0) and eng.kernel_names() == base
        eng.observe_vjp_mean(c["x"], O, ybar_mean=np.ones((3, 68), complex))
        assert "traj_mean_broadcast_kernel" in eng.kernel_names()
        eng.observe_jvp_mean(c["x"], np.ones_like(c["x"]), O)
        assert "traj_mean_reduce_kernel" in eng.kernel_names()
        F2, G2 = eng.eval(c["x"])
        assert F2 == F0 and np.array_equal(G2, G0) and eng.kernel_names() == base
