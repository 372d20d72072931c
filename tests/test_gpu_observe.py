"""grape_eval_observables on the GPU: expectation values along the trajectory and the final states against the NumPy / SciPy
reference of tests/observe_reference.py (expm per slice, states by a loop, traces by einsum) at the project's parity bar,
|y - y_ref|_inf <= 1e-10 |y_ref|_inf over the whole array (every probe set holds O_0 = Xi, so |y_ref|_inf is of order 1),
and against the 50-digit golden fixtures."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import observe_reference as obr  # noqa: E402
import rc_reference as rcr  # noqa: E402
from conftest import PARITY_RTOL, assert_parity  # noqa: E402
from test_gpu_running_cost import SHAPES, _chunk_budget, c5_case, make_case  # noqa: E402
from test_oracle_golden import GOLDEN, load_case  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5


def close(got, want, what="", min_scale=0.1):
    """the parity bar over the whole array"""
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got) - np.asarray(want)).max()
    print(f"{what}: |d|_inf={err:.2e} scale={scale:.2e}")
    assert scale >= min_scale, (what, scale)                  # (the scale is not degenerate)
    assert err <= PARITY_RTOL * scale, f"{what}: {err:.3e} > {PARITY_RTOL * scale:.3e}"


def engine(qoc, c, sys_type="UnitaryGate", **kw):
    return qoc.GrapeEngine(sys_type, c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], c["T"], c["N"], variant=c["variant"], **kw)


def probes(rng, c, n_obs, per_member):
    """O_0 = Xi (|y_0| of order 1), the others random of order 1"""
    E, n, m = c["Xi"].shape
    if per_member:
        O = rng.standard_normal((E, n_obs, n, m)) + 1j * rng.standard_normal((E, n_obs, n, m))
        O[:, 0] = c["Xi"]
    else:
        O = rng.standard_normal((n_obs, n, m)) + 1j * rng.standard_normal((n_obs, n, m))
        O[0] = c["Xi"][0]
    return O


def ref(c, O, per_member, sys_type="UnitaryGate", x=None):
    return obr.observables_ref(sys_type, c["A"], c["B"], c["Xi"], c["x"] if x is None else x, c["T"], O, per_member,
                               c["variant"])


# ---- 1: parity over the shapes that reach every edge of the decomposition -------------------------------------------------
ROWS = [r[:9] for r in SHAPES]                                # (n, m, N, E, hermitian, variant, kernel, S, W)


@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W", ROWS)
def test_parity_over_the_decomposition_edges(qoc, monkeypatch, n, m, N, E, herm, variant, kernel, S, W):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    rng = np.random.default_rng(N + E)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        for n_obs in (1, 3, 16):
            for per_member in (False, True):
                O = probes(rng, c, n_obs, per_member)
                y, Xf = eng.observe(c["x"], O, per_member=per_member, final=True)
                assert "observe_kernel" in eng.kernel_names()
                y2, Xf2 = eng.observe(c["x"], O, per_member=per_member, final=True)
                assert np.array_equal(y, y2) and np.array_equal(Xf, Xf2)        # bitwise reproducible call to call
                y_ref, X_ref = ref(c, O, per_member)
                assert y.shape == (E, n_obs, N + 1) and Xf.shape == (E, n, m)
                what = f"n={n} m={m} N={N} E={E} n_obs={n_obs} per_member={per_member}"
                close(y, y_ref, what + " y")
                close(Xf, X_ref, what + " X_final", min_scale=0.0)


# ---- 2: the sandwich types ---------------------------------------------------------------------------------------------
def sandwich_case(seed, n, N, E, hermitian, xi_kind, variant=0):
    rng = np.random.default_rng(seed)
    A, B, _, wts = rcr.random_problem(rng, n, n, 2, E, hermitian=hermitian)

    def density():
        M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        R = M @ M.conj().T
        return R / np.trace(R).real
    if xi_kind == "density":
        Xi = np.array([density() for _ in range(E)])
    else:                                                     # CoherenceTransfer: any operator
        Xi = rng.standard_normal((E, n, n)) + 1j * rng.standard_normal((E, n, n))
        Xi /= np.linalg.norm(Xi, axis=(1, 2), keepdims=True)
    Xt = np.array([density() for _ in range(E)])
    x = rng.standard_normal((2, N))
    return dict(n=n, m=n, N=N, E=E, K=2, A=A, B=B, Xi=Xi, Xt=Xt, wts=wts, x=x, variant=variant, T=T)


SANDWICH = [  # sys_type, xi_kind, n, N, S, W, kernel, hermitian
    ("StateTransfer", "density", 2, 1, 0, 0, "lane", True),
    ("StateTransfer", "density", 2, 130, 3, 2, "pair", False),
    ("StateTransfer", "density", 3, 7, 3, 1, "lane", False),
    ("StateTransfer", "density", 3, 65, 1, 2, "lane", True),
    ("StateTransfer", "density", 4, 65, 1, 3, "pair", True),
    ("StateTransfer", "density", 4, 130, 2, 3, "lane", False),
    ("CoherenceTransfer", "density", 2, 7, 2, 1, "lane", False),
    ("CoherenceTransfer", "general", 2, 65, 1, 3, "pair", True),
    ("CoherenceTransfer", "general", 3, 130, 1, 3, "lane", False),
    ("CoherenceTransfer", "density", 3, 1, 0, 0, "lane", True),
    ("CoherenceTransfer", "general", 4, 7, 2, 1, "pair", False),
    ("CoherenceTransfer", "general", 4, 130, 3, 2, "lane", True),
    ("CoherenceTransfer", "density", 4, 1, 0, 0, "pair", True),
]


@pytest.mark.parametrize("sys_type,xi_kind,n,N,S,W,kernel,herm", SANDWICH)
def test_sandwich_types(qoc, monkeypatch, sys_type, xi_kind, n, N, S, W, kernel, herm):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    E = 3
    c = sandwich_case(2000 + 10 * n + N, n, N, E, herm, xi_kind, variant=N % 2)
    rng = np.random.default_rng(N)
    # O_0 = Xi / |Xi|^2: y_0 = 1 at s = 0 whatever the purity of Xi
    O = probes(rng, c, 3, True)
    O[:, 0] = c["Xi"] / np.sum(np.abs(c["Xi"]) ** 2, axis=(1, 2), keepdims=True)
    with engine(qoc, c, sys_type, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        y, Xf = eng.observe(c["x"], O, per_member=True, final=True)
        assert "observe_kernel" in eng.kernel_names()
        ys = eng.observe(c["x"], O[0], per_member=False)
    y_ref, X_ref = ref(c, O, True, sys_type)
    what = f"{sys_type} {xi_kind} n={n} N={N}"
    close(y, y_ref, what + " y")
    assert np.abs(X_ref).max() >= 1e-2
    assert np.abs(Xf - X_ref).max() <= PARITY_RTOL * np.abs(X_ref).max()
    close(ys, ref(c, O[0], False, sys_type)[0], what + " shared probes")
    if xi_kind == "density" and herm:                         # the trace of a density operator is conserved
        tr = np.einsum("kaa->k", Xf)
        assert np.abs(tr - 1).max() <= 1e-10


# ---- 3: the golden fixtures ------------------------------------------------------------------------------------------------
SMALL = [p for p in GOLDEN if load_case(p)[0]["n"] <= 4]


@pytest.mark.parametrize("path", SMALL, ids=[os.path.basename(p)[:-5] for p in SMALL])
def test_golden_fixtures(qoc, path):
    c, A, B, Xi, Xt, wts, x, exp, traj = load_case(path)
    n, m, N = c["n"], Xi.shape[2], c["N"]
    want = traj[1]                                            # member0_states (N + 1, n, m)
    with qoc.GrapeEngine(c["sys_type"], A, B, Xi, Xt, wts, c["T"], N, variant=c["variant"]) as eng:
        y, Xf, F = eng.observe(x, obr.matrix_units(n, m), final=True, want_F=True)   # at most 16 probes: y is the whole state
        yt = eng.observe(x, Xt[:, None], per_member=True)
    got = np.moveaxis(y[0], 0, -1).reshape(N + 1, n, m)
    close(got, want, "member 0 states", min_scale=0.0)        # (matrix units: the scale is the fixture's largest state entry)
    assert np.abs(Xf[0] - want[-1]).max() <= PARITY_RTOL * np.abs(want[-1]).max()
    assert_parity(F, np.ones(1), exp["F"], np.ones(1), n, what="F")             # (its F rule; no gradient here)
    Fk = obr.member_fom(c["sys_type"], yt[:, 0, -1], n)
    for k in range(c["E"]):
        tol = PARITY_RTOL * max(abs(exp["member_F"][k]), 1e-3 * n * n)
        assert abs(Fk[k] - exp["member_F"][k]) <= tol, (k, Fk[k], exp["member_F"][k])


# ---- 4: nothing else moves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("composed", [False, True])
def test_nothing_else_moves(qoc, composed):
    c = make_case(3001, 4, 4, 50, 3, J=2, rho_kind="mixed")
    rng = np.random.default_rng(5)
    O = probes(rng, c, 3, False)
    with engine(qoc, c) as eng:
        arg = c["x"]
        if composed:
            eng.set_penalties(np.array([0.3, 0.0]), np.array([0.1, 0.2]))
            eng.set_running_cost(c["R"], c["rho"])
            phi = qoc.fourier_basis(c["N"], c["T"], 2 * np.pi / c["T"] * np.array([0.5, 1.0, 2.0]))
            eng.set_basis(phi, 0.2 * c["x"])
            eng.set_bounds(-1.0, 1.2)
            arg = 0.4 * rng.standard_normal((c["K"], phi.shape[1]))
        F0, G0 = eng.eval(arg)
        names0 = eng.kernel_names()
        y, Xf, F = eng.observe(arg, O, final=True, want_F=True)
        names_obs = eng.kernel_names()
        F1, G1 = eng.eval(arg)
        names1 = eng.kernel_names()
        x_phys = eng.controls(arg) if composed else c["x"]
    assert "observe_kernel" in names_obs and "observe_kernel" not in names0
    assert [k for k in names_obs if k != "observe_kernel"] == names0
    if composed:
        assert "running_cost_kernel" in names0 and names_obs.index("observe_kernel") > names_obs.index("running_cost_fold_kernel")
    assert F == F0 and F1 == F0 and np.array_equal(G1, G0) and names1 == names0
    y_ref, X_ref = ref(c, O, False, x=x_phys)
    close(y, y_ref, f"composed={composed} y")
    close(Xf, X_ref, f"composed={composed} X_final", min_scale=0.0)


# ---- 5: member-chunked equals unchunked, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("hermitian", [True, False])
def test_member_chunked_context_is_bitwise_the_unchunked_one(qoc, monkeypatch, hermitian):
    c = make_case(3101 + hermitian, 3, 3, 40, 10, hermitian=hermitian)
    O = probes(np.random.default_rng(8), c, 3, True)
    with engine(qoc, c) as eng:
        y, Xf, F = eng.observe(c["x"], O, per_member=True, final=True, want_F=True)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, hermitian, 4)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < c["E"], eng.info["member_chunk"]
        yc, Xfc, Fc = eng.observe(c["x"], O, per_member=True, final=True, want_F=True)
        assert eng.kernel_names().count("observe_kernel") >= 2
    assert Fc == F and np.array_equal(yc, y) and np.array_equal(Xfc, Xf)
    close(y, ref(c, O, True)[0], f"hermitian={hermitian}")


# ---- 6: decomposition invariance -----------------------------------------------------------------------------------------
def test_decomposition_invariance(qoc, monkeypatch):
    c = make_case(3201, 4, 4, 130, 2, hermitian=False)
    O = probes(np.random.default_rng(9), c, 3, False)
    res = []
    for kernel in ("lane", "pair"):
        monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
        for S, W in ((0, 0), (3, 2), (2, 3)):
            with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
                res.append(eng.observe(c["x"], O, final=True))
    for y, Xf in res[1:]:
        close(y, res[0][0], "y across decompositions")
        close(Xf, res[0][1], "X_final across decompositions")


# ---- 7: the expm's squaring branch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("n,kernel", [(4, "pair"), (3, "lane")])
def test_propagators_from_the_squaring_branch(qoc, monkeypatch, n, kernel, hermitian):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(3300 + n, n, n, 8, 3, hermitian=hermitian, T=24.0)
    O = probes(np.random.default_rng(10), c, 3, True)
    with engine(qoc, c) as eng:
        y, Xf = eng.observe(c["x"], O, per_member=True, final=True)
    y_ref, X_ref = ref(c, O, True)
    close(y, y_ref, f"T=24 n={n} hermitian={hermitian} y")
    close(Xf, X_ref, f"T=24 n={n} hermitian={hermitian} X_final", min_scale=0.0)


# ---- 8: the debug flow ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,kernel", [(4, 4, "pair"), (3, 2, "lane")])
def test_debug_flow(qoc, monkeypatch, n, m, kernel):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(3400 + n, n, m, 33, 3)
    O = probes(np.random.default_rng(11), c, 3, True)
    with engine(qoc, c, flags=qoc.engine.FLAG_KEEP_COSTATES) as eng:
        assert eng.info["unitary_flow"] == 0
        y = eng.observe(c["x"], O, per_member=True)
        X = np.array([eng.trajectory(k)[1] for k in range(c["E"])])        # (E, N + 1, n, m): the states this call stored
    close(y, np.einsum("kjab,ksab->kjs", O.conj(), X), "traces of the stored trajectory")


# ---- 9: refusals and arguments -------------------------------------------------------------------------------------------
def raw_call(qoc, eng, x, n_obs, per_member, O, y, Xf):
    lib = qoc.load_library()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.grape_eval_observables(eng._h, ptr(x), n_obs, per_member, ptr(O), ptr(y), ptr(Xf), None)
    return rc, lib.grape_last_error(eng._h).decode()


def test_refusals_and_arguments(qoc):
    c = make_case(3501, 4, 4, 20, 2)
    O = probes(np.random.default_rng(12), c, 2, False)
    GE = qoc.GrapeError

    def refused(eng, case, word):
        F0, G0 = eng.eval(case["x"])                          # the bits from before the refusal
        with pytest.raises(GE) as ei:
            eng.observe(case["x"], case["Xi"][0])
        assert ei.value.status == -2 and word in str(ei.value), str(ei.value)
        F, G = eng.eval(case["x"])
        assert F == F0 and np.array_equal(G, G0)

    for nbad in (5, 1):
        big = make_case(3502 + nbad, nbad, nbad, 8, 1)
        with engine(qoc, big) as eng:
            refused(eng, big, "dimension")
    with engine(qoc, c, gradient="exact") as eng:
        refused(eng, c, "exact")
    with engine(qoc, c, gradient="exact", objective="c1") as eng:
        refused(eng, c, "c1")
    with engine(qoc, c, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM) as eng:
        refused(eng, c, "multi-device")
    with engine(qoc, c, force_collective=True) as eng:
        refused(eng, c, "communicator")

    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        xf = np.ascontiguousarray(c["x"].T)
        Of = np.ascontiguousarray(np.swapaxes(O, -1, -2))
        y = np.empty((c["E"], 2, c["N"] + 1), complex)
        Xf = np.empty((c["E"], 4, 4), complex)
        bad_args = [
            (None, 2, 0, Of, y, Xf),                          # null x
            (xf, 2, 0, Of, None, None),                       # y and X_final both NULL
            (xf, -1, 0, Of, y, Xf), (xf, 17, 0, Of, y, Xf),   # n_obs outside 0..16
            (xf, 0, 0, Of, y, Xf),                            # n_obs = 0 with a non-NULL y
            (xf, 2, 0, None, y, Xf),                          # n_obs > 0 with a NULL O
            (xf, 2, 2, Of, y, Xf), (xf, 2, -1, Of, y, Xf),    # per_member other than 0 or 1
        ]
        for args in bad_args:
            rc, msg = raw_call(qoc, eng, *args)
            assert rc == -1 and "grape_eval_observables" in msg, (rc, msg)
            F, G = eng.eval(c["x"])
            assert F == F0 and np.array_equal(G, G0)
        bad = Of.copy()
        bad[1, 2, 3] = np.nan
        rc, msg = raw_call(qoc, eng, xf, 2, 0, bad, y, Xf)
        assert rc == -1 and "not finite" in msg, (rc, msg)
        with pytest.raises(GE) as ei:
            eng.observe(c["x"], np.where(np.arange(32).reshape(2, 4, 4) == 7, np.inf, O))
        assert ei.value.status == -1 and "not finite" in str(ei.value)
        F, G = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G, G0)
        # n_obs = 0 with X_final alone is a valid call
        rc, msg = raw_call(qoc, eng, xf, 0, 0, None, None, Xf)
        assert rc == 0, msg
        # the Python layer catches wrong shapes before the library is called
        for wrong in (O[:, :3], np.zeros((17, 4, 4)), np.zeros((c["E"], 2, 4, 4))):
            with pytest.raises(ValueError):
                eng.observe(c["x"], wrong)
        with pytest.raises(ValueError):
            eng.observe(c["x"], O, per_member=True)
        with pytest.raises(ValueError):
            eng.observe(c["x"][:, :5], O)
        with pytest.raises(ValueError):
            eng.observe(c["x"], None)
        # a NaN in x gives NaN out and no error
        xn = c["x"].copy()
        xn[1, 7] = np.nan
        yn, Xn, Fn = eng.observe(xn, O, final=True, want_F=True)
        assert np.isnan(Fn) and np.isnan(Xn).any() and np.isnan(yn[:, :, 8:]).all() and np.isfinite(yn[:, :, :8]).all()
        F, G = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G, G0)

    # before grape_set_operators
    lib = qoc.load_library()
    cfg = qoc.engine.GrapeConfig(0, 0, 4, 2, 20, 2, T, -1, 0, 0, 0, -1, 0)
    h = C.c_void_p()
    assert lib.grape_create(C.byref(cfg), C.byref(h)) == 0
    try:
        rc = lib.grape_eval_observables(h, xf.ctypes.data_as(C.c_void_p), 2, 0, Of.ctypes.data_as(C.c_void_p),
                                        y.ctypes.data_as(C.c_void_p), None, None)
        assert rc == -5 and b"operators not set" in lib.grape_last_error(h)
    finally:
        lib.grape_destroy(h)


# ---- 10: the mirror --------------------------------------------------------------------------------------------------------
def test_mirror_test_pulse(qoc):
    wl = qoc.workloads
    N = 10
    prob = qoc.Problem(B=[wl.Sx, wl.Sy], A=wl.Sz, Xi=wl.U_init, Xt=wl.U_fin, T=1.0, n_controls=2, guess=wl.controls(2, N),
                       sys_type=qoc.UnitaryGate())
    ens = qoc.EnsembleProblem(prob=prob, n_ens=3, A_g=lambda k: (k - 2) / 2 * wl.Sz, B_g=lambda k: [wl.Sx, wl.Sy],
                              XiG=lambda k: prob.Xi, XtG=lambda k: prob.Xt, wts=np.array([0.2, 0.5, 0.3]))
    for p in (prob, ens):
        alg = qoc.GRAPE(n_slices=N, optim_options={"iterations": 20})
        sol = qoc.solve(p, alg)
        Xf, member_F, F = qoc.test_pulse(p, sol)
        with qoc.api.make_engine(p, alg) as eng:
            F_eval, _ = eng.eval(sol.opti_pulses)
            Xf2, mF2, F2 = qoc.test_pulse(p, sol.opti_pulses, engine=eng)
        E = 3 if p is ens else 1
        assert Xf.shape == (E, 2, 2) and member_F.shape == (E,)
        assert abs(F - F_eval) <= 1e-10 * max(abs(F_eval), 1e-3 * 4), (F, F_eval)
        assert F2 == F and np.array_equal(Xf2, Xf)


def test_mirror_bloch_vector(qoc):
    """A deviation from the issue's wording ("the three Paulis on a ket"): an n x 1 ket under UnitaryGate cannot take 2 x 2
    probes (tr(O' X) needs O of the state's shape, and is an overlap there, not <psi|O|psi>).  The expectation values of an
    operator need the state as a density operator: the ket |0> is held as rho = |0><0| under StateTransfer; its Bloch
    vector keeps norm 1 along a unitary evolution."""
    wl = qoc.workloads
    N = 25
    sx, sy, sz = (np.array(m, complex) for m in ([[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]))
    prob = qoc.Problem(B=[wl.Sx, wl.Sy], A=wl.Sz, Xi=wl.rho_init, Xt=wl.rho_fin, T=2.0, n_controls=2, guess=wl.controls(2, N),
                       sys_type=qoc.StateTransfer())
    assert abs(np.trace(wl.rho_init @ wl.rho_init) - 1) < 1e-14          # a pure state
    times, y = qoc.expectation_values(prob, np.random.default_rng(3).standard_normal((2, N)), [sx, sy, sz])
    assert times.shape == (N + 1,) and times[0] == 0.0 and times[-1] == 2.0 and y.shape == (1, 3, N + 1)
    assert np.abs(y.imag).max() <= 1e-10
    assert np.abs(np.linalg.norm(y.real[0], axis=0) - 1.0).max() <= 1e-10
    assert np.abs(np.diff(y.real[0], axis=1)).max() > 1e-2             # (it moves)


def test_mirror_forbidden_level_occupation_is_the_running_cost(qoc):
    """The read-out against the cost it is meant to inspect: C5 on level 2 of a qutrit ket (ForbiddenStates, c5_case of the
    running-cost tests).  J = eval with the cost - eval without it = w sum_{s=1..N} rho |y_s|^2."""
    c = c5_case()
    prob = qoc.Problem(B=list(c["B"][0]), A=c["A"][0], Xi=c["Xi"][0], Xt=c["Xt"][0], T=T, n_controls=c["K"], guess=c["x"],
                       sys_type=qoc.UnitaryGate())
    with qoc.api.make_engine(prob, qoc.GRAPE(n_slices=c["N"])) as eng:
        F0, _ = eng.eval(c["x"])
    alg = qoc.GRAPE(n_slices=c["N"], running_costs=[qoc.ForbiddenStates([[0, 0, 1.0]], 0.8)])
    with qoc.api.make_engine(prob, alg) as eng:
        F1, _ = eng.eval(c["x"])
        _, y = qoc.expectation_values(prob, c["x"], np.array([[0.0], [0.0], [1.0]]), engine=eng)
    J = F1 - F0
    J_obs = 0.8 * float(np.sum(np.abs(y[0, 0, 1:]) ** 2))     # (a plain Problem carries weight 1)
    print(f"J={J:.15f} observed={J_obs:.15f}")
    assert J > 1e-3 and abs(J_obs - J) <= 1e-10 * J
