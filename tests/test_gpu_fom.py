"""GPU: grape_eval_fom (ABI v8), the figure of merit without the gradient, and the dCRAB solver built on it.

Reference values: oracle.ensemble_eval(per_member=True) for objective 0, oracle.ensemble_exact(objective=1, per_member=True)
for objective 1, and the 50-digit fixtures of tests/golden/.  Bar: |F - F_ref| <= 1e-10 max(1, |F_ref|), the same per member.
The fast path (n = 2, 3, 4 on one device) must run the forward-only kernels and no sweep kernel; everywhere else the call
returns the full evaluation's F bit for bit."""
import glob
import json
import os

import numpy as np
import pytest

from test_oracle_golden import load_case

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GOLDEN = [p for p in sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.json")))
          if json.load(open(p))["n"] <= 4]                      # the sizes the forward-only kernels serve


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    tol = RTOL * np.maximum(1.0, np.abs(ref))
    print(f"{what}: max |d| = {err.max():.3e}")
    assert np.all(err <= tol), f"{what}: |d| = {err.max():.3e} ({got} vs {ref})"


def fast_kernels(eng):
    names = eng.kernel_names()
    assert any(k in ("fom_lane_kernel", "fom_pair_kernel") for k in names), names
    assert not any(k.startswith("sweep_") for k in names), names
    return names


def random_problem(qoc, n, K, N, E, sys_type, seed, hermitian=True, m=None):
    rng = np.random.default_rng(seed)

    def gen(scale):
        M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        H = (M + M.conj().T) / 2
        if not hermitian:                        # a damping part: the generators are no longer Hermitian
            D = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
            H = H - 0.15j * (D @ D.conj().T) / n
        return H * scale
    A = np.array([gen(1.0) for _ in range(E)])
    B = np.array([[gen(0.5) for _ in range(K)] for _ in range(E)])
    if sys_type == "UnitaryGate":
        cols = m or n
        Xi = np.array([np.eye(n, dtype=complex)[:, :cols]] * E)
        Xt = np.array([np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0][:, :cols] for _ in range(E)])
    else:
        def rho():
            v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
            v /= np.linalg.norm(v)
            return np.outer(v, v.conj())
        Xi = np.array([rho() for _ in range(E)])
        Xt = np.array([rho() for _ in range(E)])
    return qoc.workloads.Workload("fom", sys_type, n, K, N, E, 1.3, A, B, Xi, Xt, rng.uniform(0.2, 1.7, E),
                                  rng.uniform(-1, 1, (K, N)))


def engine(qoc, w, **kw):
    return qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, **kw)


def check_fast(qoc, oracle, w, what, variant=0, **kw):
    """fom against the oracle (ensemble and per member) and against eval on the same context; the fast kernels ran."""
    F_ref, _, foms_ref, _ = oracle.ensemble_eval(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.x, w.T, variant=variant,
                                                 n_threads=8, per_member=True)
    with engine(qoc, w, variant=variant, **kw) as eng:
        F, mF = eng.fom(w.x, members=True)
        names = fast_kernels(eng)
        F_eval = eng.eval(w.x, want_G=False)[0]
        assert eng.fom(w.x) == F                                # identical calls agree bit for bit
    close(F, F_ref, f"{what} F")
    close(mF, foms_ref, f"{what} member F")
    close(F, F_eval, f"{what} fom vs eval")
    return names


# ------------------------------------------------------------------------------------------------- 1. fast path parity
@pytest.mark.parametrize("name,kw", [("C1", {}), ("C2", {}), ("L1d", {"E": 37, "N": 83}), ("L1d", {"E": 1024, "N": 1000})] +
                         [("C3", {"E": E, "N": N}) for E in (1, 37, 1024) for N in (1, 7, 83, 500)])
def test_fast_path_workloads(qoc, oracle, name, kw):
    w = qoc.workloads.config(name, **kw)
    names = check_fast(qoc, oracle, w, f"{name} {kw}")
    if name == "C2":
        assert w.N == 1000 and w.E == 1                         # one problem: the time axis spread over lanes
    if name in ("C3", "L1d"):
        assert "fom_pair_kernel" in names                       # n = 4: lane pairs


@pytest.mark.parametrize("sys_type", ["UnitaryGate", "StateTransfer", "CoherenceTransfer"])
@pytest.mark.parametrize("kernel", ["default", "pair"])
def test_fast_path_reference_ensembles(qoc, oracle, monkeypatch, sys_type, kernel):
    if kernel == "pair":
        monkeypatch.setenv("GRAPE_SMALL_KERNEL", "pair")
    w = qoc.workloads.reference_ensemble(sys_type, 5, 25, 5.0)
    names = check_fast(qoc, oracle, w, f"ref-ens {sys_type} {kernel}")
    assert ("fom_pair_kernel" if kernel == "pair" else "fom_lane_kernel") in names


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("sys_type", ["UnitaryGate", "StateTransfer", "CoherenceTransfer"])
@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("variant", [0, 1])
def test_fast_path_random(qoc, oracle, n, sys_type, hermitian, variant):
    seed = 100 * n + 10 * variant + int(hermitian)
    w = random_problem(qoc, n, 3, 131, 7, "UnitaryGate" if sys_type == "UnitaryGate" else "StateTransfer", seed, hermitian)
    w.sys_type = sys_type
    check_fast(qoc, oracle, w, f"random n={n} {sys_type} herm={hermitian} v{variant}", variant=variant)


@pytest.mark.parametrize("n,sys_type,kw", [(4, "UnitaryGate", {}), (4, "StateTransfer", {"waves_per_member": 4}),
                                          (2, "UnitaryGate", {"waves_per_member": 3}), (4, "UnitaryGate", {"m": 1}),
                                          (3, "UnitaryGate", {"m": 2, "waves_per_member": 2})])
def test_fast_path_lane_kernel_and_rect_states(qoc, oracle, monkeypatch, n, sys_type, kw):
    """GRAPE_SMALL_KERNEL=lane (whole matrices per lane at n = 4), several waves per member, n x m states."""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", "lane")
    kw = dict(kw)
    w = random_problem(qoc, n, 2, 300, 5, sys_type, 42 + n, hermitian=False, m=kw.pop("m", None))
    names = check_fast(qoc, oracle, w, f"lane n={n} {sys_type} {kw}", **kw)
    assert "fom_lane_kernel" in names


def test_fast_path_long_pulse_reads_controls_from_memory(qoc, oracle):
    """K N doubles beyond the LDS budget: the kernel reads x in place."""
    w = random_problem(qoc, 2, 2, 20000, 1, "UnitaryGate", 5)
    check_fast(qoc, oracle, w, "N = 20000")


# ------------------------------------------------------------------------------------------------- 2. squarings
@pytest.mark.parametrize("forced", [-1, 3])
def test_squaring_path(qoc, oracle, forced):
    w = qoc.workloads.config("C3", E=3, N=8)
    w.T = 24.0 if forced < 0 else w.T
    check_fast(qoc, oracle, w, f"squarings forced={forced}", expm_squarings=forced)


# ------------------------------------------------------------------------------------------------- 3. objective 1
@pytest.mark.parametrize("case", ["C3", "C3_T24", "ref_ug", "ref_st", "L1d", "rand3"])
def test_objective_c1(qoc, oracle, case):
    wl = qoc.workloads
    if case[:2] == "C3":
        w = wl.config("C3", E=37, N=83)
        if case == "C3_T24":
            w.T = 24.0
    elif case[:3] == "ref":
        w = wl.reference_ensemble("UnitaryGate" if case == "ref_ug" else "StateTransfer", 5, 25, 5.0)
    elif case == "L1d":
        w = wl.config("L1d", E=5, N=40)
    else:
        w = random_problem(qoc, 3, 2, 77, 4, "StateTransfer", 8, hermitian=False)
    Xi, Xt = w.Xi, w.Xt
    if Xi.shape[-1] != w.n:        # ensemble_exact takes square states: n x m states zero padded to n x n -- the same
        pad = ((0, 0), (0, 0), (0, w.n - Xi.shape[-1]))       # tr(Xt' U Xi) and the same D = n the device uses
        Xi, Xt = np.pad(Xi, pad), np.pad(Xt, pad)
    F_ref, _, foms_ref, _ = oracle.ensemble_exact(w.sys_type, w.A, w.B, Xi, Xt, w.wts, w.x, w.T, variant=1, objective=1,
                                                  per_member=True)
    with engine(qoc, w, variant=1, gradient="exact", objective="c1") as eng:
        F, mF = eng.fom(w.x, members=True)
        fast_kernels(eng)
        F_eval = eng.eval(w.x, want_G=False)[0]
    close(F, F_ref, f"c1 {case} F")
    close(mF, foms_ref, f"c1 {case} member F")
    close(F, F_eval, f"c1 {case} fom vs eval")


# ------------------------------------------------------------------------------------------------- 4. 50-digit fixtures
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-5] for p in GOLDEN])
def test_golden_fixtures(qoc, path):
    c, A, B, Xi, Xt, wts, x, exp, _ = load_case(path)
    with qoc.GrapeEngine(c["sys_type"], A, B, Xi, Xt, wts, c["T"], x.shape[1], variant=c["variant"]) as eng:
        F, mF = eng.fom(x, members=True)
        fast_kernels(eng)
    close(F, exp["F"], "golden F")
    close(mF, exp["member_F"], "golden member F")


# ------------------------------------------------------------------------------------------------- 6. fallback
@pytest.mark.parametrize("n", [1, 8, 16, 40, 70])
def test_fallback_is_the_full_evaluation(qoc, n):
    w = random_problem(qoc, n, 2, 12, 3, "UnitaryGate", 300 + n)
    with engine(qoc, w) as eng:
        assert eng.info["kernel_family"] != 0
        F, mF = eng.fom(w.x, members=True)
        assert not any(k.startswith("fom_") for k in eng.kernel_names())
        assert F == eng.eval(w.x, want_G=False)[0]
        assert np.array_equal(mF, eng.member_results()[0])
        assert eng.fom(w.x) == F


def test_fallback_group_and_member_rows(qoc):
    w = qoc.workloads.config("C3", E=9, N=33)
    flag = qoc.engine.FLAG_GROUP_PEER_SUM
    with engine(qoc, w, devices=[0, 0], flags=flag) as eng:
        F = eng.fom(w.x)
        assert F == eng.eval(w.x, want_G=False)[0]
        with pytest.raises(qoc.GrapeError) as exc:
            eng.fom(w.x, members=True)
        assert exc.value.status == -5 and "GRAPE_FLAG_MEMBER_RESULTS" in str(exc.value)
    with engine(qoc, w, devices=[0, 0], flags=flag, member_results=True, max_batch=2) as eng:
        X = np.stack([w.x, 0.5 * w.x])
        F, mF = eng.fom(X, members=True)
        for b in range(2):
            assert F[b] == eng.eval(X[b], want_G=False)[0]
            assert np.array_equal(mF[b], eng.member_results()[0])
        assert np.array_equal(eng.fom(X), eng.eval_batch(X)[0])


def test_fallback_member_chunked(qoc, monkeypatch):
    w = random_problem(qoc, 16, 2, 20, 6, "UnitaryGate", 77)
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(2 * 2 * w.N * 16 * 16 * 16 + 1000))
    with engine(qoc, w) as eng:
        assert eng.info["member_chunk"] < w.E
        F, mF = eng.fom(w.x, members=True)
        assert F == eng.eval(w.x, want_G=False)[0]
        assert np.array_equal(mF, eng.member_results()[0])


def test_fast_path_ignores_member_chunks(qoc, oracle, monkeypatch):
    """a member-chunked n = 4 context: the forward-only kernel stores no P_t and takes the ensemble in one launch."""
    w = qoc.workloads.config("C3", E=37, N=83)
    with engine(qoc, w) as eng:
        info = eng.info
    assert info["lane_pair"] == 1 and info["member_chunk"] == w.E
    per_member = info["slices_per_lane"] * 16 * 32 * info["waves_per_member"] * 16      # S n^2 CH double2 of P_t
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(9 * per_member))
    with engine(qoc, w) as eng:
        assert eng.info["member_chunk"] < w.E
        F = eng.fom(w.x)
        assert eng.kernel_names().count("fom_pair_kernel") == 1
        close(F, eng.eval(w.x, want_G=False)[0], "chunked fom vs eval")


# ------------------------------------------------------------------------------------------------- 7. batches
def test_batches(qoc, oracle):
    w = qoc.workloads.config("C3", E=37, N=83)
    rng = np.random.default_rng(3)
    X = np.stack([w.x, rng.uniform(-1, 1, w.x.shape), 0.25 * w.x])
    with engine(qoc, w, max_batch=3) as eng:
        F, mF = eng.fom(X, members=True)
        fast_kernels(eng)
        for b in range(3):
            Fb, mFb = eng.fom(X[b], members=True)
            assert F[b] == Fb and np.array_equal(mF[b], mFb)
            F_ref = oracle.ensemble_eval(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, X[b], w.T)[0]
            close(F[b], F_ref, f"batch entry {b}")
        assert np.array_equal(eng.fom(X[:2]), F[:2])
        with pytest.raises(qoc.GrapeError) as exc:
            eng.fom(np.concatenate([X, X[:1]]))
        assert exc.value.status == -1
    with engine(qoc, w, max_batch=0) as eng:
        assert eng.fom(w.x[None])[0] == eng.fom(w.x)


# ------------------------------------------------------------------------------------------------- 8. penalties
@pytest.mark.parametrize("name,kw", [("C3", {"E": 37, "N": 83}), ("C1", {})])
def test_penalties(qoc, name, kw):
    w = qoc.workloads.config(name, **kw)
    X = np.stack([w.x, 0.5 * w.x])
    with engine(qoc, w, max_batch=2) as eng:
        F0, mF0 = eng.fom(X, members=True)
        eng.set_penalties(amp=np.linspace(0.1, 0.3, w.K), var=0.7)
        F, mF = eng.fom(X, members=True)
        assert "reduce_rows_kernel" in eng.kernel_names()
        for b in range(2):
            Fe = eng.eval(X[b], want_G=False)[0]
            close(F[b], Fe, f"penalised fom vs eval, array {b}")
            assert abs(F[b] - F0[b]) > 1e-3                      # the penalty is there ...
            Fb = eng.fom(X[b])
            assert Fb == F[b]
        assert np.array_equal(mF, mF0)                           # ... and not in the members' values
        eng.set_penalties()
        assert np.array_equal(eng.fom(X), F0)


# ------------------------------------------------------------------------------------------------- 9. no side effects
def test_no_side_effects(qoc):
    w = qoc.workloads.config("C3", E=37, N=83)
    other = 0.3 * w.x[:, ::-1]
    with engine(qoc, w, member_results=True, flags=qoc.engine.FLAG_TIME_KERNELS) as eng:
        F1, G1 = eng.eval(w.x)
        foms1, grads1 = eng.member_results()
        P1 = eng.trajectory(3, states=False)[0]
        t1 = eng.kernel_time()
        eng.fom(other)
        fast_kernels(eng)
        foms2, grads2 = eng.member_results()
        assert np.array_equal(foms1, foms2) and np.array_equal(grads1, grads2)
        assert np.array_equal(P1, eng.trajectory(3, states=False)[0])
        assert eng.kernel_time() == t1
        F3, G3 = eng.eval(w.x)
        assert F3 == F1 and np.array_equal(G1, G3)
        assert any(k.startswith("sweep_") for k in eng.kernel_names())
    p = qoc.workloads.reference_ensemble("StateTransfer", 5, 25, 5.0)
    with engine(qoc, p) as eng:
        xa, ia = eng.lbfgs(p.x, iterations=15)
    with engine(qoc, p) as eng:
        eng.fom(0.3 * p.x[:, ::-1])
        xb, ib = eng.lbfgs(p.x, iterations=15)
    assert np.array_equal(xa, xb) and ia["minimum"] == ib["minimum"] and ia["evaluations"] == ib["evaluations"]


# ------------------------------------------------------------------------------------------------- 10. NaN, errors
def test_nan_and_errors(qoc):
    w = qoc.workloads.config("C3", E=5, N=40)
    x = w.x.copy()
    x[1, 17] = np.nan
    with engine(qoc, w) as eng:
        F, mF = eng.fom(x, members=True)
        assert np.isnan(F) and np.all(np.isnan(mF))
        assert np.isfinite(eng.fom(w.x))
        lib = qoc.load_library()
        one = np.zeros(1)
        assert lib.grape_eval_fom(eng._h, 1, None, one.ctypes.data, None) == -1
        assert lib.grape_eval_fom(eng._h, 1, np.ascontiguousarray(w.x.T).ctypes.data, None, None) == -1
        assert lib.grape_eval_fom(eng._h, 0, np.ascontiguousarray(w.x.T).ctypes.data, one.ctypes.data, None) == -1


# ------------------------------------------------------------------------------------------------- 11. dCRAB
def _single(qoc, sys_type, N, T):
    wl = qoc.workloads
    ug = sys_type == "UnitaryGate"
    return qoc.Problem(B=[wl.Sx, wl.Sy], A=wl.Sz, Xi=wl.U_init if ug else wl.rho_init,
                       Xt=wl.U_fin if ug else wl.rho_fin, T=T, n_controls=2, guess=wl.controls(2, N),
                       sys_type=qoc.UnitaryGate() if ug else qoc.StateTransfer())


def _functional(oracle, qoc, prob, x, N):
    members = qoc.init_ensemble(prob) if isinstance(prob, qoc.EnsembleProblem) else [prob]
    wts = np.asarray(prob.wts, float) if isinstance(prob, qoc.EnsembleProblem) else np.ones(1)
    A, B, Xi, Xt = qoc.api._pack(members)
    return oracle.ensemble_exact(members[0].sys_type.name, A, B, Xi, Xt, wts, x, members[0].T, variant=1, objective=1)[0]


@pytest.mark.parametrize("case", ["state_transfer", "unitary_gate", "ensemble"])
def test_dcrab(qoc, oracle, case):
    wl = qoc.workloads
    if case == "ensemble":
        N = 25
        base = _single(qoc, "StateTransfer", N, 5.0)
        prob = qoc.EnsembleProblem(prob=base, n_ens=5, A_g=lambda k: (k - 2.5) / 2.5 * wl.Sz * 5, B_g=lambda k: [wl.Sx, wl.Sy],
                                   XiG=lambda k: base.Xi, XtG=lambda k: wl.rho_fin if k % 2 else wl.rho_init,
                                   wts=np.ones(5) / 5)
        guess = base.guess
    else:
        N = 10
        prob = _single(qoc, "StateTransfer" if case == "state_transfer" else "UnitaryGate", N, 1.0)
        guess = prob.guess
    guess = np.array(guess, dtype=np.float64)
    sol = qoc.solve(prob, qoc.dCRAB(n_slices=N, seed=1))
    assert isinstance(sol, qoc.EnsembleSolutionResult if case == "ensemble" else qoc.SolutionResult)
    assert len(sol.result) == len(sol.fidelity) == 2 and sol.opti_pulses.shape == (2, N)
    assert np.array_equal(guess, np.asarray((prob.prob if case == "ensemble" else prob).guess))   # the guess is not modified
    F_guess = _functional(oracle, qoc, prob, guess, N)
    print(f"dCRAB {case}: guess {F_guess:.6f} -> {sol.fidelity}")
    assert sol.fidelity[0] <= F_guess + RTOL
    assert all(b <= a for a, b in zip(sol.fidelity, sol.fidelity[1:]))
    close(sol.fidelity[-1], _functional(oracle, qoc, prob, sol.opti_pulses, N), f"dCRAB {case} final value")
