"""GPU: the control penalties C3 / C4 (grape_set_penalties, src/cost_functions.jl:29-39, 66-69) on every flow.  The
reference value is the oracle's [G, F] plus a NumPy penalty written here from the formulas of include/grape_hip.h; the
penalty is counted once per control array whatever the path (batches, member chunks, shards, ranks), penalties off is the
library without them bit for bit, and grape_lbfgs minimises the penalised objective."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_parity

pytestmark = pytest.mark.gpu


def penalty_ref(x, amp, var):
    x = np.asarray(x, dtype=np.float64)
    a = np.zeros(x.shape[0]) if amp is None else np.asarray(amp, dtype=np.float64)
    v = np.zeros(x.shape[0]) if var is None else np.asarray(var, dtype=np.float64)
    d = np.diff(x, axis=1)
    F = float(np.sum(a[:, None] * x ** 2) + np.sum(v[:, None] * d ** 2))
    G = 2 * a[:, None] * x
    G[:, 1:] += 2 * v[:, None] * d
    G[:, :-1] -= 2 * v[:, None] * d
    return F, G


def weights(K):
    """different weights per control, one of them zero"""
    amp = np.linspace(0.3, 0.9, K)
    var = np.linspace(0.8, 0.2, K)
    if K > 1:
        amp[1] = 0.0
    else:
        var[0] = 0.5
    return amp, var


def _random(qoc, n, K, N, E, sys_type, seed, hermitian=True):
    rng = np.random.default_rng(seed)

    def rnd():
        M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        return (M + M.conj().T) / 2 if hermitian else M
    A = np.array([rnd() for _ in range(E)]) * 0.7
    B = np.array([[rnd() for _ in range(K)] for _ in range(E)]) * 0.5
    if sys_type == "UnitaryGate":
        Xi = np.array([np.eye(n, dtype=complex)] * E)
        Xt = np.array([np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0] for _ in range(E)])
    else:
        def pure():
            v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
            v /= np.linalg.norm(v)
            return np.outer(v, v.conj())
        Xi = np.array([pure() for _ in range(E)])
        Xt = np.array([pure() for _ in range(E)])
    return qoc.workloads.Workload("rnd", sys_type, n, K, N, E, 1.0, A, B, Xi, Xt, np.full(E, 1.0 / E),
                                  rng.uniform(-1, 1, (K, N)))


def _scaled_c4(qoc):
    w = qoc.workloads.config("C4", E=6, N=20)
    s = np.linspace(0.8, 1.2, w.E)
    w.B = np.array([w.B[0] * s[k] for k in range(w.E)])
    return w


CASES = {
    "n2_sweep_small": lambda q: q.workloads.config("C1"),
    "n3_sweep_small": lambda q: _random(q, 3, 2, 12, 4, "StateTransfer", 3),
    "n4_unitary_direct": lambda q: q.workloads.config("C3", E=8, N=100),
    "n4_general": lambda q: q.workloads.config("C3", E=8, N=100),
    "n8_tile": lambda q: _random(q, 8, 2, 12, 3, "StateTransfer", 8),
    "n16_hoisted": lambda q: q.workloads.config("C4", E=9, N=21),
    "n16_rank_one": lambda q: q.workloads.config("C4", E=2, N=40),
    "n16_single_fold": lambda q: q.workloads.config("C4", E=1, N=30),
    "n40_grid": lambda q: _random(q, 40, 2, 6, 2, "UnitaryGate", 40),
    "n70_size_generic": lambda q: _random(q, 70, 2, 4, 2, "UnitaryGate", 70),
    "n1": lambda q: _random(q, 1, 2, 10, 3, "UnitaryGate", 1),
    "c4_scaled_controls": _scaled_c4,
}


def _reference(oracle, w, amp, var, x=None, **kw):
    x = w.x if x is None else x
    F, G = oracle.ensemble_eval(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, x, w.T, **kw)
    Fp, Gp = penalty_ref(x, amp, var)
    return F + Fp, G + Gp


def _engine(qoc, w, **kw):
    return qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, **kw)


@pytest.mark.parametrize("case", sorted(CASES))
def test_penalised_parity_on_every_flow(qoc, oracle, case):
    w = CASES[case](qoc)
    amp, var = weights(w.K)
    flags = qoc.engine.FLAG_FORCE_GENERAL if case == "n4_general" else 0
    F_ref, G_ref = _reference(oracle, w, amp, var)
    with _engine(qoc, w, flags=flags) as eng:
        F0, _ = eng.eval(w.x)
        eng.set_penalties(amp, var)
        F, G = eng.eval(w.x)
        info = eng.info
    assert_parity(F, G, F_ref, G_ref, w.n, what=case)
    assert F != F0
    if case == "n16_hoisted":
        assert info["hoisted_controls"] == 1
    if case == "n16_rank_one":
        assert info["rank_one_chain"] == 1
    if case == "c4_scaled_controls":
        assert info["scaled_controls"] == 1
    if case == "n40_grid":
        assert info["kernel_family"] == 1
    if case in ("n70_size_generic", "n1"):
        assert info["kernel_family"] == 2


@pytest.mark.parametrize("which", ["n4", "n16"])
def test_exact_gradient_and_c1_objective_with_penalties(qoc, oracle, which):
    w = qoc.workloads.config("C3", E=4, N=20) if which == "n4" else _random(qoc, 16, 2, 8, 2, "UnitaryGate", 16)
    amp, var = weights(w.K)
    for objective, variant in (("fom", 0), ("c1", 1)):
        F, G = oracle.ensemble_exact(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.x, w.T, variant=variant,
                                     objective=0 if objective == "fom" else 1)
        Fp, Gp = penalty_ref(w.x, amp, var)
        with _engine(qoc, w, gradient="exact", objective=objective, variant=variant) as eng:
            eng.set_penalties(amp, var)
            Fd, Gd = eng.eval(w.x)
        assert_parity(Fd, Gd, F + Fp, G + Gp, w.n, what=f"{which} {objective}")


@pytest.mark.parametrize("case", ["n4_unitary_direct", "n16_single_fold", "n16_hoisted", "n2_sweep_small"])
def test_penalties_off_is_the_library_without_them(qoc, case):
    w = CASES[case](qoc)
    amp, var = weights(w.K)
    res = []
    for mode in ("never", "null", "zeros", "cleared"):
        with _engine(qoc, w) as eng:
            if mode == "null":
                eng.set_penalties(None, None)
            elif mode == "zeros":
                eng.set_penalties(np.zeros(w.K), np.zeros(w.K))
            elif mode == "cleared":
                eng.set_penalties(amp, var)
                Fp, _ = eng.eval(w.x)
                eng.set_penalties(None, None)
            F, G = eng.eval(w.x)
            res.append((F, G, eng.kernel_names()))
    for F, G, names in res[1:]:
        assert F == res[0][0] and np.array_equal(G, res[0][1]) and names == res[0][2], case


def test_member_results_do_not_carry_the_penalty(qoc):
    w = qoc.workloads.config("C4", E=3, N=12)
    amp, var = weights(w.K)
    with _engine(qoc, w, member_results=True) as eng:
        eng.eval(w.x)
        f0, g0 = eng.member_results()
        eng.set_penalties(amp, var)
        eng.eval(w.x)
        f1, g1 = eng.member_results()
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1)


def _close(a, b, rel=1e-13):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def _same(F, G, F0, G0, what):
    assert _close(F, F0), (what, F, F0)
    assert np.abs(G - G0).max() <= 1e-13 * np.abs(G0).max(), what


@pytest.mark.parametrize("cfg", ["C3", "C4"])
def test_batch_entries_each_carry_their_own_penalty(qoc, oracle, cfg):
    w = qoc.workloads.config(cfg, E=8, N=100) if cfg == "C3" else qoc.workloads.config("C4", E=3, N=12)
    amp, var = weights(w.K)
    rng = np.random.default_rng(2)
    X = np.array([w.x, 0.5 * w.x, w.x + 0.2 * rng.standard_normal(w.x.shape)])
    with _engine(qoc, w, max_batch=3) as eng:
        eng.set_penalties(amp, var)
        Fb, Gb = eng.eval_batch(X)
        for b in range(3):
            F, G = eng.eval(X[b])
            _same(Fb[b], Gb[b], F, G, f"batch entry {b}")
    F_ref, G_ref = _reference(oracle, w, amp, var, x=X[2])
    assert_parity(Fb[2], Gb[2], F_ref, G_ref, w.n, what="batch entry 2")


def test_counted_once_on_chunks_shards_and_collectives(qoc, monkeypatch):
    w = _random(qoc, 70, 2, 4, 5, "UnitaryGate", 71)
    amp, var = weights(w.K)
    with _engine(qoc, w) as eng:
        eng.set_penalties(amp, var)
        F0, G0 = eng.eval(w.x)
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(2 * 2 * w.N * 70 * 70 * 16 + 1000))
    with _engine(qoc, w) as eng:
        eng.set_penalties(amp, var)
        F, G = eng.eval(w.x)
        assert eng.info["member_chunk"] == 2
    _same(F, G, F0, G0, "member-chunked")
    monkeypatch.delenv("GRAPE_MAX_WORKSPACE_BYTES")
    w = qoc.workloads.config("C3", E=8, N=100)
    amp, var = weights(w.K)
    with _engine(qoc, w) as eng:
        eng.set_penalties(amp, var)
        F0, G0 = eng.eval(w.x)
    with _engine(qoc, w, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM) as eng:
        eng.set_penalties(amp, var)                           # (before or after the operators: here after)
        F, G = eng.eval(w.x)
    _same(F, G, F0, G0, "devices=[0, 0] peer sum")
    with _engine(qoc, w, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM, max_batch=2) as eng:
        eng.set_penalties(amp, var)
        Fb, Gb = eng.eval_batch(np.array([w.x, w.x]))
    _same(Fb[1], Gb[1], F0, G0, "devices=[0, 0] batch")
    with _engine(qoc, w, force_collective=True, device=0) as eng:
        eng.set_penalties(amp, var)
        F, G = eng.eval(w.x)
    _same(F, G, F0, G0, "1-rank collective")


def test_two_ipc_ranks_count_the_penalty_once(qoc, tmp_path):
    w = qoc.workloads.config("C3", E=10, N=60)
    amp, var = weights(w.K)
    with _engine(qoc, w) as eng:
        eng.set_penalties(amp, var)
        F0, G0 = eng.eval(w.x)
    out = str(tmp_path / "pen")
    port = 29600 + (os.getpid() + 11) % 300
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "workers", "ipc_penalty_rank.py"), out, str(w.E), str(w.N)]
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = [np.load(f"{out}.rank{r}.npz") for r in range(2)]
    assert all(str(r["collective"]) == "ipc" for r in res), [str(r["error"]) for r in res]
    for r in res:
        _same(float(r["F"]), r["G"], F0, G0, "ipc rank")
        assert float(r["F"]) == float(res[0]["F"]) and np.array_equal(r["G"], res[0]["G"])


def test_eval_device_writes_the_penalised_row(qoc, oracle):
    import torch
    w = qoc.workloads.config("C3", E=8, N=100)
    amp, var = weights(w.K)
    with _engine(qoc, w, device=0) as eng:
        eng.set_penalties(amp, var)
        F, G = eng.eval(w.x)
        xd = torch.as_tensor(np.ascontiguousarray(w.x.T), device="cuda:0")
        fg = torch.zeros(w.K * w.N + 1, dtype=torch.float64, device="cuda:0")
        eng.eval_device(xd.data_ptr(), fg.data_ptr(), torch.cuda.current_stream(0).cuda_stream)
        torch.cuda.synchronize(0)
        h = fg.cpu().numpy()
        eng.set_penalties(2 * amp, None)                      # ordered behind the device evaluation
        F2, G2 = eng.eval(w.x)
    assert h[-1] == F and np.array_equal(h[:-1].reshape(w.N, w.K).T, G)
    F_ref, G_ref = _reference(oracle, w, 2 * amp, None)
    assert_parity(F2, G2, F_ref, G_ref, w.n, what="after re-setting the weights")


def test_device_lbfgs_minimises_the_penalised_objective(qoc):
    """C3's shape with the exact gradient (the reference's UnitaryGate gradient is not the derivative of its figure of
    merit, so no line search can converge on it); the penalised minimum against SciPy's L-BFGS-B on the same objective."""
    from scipy.optimize import minimize
    w = qoc.workloads.config("C3", E=4, N=20)
    amp, var = np.array([0.02, 0.03, 0.0, 0.01])[:w.K], np.array([0.05, 0.0, 0.02, 0.04])[:w.K]
    g_tol = 1e-7
    with _engine(qoc, w, gradient="exact") as eng:
        x_free, info_free = eng.lbfgs(w.x, g_tol=g_tol, iterations=500)
        eng.set_penalties(amp, var)
        x_min, info = eng.lbfgs(w.x, g_tol=g_tol, iterations=500)
        F, G = eng.eval(x_min)
        assert info["status"] == 0, info
        assert np.abs(G).max() <= g_tol and info["g_norm"] <= g_tol
        assert F == pytest.approx(info["minimum"], rel=1e-12, abs=1e-15)

        def fun(xf):
            Fh, Gh = eng.eval(xf.reshape(w.x.shape))
            return Fh, Gh.reshape(-1)
        ref = minimize(fun, w.x.reshape(-1), jac=True, method="L-BFGS-B",
                       options={"gtol": 1e-10, "ftol": 1e-15, "maxiter": 2000, "maxls": 40})
        assert abs(ref.fun - info["minimum"]) <= 1e-8, (ref.fun, info["minimum"])
        eng.set_penalties(np.full(w.K, 5.0), None)
        x_big, _ = eng.lbfgs(w.x, g_tol=g_tol, iterations=500)
    assert np.abs(x_big).max() < np.abs(x_free).max()


def test_invalid_weights_are_refused_and_the_old_ones_stay(qoc):
    w = qoc.workloads.config("C3", E=8, N=100)
    amp, var = weights(w.K)
    with _engine(qoc, w) as eng:
        eng.set_penalties(amp, var)
        F0, G0 = eng.eval(w.x)
        for bad in (np.nan, np.inf, -1.0):
            a = amp.copy()
            a[0] = bad
            with pytest.raises(qoc.GrapeError) as ei:
                eng.set_penalties(a, var)
            assert ei.value.status == -1
            with pytest.raises(qoc.GrapeError):
                eng.set_penalties(None, np.full(w.K, bad))
            F, G = eng.eval(w.x)
            assert F == F0 and np.array_equal(G, G0)


def test_solve_with_penalty_functionals(qoc, oracle):
    """GRAPE(penalties=...) through make_engine: the host optimiser's minimum includes the penalty."""
    w = qoc.workloads.reference_ensemble("StateTransfer", 5, 25, 5.0)
    prob = qoc.Problem(B=list(w.B[0]), A=w.A[0], Xi=w.Xi[0], Xt=w.Xt[0], T=w.T, n_controls=w.K, guess=w.x,
                       sys_type=qoc.StateTransfer())
    pf = qoc.PenaltyFunctionals([0.01, [0.02, 0.03]], [qoc.C3, qoc.C4])
    alg = qoc.GRAPE(n_slices=w.N, penalties=pf, optim_options={"iterations": 50})
    eng = qoc.api.make_engine(prob, alg)
    try:
        F, G = eng.eval(w.x)
    finally:
        eng.close()
    F_ref, G_ref = oracle.ensemble_eval(w.sys_type, w.A[:1], w.B[:1], w.Xi[:1], w.Xt[:1], np.ones(1), w.x, w.T)
    assert_parity(F, G, F_ref + pf(w.x), G_ref + penalty_ref(w.x, *pf.device_weights(w.K))[1], w.n, what="make_engine")
    sol = qoc.solve(prob, qoc.GRAPE(n_slices=w.N, penalties=pf, optimizer="device"))
    eng = qoc.api.make_engine(prob, alg)
    try:
        assert sol.fidelity == pytest.approx(eng.eval(sol.opti_pulses)[0], rel=1e-12)
    finally:
        eng.close()
