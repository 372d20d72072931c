"""GPU: the soft worst case over the ensemble on the device (grape_set_risk / grape_get_risk_weights).

With a risk in force every family's final reduction is risk_weights_kernel + the weighted sum of the members' unweighted rows
with this evaluation's weights p, F_beta in front of the penalty.  What is checked, and against what:

  parity       F, G through conftest.assert_parity (1e-10) and p to 1e-10 W against tests/risk_reference.py -- the oracle's
               per-member (F_k, g_k), the header's formulas in NumPy, settings_sequences.penalty_ref, basis and bounds as
               bounds_sequences lays them around the evaluation.  No device result enters the reference.  The device's F_k
               agree with the oracle to about 4e-14 relative and p_k inherits beta times that, so every case keeps
               |beta| max_k |F_k| <= 20 (asserted): two orders of margin.
  collapse     beta = +-2000 / gap: every weight but one underflows to exactly 0 -- F, G, p of the extreme member at 1e-10.
  bits         the entry points against each other, member-chunked against unchunked, call to call, and off against a
               context that never set a risk.
"""
import numpy as np
import pytest

import risk_reference as rr
from conftest import assert_parity
from test_gpu_basis import sized
from test_gpu_tile import _random_problem

pytestmark = pytest.mark.gpu
MAX_EXPONENT = 20.0
SYS_TYPES = ("UnitaryGate", "StateTransfer", "CoherenceTransfer")


def engine(qoc, w, **kw):
    return qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, **kw)


def check_parity(eng, w, foms, grads, beta, what, names_have=True):
    """one evaluation under the risk beta against the reference built from the oracle's (foms, grads); returns (F, G, p)"""
    W = w.wts.sum()
    assert abs(beta) * np.abs(foms).max() <= MAX_EXPONENT, (what, beta, np.abs(foms).max())
    F_ref, G_ref, p_ref = rr.combine(foms, grads, w.wts, beta)
    eng.set_risk(beta)
    F, G = eng.eval(w.x)
    names = eng.kernel_names()
    p = eng.risk_weights()
    print(f"{what} beta={beta}: |dF| = {abs(F - F_ref):.2e}, max |dG| / max |G_ref| = "
          f"{np.abs(G - G_ref).max() / np.abs(G_ref).max():.2e}, max |dp| / W = {np.abs(p - p_ref).max() / W:.2e}")
    if names_have:
        assert "risk_weights_kernel" in names, names
    assert_parity(F, G, F_ref, G_ref, w.n, what=f"{what} beta={beta}")
    assert p.shape == (w.E,) and np.abs(p - p_ref).max() <= 1e-10 * W, (what, beta)
    assert np.all(p[w.wts == 0] == 0.0)
    return F, G, p


def draw_bounded(oracle, n, K, N, E, sys_type, seed, herm, variant, beta_max, **kw):
    """the first problem from `seed` on (steps of 1000) whose oracle F_k keep |beta| max |F_k| <= 20 for every beta used"""
    for s in range(seed, seed + 20000, 1000):
        w = rr.problem(n, K, N, E, sys_type, s, hermitian=herm, **kw)
        foms, grads = rr.members(oracle, w, w.x, variant)
        if beta_max * np.abs(foms).max() <= MAX_EXPONENT:
            return w, foms, grads
    raise AssertionError("no draw inside the bound")


# ---- 1. parity on the small kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("herm", [True, False])
@pytest.mark.parametrize("n,kernel", [(2, "lane"), (2, "pair"), (3, "lane"), (4, "lane"), (4, "pair")])
def test_parity_on_the_small_kernels(qoc, oracle, monkeypatch, n, kernel, herm, variant):
    """N in {1, 5, 83} x E in {1, 7} x K in {1, 3}, beta in {-3, 0.5, 6} on each context; the three system types take turns"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    i = 0
    for N in (1, 5, 83):
        for E in (1, 7):
            for K in (1, 3):
                sys_type = SYS_TYPES[(i + n + variant) % 3]
                i += 1
                w, foms, grads = draw_bounded(oracle, n, K, N, E, sys_type, 100 * n + 10 * i + 2 * variant + herm, herm,
                                              variant, 6.0)
                assert E == 1 or (w.wts == 0).sum() == 1
                with engine(qoc, w, variant=variant) as eng:
                    info = eng.info
                    assert info["lane_pair"] == (1 if kernel == "pair" else 0) and info["kernel_family"] == 0
                    for beta in (-3.0, 0.5, 6.0):
                        check_parity(eng, w, foms, grads, beta, f"n={n} {kernel} {sys_type} herm={herm} v{variant} N={N} E={E} K={K}")


# ---- 2. parity elsewhere --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,sys_type,family", [(8, "StateTransfer", 1), (40, "UnitaryGate", 1), (1, "UnitaryGate", 2),
                                                (66, "UnitaryGate", 2)])
def test_parity_in_the_other_families(qoc, oracle, n, sys_type, family):
    if n == 1:                                               # (Hermitian 1 x 1 generators only turn a phase: G would be 0)
        w = _random_problem(qoc, 1, 3, 12, 3, sys_type, seed=901, hermitian=False)
        w.A *= 0.6
        w.B *= 0.6
    else:
        w = sized(qoc, n, sys_type, 900 + n)
    w.wts = np.array([0.7, 0.0, 1.1])[:w.E] if w.E == 3 else np.array([0.4, 1.3])
    foms, grads = rr.members(oracle, w, w.x)
    assert np.abs(grads).max() > 1e-3
    b = min(4.0, 0.5 * MAX_EXPONENT / np.abs(foms).max())     # (|F_k| reaches 10 at n = 40: beta drawn inside the bound)
    with engine(qoc, w) as eng:
        assert eng.info["kernel_family"] == family
        for beta in (-0.75 * b, b):
            check_parity(eng, w, foms, grads, beta, f"n={n} {sys_type}")


@pytest.mark.parametrize("n", [2, 8])
def test_parity_with_the_exact_gradient_of_c1(qoc, oracle, n):
    if n == 2:
        w = rr.problem(2, 3, 20, 5, "StateTransfer", seed=21)
    else:
        w = sized(qoc, 8, "StateTransfer", 908)
        w.wts = np.array([0.7, 0.0, 1.1])
    foms, grads = rr.members(oracle, w, w.x, variant=1, exact=True, objective=1)
    with engine(qoc, w, variant=1, gradient="exact", objective="c1") as eng:
        for beta in (-3.0, 6.0):
            check_parity(eng, w, foms, grads, beta, f"exact c1 n={n}")


# ---- 3. collapse onto the worst member ------------------------------------------------------------------------------------
def test_collapse_onto_the_extreme_member(qoc, oracle):
    """beta = 2000 / gap: exp(-2000) is 0 in double precision, so S is the extreme member's term alone and
    F = W F_max + (W / beta) log(w_max / W), G = W g_max, p = W e_max -- exactly, on the reference and on the device"""
    for seed in range(300, 400):
        w = rr.problem(4, 2, 20, 6, "StateTransfer", seed, zero_weight=False)
        foms, grads = rr.members(oracle, w, w.x)
        f = np.sort(foms)
        if f[-1] - f[-2] >= 1e-3 and f[1] - f[0] >= 1e-3:
            break
    else:
        raise AssertionError("no draw with both gaps >= 1e-3")
    W = w.wts.sum()
    with engine(qoc, w) as eng:
        for sign, k, gap in ((1.0, int(np.argmax(foms)), f[-1] - f[-2]), (-1.0, int(np.argmin(foms)), f[1] - f[0])):
            beta = sign * 2000.0 / gap
            eng.set_risk(beta)
            F, G = eng.eval(w.x)
            p = eng.risk_weights()
            F_want, G_want = W * foms[k] + (W / beta) * np.log(w.wts[k] / W), W * grads[k]
            F_ref, G_ref, p_ref = rr.combine(foms, grads, w.wts, beta)
            assert abs(F_ref - F_want) <= 1e-13 * W and np.array_equal(G_ref, G_want)       # the reference collapses as well
            print(f"beta = {beta:.4g}: F = {F!r} (want {F_want!r}), p = {p}")
            assert np.isfinite(F) and np.all(np.isfinite(G)) and np.all(np.isfinite(p))
            assert_parity(F, G, F_want, G_want, 4, what=f"collapse beta={beta:.4g}")
            assert np.count_nonzero(p) == 1 and abs(p[k] - W) <= 1e-10 * W


# ---- 4. composition -------------------------------------------------------------------------------------------------------
def _device_eval(eng, arr, K, cols):
    import torch
    xd = torch.as_tensor(np.ascontiguousarray(arr.T), device="cuda:0")
    fg = torch.zeros(K * cols + 1, dtype=torch.float64, device="cuda:0")
    eng.eval_device(xd.data_ptr(), fg.data_ptr(), torch.cuda.current_stream(0).cuda_stream)
    torch.cuda.synchronize(0)
    h = fg.cpu().numpy()
    return h[-1], h[:-1].reshape(cols, K).T


@pytest.mark.parametrize("n,kernel,herm", [(4, "pair", True), (3, "lane", False)])
def test_composition_with_penalties_basis_and_bounds(qoc, oracle, monkeypatch, n, kernel, herm):
    """expand / saturate -> evaluate -> risk-weighted sum -> penalty -> slope / projection, against the composed reference; and
    the entry points against each other, bit for bit"""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    K, N, E, M = 3, 20, 5, 4
    w = rr.problem(n, K, N, E, "UnitaryGate", seed=40 + n, hermitian=herm)
    rng = np.random.default_rng(41 + n)
    phi, x0 = rng.standard_normal((N, M)), 0.3 * rng.standard_normal((K, N))
    lo, hi = np.array([-0.6, -np.inf, -0.2]), np.array([0.8, np.inf, 1.1])
    pen = (np.array([0.3, 0.5, 0.2]), np.array([0.1, 0.05, 0.25]))
    thetas = rng.uniform(-1, 1, (3, K, M)) / np.sqrt(M)
    probes = rng.standard_normal((2, n, n)) + 1j * rng.standard_normal((2, n, n))
    xs = [rr.composed(oracle, w, th, 0.0, 0, pen, phi, x0, (lo, hi))[3] for th in thetas]
    fk = max(np.abs(rr.members(oracle, w, x)[0]).max() for x in xs)
    beta = min(4.0, 0.5 * MAX_EXPONENT / fk)
    assert beta * fk <= MAX_EXPONENT
    refs = [rr.composed(oracle, w, th, beta, 0, pen, phi, x0, (lo, hi)) for th in thetas]
    with engine(qoc, w, max_batch=3) as eng:
        eng.set_penalties(*pen)
        eng.set_basis(phi, x0)
        eng.set_bounds(lo, hi)
        y_plain = eng.observe(thetas[0], probes)
        F_plain = eng.eval(thetas[0], want_G=False)[0]
        eng.set_risk(beta)
        single = [eng.eval(th) for th in thetas]
        names = eng.kernel_names()
        p = eng.risk_weights()
        again = eng.eval(thetas[0])
        F_only = eng.eval(thetas[1], want_G=False)[0]
        Fb, Gb = eng.eval_batch(thetas)
        p_batch = eng.risk_weights()
        Fd, Gd = _device_eval(eng, thetas[2], K, M)
        f1 = eng.fom(thetas[0])
        f2, mF = eng.fom(thetas[1], members=True)
        fb, mFb = eng.fom(thetas, members=True)
        y, F_obs = eng.observe(thetas[0], probes, want_F=True)
    assert names[0] == "basis_expand_kernel" and names[-1] == "basis_project_kernel" and "risk_weights_kernel" in names, names
    for b in range(3):
        F_ref, G_ref, p_ref, x_ref = refs[b]
        assert_parity(single[b][0], single[b][1], F_ref, G_ref, n, what=f"composition {b}")
        assert single[b][1].shape == (K, M)
    assert np.abs(p - refs[2][2]).max() <= 1e-10 * w.wts.sum()               # (the last single evaluation: thetas[2])
    assert np.abs(p_batch - refs[0][2]).max() <= 1e-10 * w.wts.sum()         # (array 0 of the batch)
    assert abs(F_plain - single[0][0]) > 1e-6                                # the risk bites
    assert again[0] == single[0][0] and np.array_equal(again[1], single[0][1])
    assert F_only == single[1][0]
    for b in range(3):
        assert Fb[b] == single[b][0] and np.array_equal(Gb[b], single[b][1]), b
        assert fb[b] == single[b][0], b
    assert Fd == single[2][0] and np.array_equal(Gd, single[2][1])
    assert f1 == single[0][0] and f2 == single[1][0] and F_obs == single[0][0]
    # member_F: the members' unweighted F_k of the physical pulse, whatever the risk
    mF_ref = rr.members(oracle, w, xs[1])[0]
    assert np.abs(mF - mF_ref).max() <= 1e-10 * max(1.0, np.abs(mF_ref).max())
    assert np.array_equal(mFb[1], mF)
    assert np.array_equal(y, y_plain)                                        # the read-out does not see the risk


# ---- 5. member-chunked context --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("herm", [True, False])
def test_member_chunked_context_is_the_unchunked_one(qoc, oracle, monkeypatch, herm):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", "lane")
    w = rr.problem(4, 2, 65, 7, "UnitaryGate", seed=50, hermitian=herm)
    foms, grads = rr.members(oracle, w, w.x)
    beta = min(6.0, 0.5 * MAX_EXPONENT / np.abs(foms).max())
    X = np.array([w.x, 0.5 * w.x])
    res = []
    for budget in (None, int(2.5 * 2 * 16 * 1 * 16 * 64 * 2)):     # two and a half members' propagators and states
        if budget:
            monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(budget))
        with engine(qoc, w, waves_per_member=2, max_batch=2) as eng:
            F, G, p = check_parity(eng, w, foms, grads, beta, f"budget {budget}")
            F2, G2 = eng.eval(w.x)
            p2 = eng.risk_weights()
            assert F2 == F and np.array_equal(G2, G) and np.array_equal(p2, p), "not reproducible call to call"
            Fb, Gb = eng.eval_batch(X)
            assert Fb[0] == F and np.array_equal(Gb[0], G)
            res.append((F, G, p, Fb, Gb, eng.info["member_chunk"]))
    r0, r1 = res
    assert 0 < r1[5] < 7 and not 0 < r0[5] < 7, (r0[5], r1[5])
    for a, b in zip(r0[:5], r1[:5]):
        assert np.array_equal(a, b)


# ---- 6. off means off -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C3", "C4", "C1"])
def test_off_means_off(qoc, cfg):
    wl = qoc.workloads
    w = {"C3": lambda: wl.config("C3", E=8, N=100), "C4": lambda: wl.config("C4", E=3, N=12), "C1": lambda: wl.config("C1")}[cfg]()
    X = np.array([w.x, 0.5 * w.x])

    def observe(eng):
        F, G = eng.eval(w.x)
        names = eng.kernel_names()
        f = eng.fom(w.x)
        fnames = eng.kernel_names()
        Fb, Gb = eng.eval_batch(X)
        return F, G, names, f, fnames, Fb, Gb, eng.kernel_names()

    def same(a, b):
        return all(np.array_equal(p, q) if isinstance(p, np.ndarray) else p == q for p, q in zip(a, b))

    with engine(qoc, w, max_batch=2) as never:
        base = observe(never)
        with pytest.raises(qoc.GrapeError) as ei:
            never.risk_weights()
        assert ei.value.status == -5
    assert not any("risk" in k for k in base[2] + base[4] + base[7])
    with engine(qoc, w, max_batch=2) as eng:
        eng.set_risk(2.0)
        with pytest.raises(qoc.GrapeError) as ei:            # set, not evaluated yet
            eng.risk_weights()
        assert ei.value.status == -5
        on = observe(eng)
        assert "risk_weights_kernel" in on[2] and "risk_weights_kernel" in on[4] and on[7].count("risk_weights_kernel") == 2
        assert on[3] == on[0]                                # fom takes its fallback: eval's F
        if w.E > 1:
            assert on[0] != base[0]
        if eng.info["kernel_family"] == 0:                   # the rows this feature keeps are private to it
            with pytest.raises(qoc.GrapeError) as ei:
                eng.member_results()
            assert ei.value.status == -5
        eng.set_risk(0.0)
        assert same(observe(eng), base), "set -> 0"
        with pytest.raises(qoc.GrapeError) as ei:
            eng.risk_weights()
        assert ei.value.status == -5
    with engine(qoc, w, max_batch=2) as eng:
        eng.set_risk(0.0)
        assert same(observe(eng), base), "beta = 0 from the start"


# ---- 7. re-upload under a standing risk -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kernel", [(2, "pair"), (3, "lane"), (4, "pair")])
def test_risk_persists_across_set_operators(qoc, oracle, monkeypatch, n, kernel):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    ws = [rr.problem(n, 2, 20, 5, "StateTransfer", seed=70 + n + h, hermitian=bool(h)) for h in (1, 0, 1)]
    beta = 5.0
    with engine(qoc, ws[0]) as eng:
        eng.set_risk(beta)
        for w, flow in zip(ws, (1, 0, 1)):
            eng.set_operators(w.A, w.B, w.Xi, w.Xt, w.wts)
            assert eng.info["unitary_flow"] == flow
            with pytest.raises(qoc.GrapeError) as ei:        # the weights of the previous operators are gone with them
                eng.risk_weights()
            assert ei.value.status == -5
            foms, grads = rr.members(oracle, w, w.x)
            check_parity(eng, w, foms, grads, beta, f"upload herm={flow}")


# ---- 8. refusals and arguments --------------------------------------------------------------------------------------------
def test_refusals_and_arguments(qoc, oracle):
    w = rr.problem(4, 2, 20, 4, "UnitaryGate", seed=80)
    beta = 1.5

    def refused(eng, status, word, call):
        with pytest.raises(qoc.GrapeError) as ei:
            call()
        assert ei.value.status == status and word in str(ei.value), str(ei.value)

    with engine(qoc, w) as eng:
        eng.set_risk(beta)
        before = eng.eval(w.x)
        for bad in (np.nan, np.inf, -np.inf):
            refused(eng, -1, "beta", lambda: eng.set_risk(bad))
            after = eng.eval(w.x)
            assert after[0] == before[0] and np.array_equal(after[1], before[1])
        neg = w.wts.copy()
        neg[1] = -0.1
        refused(eng, -1, "weight", lambda: eng.set_operators(w.A, w.B, w.Xi, w.Xt, neg))
        refused(eng, -1, "weight", lambda: eng.set_operators(w.A, w.B, w.Xi, w.Xt, np.zeros(w.E)))
        after = eng.eval(w.x)
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
        R = np.broadcast_to(w.Xt, (1,) + w.Xt.shape)
        refused(eng, -2, "running cost", lambda: eng.set_running_cost(R, np.full(w.N, 0.1)))
        after = eng.eval(w.x)
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
        eng.set_running_cost(None)                           # switching off what is not on stays allowed
    with engine(qoc, w) as eng:                              # the other order: the running cost first
        eng.set_running_cost(np.broadcast_to(w.Xt, (1,) + w.Xt.shape), np.full(w.N, 0.1))
        before = eng.eval(w.x)
        refused(eng, -2, "running cost", lambda: eng.set_risk(beta))
        after = eng.eval(w.x)
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
        eng.set_risk(0.0)
    neg = w.wts.copy()
    neg[2] = -0.3
    with qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, neg, w.T, w.N) as eng:
        before = eng.eval(w.x)                               # (the mean takes any weights)
        refused(eng, -1, "weight", lambda: eng.set_risk(beta))
        after = eng.eval(w.x)
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    for kw, word in ((dict(devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM), "multi-device"),
                     (dict(force_collective=True, device=0), "communicator")):
        with engine(qoc, w, **kw) as eng:
            before = eng.eval(w.x)
            refused(eng, -2, word, lambda: eng.set_risk(beta))
            eng.set_risk(0.0)
            after = eng.eval(w.x)
            assert after[0] == before[0] and np.array_equal(after[1], before[1])
            refused(eng, -5, "risk", lambda: eng.risk_weights())


# ---- 9. optimisers --------------------------------------------------------------------------------------------------------
def test_lbfgs_matches_the_host_restatement_on_the_reference_objective(qoc, oracle):
    """grape_lbfgs(line_search = 1) under beta = 4 on the 2 x 2 StateTransfer ensemble of the reference's testsets (E = 5,
    N = 10), three iterations, against oracle/optim_lbfgs.py driven by the REFERENCE objective (risk_reference.py: no device
    result): accepted step length to 1e-6, iterate to 1e-9, evaluations equal -- the bars of
    test_gpu_lbfgs.py::test_iterates_match_the_host_restatement"""
    from oracle import optim_lbfgs
    w = qoc.workloads.reference_ensemble("StateTransfer", 5, 10, 5.0)
    beta, n_it = 4.0, 3
    ref = optim_lbfgs.lbfgs(lambda x: rr.risk_reference(oracle, w, x, beta)[:2], w.x, iterations=n_it)
    tr = ref["trace"]
    assert len(tr) == n_it
    with engine(qoc, w) as eng:
        eng.set_risk(beta)
        xs, infos = [], []
        for k in range(1, n_it + 1):
            xk, info = eng.lbfgs(w.x, iterations=k, line_search="optim")
            xs.append(xk)
            infos.append(info)
        al, ev = eng.lbfgs_trace()
        F_end, G_end = eng.eval(xs[-1])
    assert len(al) == n_it
    per_dev = np.diff(np.concatenate([[1], ev]))
    per_ref = np.diff([1] + [t["evaluations"] for t in tr])
    for i in range(n_it):
        a_ref, x_ref = tr[i]["alpha"], tr[i]["x"].reshape(w.x.shape)
        print(f"iteration {i}: alpha {al[i]!r} vs {a_ref!r}, |dx| = {np.abs(xs[i] - x_ref).max():.3e}, evaluations "
              f"{per_dev[i]} vs {per_ref[i]}")
        assert abs(al[i] - a_ref) <= 1e-6 * abs(a_ref), (i, al[i], a_ref)
        assert np.abs(xs[i] - x_ref).max() <= 1e-9 * max(1.0, np.abs(x_ref).max()), i
        assert per_ref[i] <= 15 and per_dev[i] == per_ref[i], (i, list(per_dev), list(per_ref))
    # minimum and g_norm are those of F_beta
    F_ref, G_ref, _, _ = rr.risk_reference(oracle, w, xs[-1], beta)
    assert abs(infos[-1]["minimum"] - F_ref) <= 1e-10 and abs(infos[-1]["minimum"] - F_end) <= 1e-12
    assert abs(infos[-1]["g_norm"] - np.abs(G_ref).max()) <= 1e-9 * max(1.0, np.abs(G_ref).max())


@pytest.mark.parametrize("optimizer", ["host", "device"])
def test_solve_with_a_risk_lowers_the_worst_member(qoc, optimizer):
    """solve(prob, GRAPE(n_slices=10, risk=4.0)) against the mean-optimised pulse from the same start and the same iteration
    budget: max_k F_k is no larger.  Fixture: the reference's n_ens = 5 StateTransfer ensemble (state_transfer_tests.jl:42-68)
    at T = 5, five iterations, the device optimiser with line_search = "optim".  On the CPU reference (risk_reference.py
    driven by SciPy's L-BFGS-B for the host optimiser, by oracle/optim_lbfgs.py for the device one) this budget gives
    max_k F_k = 0.891 (mean) against 0.808 (risk) and 0.995 against 0.849; a budget of ten iterations does NOT show it for
    optim_lbfgs (0.8550 against 0.8557: the landscape is not convex), which is why five was chosen."""
    wl = qoc.workloads
    prob = qoc.Problem(B=[wl.Sx, wl.Sy], A=wl.Sz, Xi=wl.rho_init, Xt=wl.rho_fin, T=5.0, n_controls=2, guess=wl.controls(2, 10),
                       sys_type=qoc.StateTransfer())
    ens = qoc.EnsembleProblem(prob=prob, n_ens=5, A_g=lambda k: (k - 2.5) / 2.5 * wl.Sz * 5, B_g=lambda k: [wl.Sx, wl.Sy],
                              XiG=lambda k: prob.Xi, XtG=lambda k: wl.rho_fin if k % 2 else wl.rho_init, wts=np.ones(5) / 5)
    opts = {"iterations": 5, "line_search": "optim"}
    worst = {}
    for risk in (0.0, 4.0):
        sol = qoc.solve(ens, qoc.GRAPE(n_slices=10, risk=risk, optimizer=optimizer, optim_options=opts))
        _, member_F, F_mean = qoc.api.test_pulse(ens, sol)    # per-member values, whatever the risk
        worst[risk] = member_F.max()
        F_soft = rr.soft_max(member_F, np.ones(5) / 5, risk)[0]
        print(f"{optimizer} risk={risk}: minimum {sol.result.minimum!r}, max F_k {member_F.max()!r}, mean {F_mean!r}")
        assert abs(sol.result.minimum - F_soft) <= 1e-9       # res.minimum is F_beta of the returned pulse
    assert worst[4.0] <= worst[0.0]
