"""grape_set_running_cost on the GPU: running costs on the intermediate states (C5 / C6 / C7, src/cost_functions.jl:44-61)
against the NumPy / SciPy reference of tests/rc_reference.py (expm per slice, states by a loop, the first-order gradient from
the O(N^2) double sum) added to the oracle's first-order ensemble result, at the project's parity bar."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rc_reference as rcr  # noqa: E402
from conftest import assert_parity  # noqa: E402

pytestmark = pytest.mark.gpu

T = 1.5


def make_case(seed, n, m, N, E, K=2, hermitian=True, variant=0, J=1, rho_kind="random", T=T):
    """Operators of norm ~1 (dt |H| well inside the expm's unscaled range at the larger N), a target a perturbed-pulse
    propagation away, probes of order 1 and slice weights that add up to order 1.  (T = 24 at small N leaves that range.)"""
    rng = np.random.default_rng(seed)
    A, B, Xi, wts = rcr.random_problem(rng, n, m, K, E, hermitian=hermitian)
    x = rng.standard_normal((K, N))
    Xt = rcr.perturbed_target(A, B, Xi, x, T, rng, variant)     # (T: the argument)
    R = rng.standard_normal((J, E, n, m)) + 1j * rng.standard_normal((J, E, n, m))
    R[0] = Xt                                                 # (term 0: the C6 / C7 probe)
    rho = rng.uniform(0.5, 1.5, (J, N)) * min(1.0, 4.0 / N)   # total weight of order 1: J and F of the same size
    if rho_kind == "mixed":                                   # zeros and negative entries
        rho[:, ::3] = 0.0
        rho[:, 1::4] *= -1.0
    elif rho_kind == "single":                                # one non-zero slice: rho[s-1] <-> the state after s slices
        rho[:] = 0.0
        rho[:, (N - 1) // 2] = 1.7
    return dict(n=n, m=m, N=N, E=E, K=K, A=A, B=B, Xi=Xi, Xt=Xt, wts=wts, x=x, R=R, rho=rho, variant=variant, T=T)


_REF = {}


def reference(oracle, key, c, x=None):
    """(F, G, F_J, G_J) of the reference, computed once per case and shared"""
    if key not in _REF:
        xx = c["x"] if x is None else x
        F0, G0 = oracle.ensemble_eval("UnitaryGate", c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], xx, c["T"], c["variant"])
        FJ, GJ = rcr.running_cost_ref(c["A"], c["B"], c["Xi"], c["wts"], xx, c["T"], c["R"], c["rho"], c["variant"])
        for a in (G0, GJ):
            a.setflags(write=False)
        _REF[key] = (F0 + FJ, G0 + GJ, F0, G0, FJ, GJ)
    return _REF[key]


def visible(ref):
    """the term cannot hide under the tolerance: its gradient is at least 1e-3 of the whole"""
    _, G, _, _, _, GJ = ref
    assert np.abs(GJ).max() >= 1e-3 * np.abs(G).max(), (np.abs(GJ).max(), np.abs(G).max())


def engine(qoc, c, **kw):
    return qoc.GrapeEngine("UnitaryGate", c["A"], c["B"], c["Xi"], c["Xt"], c["wts"], c["T"], c["N"], variant=c["variant"], **kw)


# n, m, N, E, hermitian, variant, kernel, S, W, J, rho_kind
SHAPES = [
    (2, 2, 1, 1, True, 0, "lane", 0, 0, 1, "random"),        # a single slice
    (2, 1, 2, 3, False, 1, "pair", 0, 0, 3, "random"),       # fewer slices than lanes
    (2, 2, 130, 70, True, 1, "pair", 3, 2, 1, "mixed"),      # ragged on both sides of a wave, many members
    (2, 2, 333, 3, False, 0, "lane", 2, 3, 3, "mixed"),      # three waves per member
    (3, 3, 7, 70, True, 0, "lane", 3, 1, 1, "single"),       # forced S leaves most lanes without a slice
    (3, 1, 64, 3, False, 0, "lane", 1, 1, 3, "random"),      # exactly one wave of single-slice chunks
    (3, 3, 65, 3, False, 1, "lane", 2, 1, 3, "mixed"),
    (3, 2, 130, 1, True, 1, "lane", 1, 3, 1, "random"),
    (4, 4, 65, 3, True, 1, "pair", 1, 3, 1, "random"),       # 65 single-slice chunks over three waves of 32
    (4, 2, 130, 1, False, 0, "pair", 2, 3, 3, "mixed"),
    (4, 1, 64, 3, False, 0, "pair", 0, 0, 3, "random"),      # n x 1 under a non-Hermitian generator: the pair kernel's vector sweep
    (4, 1, 333, 3, True, 0, "lane", 0, 0, 1, "single"),
    (4, 4, 333, 1, False, 1, "lane", 3, 2, 3, "random"),
    (4, 4, 7, 70, True, 0, "pair", 2, 1, 1, "mixed"),
    (4, 3, 64, 3, True, 0, "lane", 0, 0, 3, "random"),
]


@pytest.mark.parametrize("n,m,N,E,herm,variant,kernel,S,W,J,rho_kind", SHAPES)
def test_parity_against_the_double_sum_reference(qoc, oracle, monkeypatch, n, m, N, E, herm, variant, kernel, S, W, J, rho_kind):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant, J=J, rho_kind=rho_kind)
    ref = reference(oracle, ("shape", n, m, N, E, herm, variant, J, rho_kind), c)
    visible(ref)
    with engine(qoc, c, slices_per_lane=S, waves_per_member=W) as eng:
        assert eng.info["unitary_flow"] == (1 if herm else 0) and eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
        eng.set_running_cost(c["R"], c["rho"])
        F, G = eng.eval(c["x"])
        names = eng.kernel_names()
        F2, G2 = eng.eval(c["x"])
    print(f"n={n} m={m} N={N} E={E}: |dF|={abs(F - ref[0]):.2e} relG={np.abs(G - ref[1]).max() / np.abs(ref[1]).max():.2e}")
    assert "running_cost_kernel" in names and "running_cost_fold_kernel" in names
    assert_parity(F, G, ref[0], ref[1], n, what=f"n={n} m={m} N={N} E={E}")
    assert F2 == F and np.array_equal(G2, G)                  # bitwise reproducible call to call


def c5_case():
    """a qutrit held as a ket, level 2 forbidden"""
    c = make_case(7, 3, 1, 40, 1, J=1)
    c["Xi"] = np.array([[[1.0], [0.0], [0.0]]], complex)
    c["Xt"] = np.array([[[0.0], [1.0], [0.0]]], complex)
    c["R"] = np.array([[[[0.0], [0.0], [1.0]]]], complex)
    c["rho"] = np.full((1, 40), 0.8)
    return c


def c6_case():
    c = make_case(8, 4, 4, 30, 2, J=1)
    c["rho"] = np.full((1, 30), -1.5 / (30 * 16))
    return c


def c7_case():
    c = make_case(9, 4, 1, 30, 1, J=1)
    c["rho"] = np.full((1, 30), -1.5 / 30)
    return c


def as_problem(qoc, c):
    base = qoc.Problem(B=list(c["B"][0]), A=c["A"][0], Xi=c["Xi"][0], Xt=c["Xt"][0], T=T, n_controls=c["K"], guess=c["x"],
                       sys_type=qoc.UnitaryGate())
    if c["E"] == 1:
        return base
    return qoc.EnsembleProblem(base, c["E"], lambda k: c["A"][k - 1], lambda k: list(c["B"][k - 1]), lambda k: c["Xi"][k - 1],
                               lambda k: c["Xt"][k - 1], c["wts"])


@pytest.mark.parametrize("which", ["C5", "C6", "C7"])
def test_instances_raw_and_through_descriptors(qoc, oracle, which):
    c = {"C5": c5_case, "C6": c6_case, "C7": c7_case}[which]()
    desc = {"C5": qoc.ForbiddenStates([[0, 0, 1.0]], 0.8), "C6": qoc.EvolutionTime(1.5), "C7": qoc.EvolutionTime(1.5)}[which]
    ref = reference(oracle, ("instance", which), c)
    visible(ref)
    with engine(qoc, c) as eng:
        eng.set_running_cost(c["R"], c["rho"])
        F, G = eng.eval(c["x"])
    assert_parity(F, G, ref[0], ref[1], c["n"], what=which + " raw")
    prob = as_problem(qoc, c)
    if c["E"] == 1:
        c["wts"] = np.ones(1)                                 # (a plain Problem carries weight 1)
        ref = reference(oracle, ("instance1", which), c)
    eng = qoc.api.make_engine(prob, qoc.GRAPE(n_slices=c["N"], running_costs=[desc]))
    try:
        Fd, Gd = eng.eval(c["x"])
        const = eng.running_cost_constant
    finally:
        eng.close()
    assert const == (0.0 if which == "C5" else 1.5 * float(np.sum(c["wts"])))
    assert_parity(Fd, Gd, ref[0], ref[1], c["n"], what=which + " descriptor")
    # the value is weight x the host functional of the trajectory
    X = rcr.states(rcr.propagators(c["A"], c["B"], c["x"], T, c["variant"]), c["Xi"])[1:]
    if which == "C5":
        want = 0.8 * qoc.C5([0, 0, 1.0], X[:, 0])
    elif which == "C6":
        want = sum(c["wts"][k] * 1.5 * qoc.C6(c["Xt"][k], X[:, k], c["N"], 4) for k in range(c["E"]))
    else:
        want = 1.5 * (1 - sum(abs(np.vdot(c["Xt"][0], v)) ** 2 for v in X[:, 0]) / c["N"])
    assert ref[4] + const == pytest.approx(want, rel=1e-12)


def leakage(c, x):
    X = rcr.states(rcr.propagators(c["A"], c["B"], x, T, 0), c["Xi"])[1:, 0]
    return float(np.sum(np.abs(X[:, 2, 0]) ** 2))


@pytest.mark.parametrize("optimizer", ["host", "device"])
def test_solve_with_forbidden_states_lowers_the_occupation(qoc, optimizer):
    c = c5_case()
    prob = as_problem(qoc, c)
    opts = {"iterations": 60}
    plain = qoc.solve(prob, qoc.GRAPE(n_slices=c["N"], optimizer=optimizer, optim_options=opts))
    pen = qoc.solve(prob, qoc.GRAPE(n_slices=c["N"], optimizer=optimizer, optim_options=opts,
                                    running_costs=[qoc.ForbiddenStates([[0, 0, 1.0]], 0.8)]))
    l0, l1 = leakage(c, plain.opti_pulses), leakage(c, pen.opti_pulses)
    print(f"{optimizer}: forbidden-level occupation summed over the slices {l0:.4f} -> {l1:.4f}")
    assert l1 < l0


def test_composition_with_penalties_and_basis(qoc, oracle):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_penalties_host import penalty_ref
    c = make_case(21, 4, 4, 50, 3, J=3, rho_kind="mixed")
    rng = np.random.default_rng(4)
    M = 6
    phi = rng.standard_normal((c["N"], M))
    x0 = 0.2 * rng.standard_normal((c["K"], c["N"]))
    theta = 0.3 * rng.standard_normal((c["K"], M))
    x = x0 + theta @ phi.T
    amp, var = np.array([0.3, 0.0]), np.array([0.1, 0.2])
    ref = reference(oracle, ("compose",), c, x=x)
    visible(ref)
    Fp, Gp = penalty_ref(x, amp, var)
    with engine(qoc, c) as eng:
        eng.set_running_cost(c["R"], c["rho"])
        eng.set_penalties(amp, var)
        eng.set_basis(phi, x0)
        F, G = eng.eval(theta)
    assert_parity(F, G, ref[0] + Fp, (ref[1] + Gp) @ phi, c["n"], what="running cost + penalties + basis")


def test_entry_points_agree_bitwise(qoc, oracle, monkeypatch):
    import torch
    c = make_case(31, 4, 4, 70, 5, J=3, rho_kind="mixed")
    rng = np.random.default_rng(6)
    Xs = np.array([c["x"], c["x"] + 0.1 * rng.standard_normal(c["x"].shape), -c["x"]])
    with engine(qoc, c, max_batch=3) as eng:
        eng.set_running_cost(c["R"], c["rho"])
        single = [eng.eval(x) for x in Xs]
        Fb, Gb = eng.eval_batch(Xs)
        for b in range(3):
            assert Fb[b] == single[b][0] and np.array_equal(Gb[b], single[b][1])
            assert eng.fom(Xs[b]) == single[b][0]
        assert np.array_equal(eng.fom(Xs), Fb)
        d_x = torch.tensor(np.ascontiguousarray(Xs[1].T), device="cuda")
        d_fg = torch.zeros(c["K"] * c["N"] + 1, dtype=torch.float64, device="cuda")
        eng.eval_device(d_x.data_ptr(), d_fg.data_ptr())
        torch.cuda.synchronize()
        fg = d_fg.cpu().numpy()
        assert fg[-1] == single[1][0] and np.array_equal(fg[:-1].reshape(c["N"], c["K"]).T, single[1][1])
    ref = reference(oracle, ("entry",), c)
    assert_parity(single[0][0], single[0][1], ref[0], ref[1], c["n"], what="batch case")


def test_member_chunked_context_is_bitwise_the_unchunked_one(qoc, monkeypatch):
    c = make_case(41, 3, 3, 40, 10, hermitian=False, J=3)
    with engine(qoc, c) as eng:
        eng.set_running_cost(c["R"], c["rho"])
        F, G = eng.eval(c["x"])
        info = eng.info
    # room for four and a half members' propagators and prefix products (general flow, lane kernel: 64 W chunks of S slices)
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(int(4.5 * 2 * info["slices_per_lane"] * 64 * info["waves_per_member"] * 9 * 16)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < c["E"], eng.info["member_chunk"]
        eng.set_running_cost(c["R"], c["rho"])
        Fc, Gc = eng.eval(c["x"])
    assert Fc == F and np.array_equal(Gc, G)


def test_off_means_off(qoc):
    c = make_case(51, 4, 4, 33, 1, J=1)
    with engine(qoc, c, member_results=True) as eng:
        F0, G0 = eng.eval(c["x"])
        names0 = eng.kernel_names()
        mem0 = eng.member_results()
        eng.set_running_cost(c["R"], c["rho"])
        F1, G1 = eng.eval(c["x"])
        mem1 = eng.member_results()
        assert F1 != F0 and "running_cost_kernel" in eng.kernel_names()
        assert np.array_equal(mem0[0], mem1[0]) and np.array_equal(mem0[1], mem1[1])     # member rows stay without J
        eng.set_running_cost(None)
        F2, G2 = eng.eval(c["x"])
        assert eng.kernel_names() == names0 and "running_cost_kernel" not in names0
        assert F2 == F0 and np.array_equal(G2, G0)
        # it persists across grape_set_operators
        eng.set_running_cost(c["R"], c["rho"])
        eng.set_operators(c["A"], c["B"], c["Xi"], c["Xt"], c["wts"])
        F3, G3 = eng.eval(c["x"])
        assert F3 == F1 and np.array_equal(G3, G1)


def test_refusals_keep_the_previous_setting(qoc):
    c = make_case(61, 4, 4, 20, 2, J=1)
    GE = qoc.GrapeError

    def refused(eng, status, word, R=None, rho=None):
        with pytest.raises(GE) as ei:
            eng.set_running_cost(c["R"] if R is None else R, c["rho"] if rho is None else rho)
        assert ei.value.status == status and word in str(ei.value), str(ei.value)

    with engine(qoc, c) as eng:
        eng.set_running_cost(c["R"], c["rho"])
        F1, G1 = eng.eval(c["x"])
        bad = c["R"].copy()
        bad[0, 1, 2, 3] = np.nan
        refused(eng, -1, "not finite", R=bad)
        bad_rho = c["rho"].copy()
        bad_rho[0, 3] = np.inf
        refused(eng, -1, "not finite", rho=bad_rho)
        lib = qoc.load_library()
        buf = np.ones(2 * 16 * 2 * 5)
        for nt in (-1, 5):
            assert lib.grape_set_running_cost(eng._h, nt, buf.ctypes.data, buf.ctypes.data) == -1
            assert b"n_terms" in lib.grape_last_error(eng._h)
        F2, G2 = eng.eval(c["x"])
        assert F2 == F1 and np.array_equal(G2, G1)            # the previous setting stayed in force
        with pytest.raises(GE) as ei:                         # attaching an exchange behind a running cost
            eng.ipc_attach([eng.ipc_export(1)], 0, 1)
        assert ei.value.status == -2 and "running cost" in str(ei.value)
        with pytest.raises(GE) as ei:
            eng.comm_attach(bytes(128), 0, 1)
        assert ei.value.status == -2 and "running cost" in str(ei.value)
    st = make_case(62, 4, 4, 20, 2)
    with qoc.GrapeEngine("StateTransfer", st["A"], st["B"], st["Xi"], st["Xt"], st["wts"], T, 20) as eng:
        refused(eng, -2, "StateTransfer", R=st["R"], rho=st["rho"])
    with engine(qoc, c, gradient="exact") as eng:
        refused(eng, -2, "exact")
    with engine(qoc, c, gradient="exact", objective="c1") as eng:
        refused(eng, -2, "exact")
    with engine(qoc, c, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM) as eng:
        refused(eng, -2, "multi-device")
    with engine(qoc, c, force_collective=True) as eng:        # a communicator is attached (one rank)
        refused(eng, -2, "communicator")
    big = make_case(63, 5, 5, 8, 1)
    with qoc.GrapeEngine("UnitaryGate", big["A"], big["B"], big["Xi"], big["Xt"], big["wts"], T, 8) as eng:
        refused(eng, -2, "dimension", R=big["R"], rho=big["rho"])


# ---- the edges a standing running cost has to survive ---------------------------------------------------------------------
import settings_sequences as ss  # noqa: E402


def with_operators(c, o):
    """case c (pulse, probes, weights) on the operators of case o"""
    return dict(c, **{k: o[k] for k in ("A", "B", "Xi", "Xt", "wts")})


@pytest.mark.parametrize("start_hermitian", [True, False])
@pytest.mark.parametrize("n,m,kernel", [(3, 3, "lane"), (4, 4, "lane"), (4, 2, "pair")])
def test_flow_switch_under_a_standing_cost(qoc, oracle, monkeypatch, n, m, kernel, start_hermitian):
    """The general flow's state scratch does not exist while the generators are Hermitian, and rc_ensure sizes it at the first
    evaluation that needs it: the cost is set once, the operators change the flow under it and change it back."""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    first = make_case(700 + 10 * n + m, n, m, 65, 3, hermitian=start_hermitian, J=3, rho_kind="mixed")
    other = with_operators(first, make_case(800 + 10 * n + m, n, m, 65, 3, hermitian=not start_hermitian, J=3))
    refs = [reference(oracle, ("switch", n, m, start_hermitian, i), c) for i, c in enumerate((first, other))]
    for r in refs:
        visible(r)
    with engine(qoc, first) as eng:
        eng.set_running_cost(first["R"], first["rho"])
        res = []
        for c in (first, other, first):
            if res:
                eng.set_operators(c["A"], c["B"], c["Xi"], c["Xt"], c["wts"])
            res.append(eng.eval(c["x"]))
            assert eng.info["unitary_flow"] == (1 if (c is first) == start_hermitian else 0)
            assert eng.info["lane_pair"] == (1 if kernel == "pair" else 0)
            assert "running_cost_kernel" in eng.kernel_names()
    for i, (F, G) in enumerate(res):
        assert_parity(F, G, refs[i % 2][0], refs[i % 2][1], n, what=f"n={n} {kernel} evaluation {i}")
    assert res[2][0] == res[0][0] and np.array_equal(res[2][1], res[0][1])           # back on the first operators: bit for bit


def _chunk_budget(c, info, hermitian, members):
    """room for `members` and a half members' workspace: the propagators, and the states beside them in the general flow"""
    chunks = 64 * info["waves_per_member"] // (2 if info["lane_pair"] else 1)
    return int((members + 0.5) * (1 if hermitian else 2) * info["slices_per_lane"] * chunks * c["n"] ** 2 * 16)


@pytest.mark.parametrize("hermitian,m,chunked", [(False, 4, False), (False, 1, False), (False, 4, True), (False, 1, True),
                                                 (True, 4, True)])
def test_batches_on_the_general_flow_and_on_member_chunks(qoc, oracle, monkeypatch, hermitian, m, chunked):
    """running_cost_kernel's workgroup index runs over (control array, member): workspace, scratch and rows go by it, the
    probes by the member alone.  A member-chunked context (two members at a time, the last chunk short) walks a batch array by
    array and addresses the probes from the chunk's first member on."""
    c = make_case(900 + m + 10 * hermitian, 4, m, 70, 5, hermitian=hermitian, J=3, rho_kind="mixed")
    rng = np.random.default_rng(7)
    Xs = np.array([c["x"], c["x"] + 0.1 * rng.standard_normal(c["x"].shape), -c["x"]])
    refs = [reference(oracle, ("batch", hermitian, m, b), c, x=Xs[b]) for b in range(3)]
    for r in refs:
        visible(r)
    if chunked:
        with engine(qoc, c, max_batch=3) as eng:
            info = eng.info
        monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, hermitian, 2)))
    with engine(qoc, c, max_batch=3) as eng:
        assert eng.info["member_chunk"] == (2 if chunked else 5) and eng.info["unitary_flow"] == (1 if hermitian else 0)
        eng.set_running_cost(c["R"], c["rho"])
        single = [eng.eval(x) for x in Xs]
        Fb, Gb = eng.eval_batch(Xs)
        F2, G2 = eng.eval_batch(Xs[1:])
    for b in range(3):
        assert Fb[b] == single[b][0] and np.array_equal(Gb[b], single[b][1]), b
        assert_parity(Fb[b], Gb[b], refs[b][0], refs[b][1], 4, what=f"hermitian={hermitian} m={m} chunked={chunked} entry {b}")
    assert np.array_equal(F2, Fb[1:]) and np.array_equal(G2, Gb[1:])


@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("K,J", [(1, 4), (5, 2), (5, 4)])
def test_k_and_j_at_their_ends(qoc, oracle, K, J, n, hermitian):
    c = make_case(1000 + 100 * K + 10 * J + n, n, n, 20, 3, K=K, hermitian=hermitian, J=J)
    ref = reference(oracle, ("ends", K, J, n, hermitian), c)
    visible(ref)
    with engine(qoc, c) as eng:
        eng.set_running_cost(c["R"], c["rho"])
        F, G = eng.eval(c["x"])
    assert G.shape == (K, 20)
    assert_parity(F, G, ref[0], ref[1], n, what=f"K={K} J={J} n={n} hermitian={hermitian}")


@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("n,kernel", [(4, "pair"), (3, "lane")])
@pytest.mark.parametrize("T_case,squarings", [(24.0, -1), (1.5, 3)])
def test_propagators_from_the_squaring_branch(qoc, oracle, monkeypatch, T_case, squarings, n, kernel, hermitian):
    """The kernel reads what the sweep's expm stored: here exp(-i dt H) with dt |H|_1 of 20 to 40 (T = 24 over 8 slices), where
    the expm scales and squares, and with three forced squarings at T = 1.5.  The reference's propagators are SciPy's expm;
    on the CPU the oracle's expm and SciPy's agree on these very generators to 2.0e-15 (n = 3, 4, both flows, T = 24) and
    5.8e-16 (T = 1.5) relative to the largest entry, five orders below the bar.
    The forced case has 48 slices: dt |H|_1 <= 0.64 = 2^3 x 0.08, the norm up to which the expm itself would stop at three
    squarings.  Forcing FEWER squarings than the norm asks for is the caller's trade of accuracy for time, not this kernel's
    business: at 8 slices (dt |H|_1 = 1.9, scaled 0.24) the degree-8 polynomial's truncation 0.24^9 / 9! = 7e-12 per
    propagator, doubled by each squaring, showed as 3.9e-10 of max |G| on the n = 4 Hermitian case."""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(1100 + n + int(T_case), n, n, 8 if squarings < 0 else 48, 3, hermitian=hermitian, J=3, T=T_case)
    ref = reference(oracle, ("squarings", T_case, n, hermitian), c)
    visible(ref)
    with engine(qoc, c, expm_squarings=squarings) as eng:
        eng.set_running_cost(c["R"], c["rho"])
        F, G = eng.eval(c["x"])
        assert eng.info["unitary_flow"] == (1 if hermitian else 0)
    print(f"T={T_case} s={squarings} n={n} hermitian={hermitian}: |dF|={abs(F - ref[0]):.2e} "
          f"relG={np.abs(G - ref[1]).max() / np.abs(ref[1]).max():.2e}")
    assert_parity(F, G, ref[0], ref[1], n, what=f"T={T_case} squarings={squarings} n={n} hermitian={hermitian}")


@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("n,m,kernel", [(4, 4, "pair"), (3, 2, "lane")])
def test_debug_flow_with_a_running_cost(qoc, oracle, monkeypatch, n, m, kernel, hermitian):
    """GRAPE_FLAG_KEEP_COSTATES: the sweep stores every costate beside the states (the general data flow whatever the
    generators are), and the running cost reads the propagators of that sweep like those of any other."""
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c = make_case(1200 + n, n, m, 33, 3, hermitian=hermitian, J=2)
    ref = reference(oracle, ("debug", n, hermitian), c)
    visible(ref)
    with engine(qoc, c, flags=qoc.engine.FLAG_KEEP_COSTATES) as eng:
        assert eng.info["unitary_flow"] == 0
        eng.set_running_cost(c["R"], c["rho"])
        F, G = eng.eval(c["x"])
        assert "running_cost_kernel" in eng.kernel_names()
        L = eng.trajectory(1, costates=True)[2]              # the costates it is there for: those of F alone
    assert_parity(F, G, ref[0], ref[1], n, what=f"debug flow n={n} hermitian={hermitian}")
    assert L.shape == (34, n, m) and np.array_equal(L[-1], c["Xt"][1])


@pytest.mark.parametrize("case", ["running_cost_alone", "running_cost_penalties_basis"])
def test_lbfgs_iterates_match_the_host_restatement_under_a_running_cost(qoc, oracle, case):
    """grape_lbfgs(line_search = "optim") against oracle/optim_lbfgs.py driven with the composed REFERENCE (oracle + penalty_ref
    + the double sum, the basis in NumPy): the line search's probes close through the fold kernel and the reduce (slice mode)
    or the projection (parameter mode).  Ten iterations, at least eight compared.
    UnitaryGate's F is Re(z^2) while its gradient is that of -|z|^2: where the two disagree the
    approximate Wolfe test is never met, Hager-Zhang bisects down to eps(b) and the comparison loop ends (as in
    tests/test_gpu_lbfgs.py).  So both cases start where the REFERENCE's own trace, computed on the CPU from the reference
    alone, is ten regular line searches -- evaluations per iteration 2, 4, 3, 3, 3, 3, 4, 3, 3, 3 for the qutrit ket of
    c5_case from -x (F from 2.94 to -0.26), 3, 2, 2, 3, 2, 2, 4, 2, 2, 3 for the gate (static variant) -- and all ten
    iterations are compared.  (From +x the qutrit's reference bisects in its second iteration, 64 evaluations: two
    iterations compared, on which an MI355X agreed to 3.6e-10 in the step length and 3.6e-15 in the iterate.)"""
    from oracle import optim_lbfgs
    if case == "running_cost_alone":
        c, pen, phi = c5_case(), None, None
        start = -np.array(c["x"])
    else:
        c = make_case(1301, 4, 4, 25, 3, J=2, rho_kind="mixed", variant=1)
        pen = dict(amp=np.array([0.3, 0.1]), var=np.array([0.05, 0.2]))
        phi = qoc.fourier_basis(c["N"], c["T"], 2 * np.pi / c["T"] * np.array([0.5, 1.0]))
        assert phi.shape == (c["N"], 4)
        start = np.zeros((c["K"], 4))

    def composed(th):
        x = th if phi is None else c["x"] + th @ phi.T
        F, G, _ = ss.composed_reference(oracle, c, x, c["T"], c["variant"], pen, dict(R=c["R"], rho=c["rho"]))
        return F, (G if phi is None else G @ phi)

    F0, G0 = composed(start)
    ref = optim_lbfgs.lbfgs(composed, start, iterations=10)
    with engine(qoc, c) as eng:
        eng.set_running_cost(c["R"], c["rho"])
        if pen:
            eng.set_penalties(pen["amp"], pen["var"])
        if phi is not None:
            eng.set_basis(phi, c["x"])
        F, G = eng.eval(start)
        assert_parity(F, G, F0, G0, c["n"], what=case)
        ss.compare_lbfgs_iterates(eng, ref, start, 10, case, min_compared=8)
