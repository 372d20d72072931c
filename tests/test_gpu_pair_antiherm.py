"""GPU: the lane-pair kernel's unitary UnitaryGate flow with the backward sweep on the anti-Hermitian part of z M_t alone
(sweep_pair.hip, PMODE_UNITARY_AH).  tr M_t does not depend on t (the P_t are unitary), so z is one number per
member, and Re tr(B'_c z M_t) sees only A_t = (z M_t - conj(z) M_t') / 2, which conjugation by P_t keeps anti-Hermitian: the
sweep carries one triangle of A_t.  Held per member to the C oracle at the project's 1e-10 bar and to the full-M sweep
(GRAPE_PAIR_AH=0, a fresh engine) at 1e-12 of max(1, .) -- the bar tests/test_gpu_pair_vec.py sets for two FP64 orders of the
same sums.  Dense random Hermitian A (different per member) and B_c (not Pauli), random unitary Xi, Xt; E = 5 is no multiple
of the 4 members of a workgroup, N = 37 leaves ragged chunks, K = 3 an odd control count.  grape_info.pair_antiherm says which
sweep a context takes; the exact gradient (it needs the full M_t) and n = 2 keep the old one."""
import numpy as np
import pytest

from conftest import assert_parity

pytestmark = pytest.mark.gpu
T = 1.3


def _unitary(rng, n):
    return np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0]


def _problem(E, N, K, seed, n=4):
    rng = np.random.default_rng(seed)

    def herm():
        M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        return (M + M.conj().T) / 2
    A = np.array([herm() for _ in range(E)]) * 0.7
    B = np.array([[herm() for _ in range(K)] for _ in range(E)]) * 0.5
    Xi = np.array([_unitary(rng, n) for _ in range(E)])
    Xt = np.array([_unitary(rng, n) for _ in range(E)])
    wts = rng.uniform(0.2, 1.0, E)
    x = rng.uniform(-1, 1, (K, N))
    return A, B, Xi, Xt, wts, x


def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


def _both(qoc, monkeypatch, run, **kw):
    """run(eng) on a fresh engine per sweep: {"antiherm": ..., "full": ...}; the path each took is asserted here"""
    out = {}
    for tag, env in (("antiherm", None), ("full", "0")):
        if env is None:
            monkeypatch.delenv("GRAPE_PAIR_AH", raising=False)
        else:
            monkeypatch.setenv("GRAPE_PAIR_AH", env)
        with qoc.GrapeEngine(*kw["ops"], T, kw["N"], **kw.get("engine", {})) as eng:
            out[tag] = run(eng)
            info = eng.info
            assert "sweep_pair_kernel" in eng.kernel_names(), eng.kernel_names()
        assert info["lane_pair"] == 1 and info["unitary_flow"] == 1, info
        assert info["pair_antiherm"] == (1 if tag == "antiherm" else 0), (tag, info)
    monkeypatch.delenv("GRAPE_PAIR_AH", raising=False)
    return out


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("N", [37, 130])
def test_antihermitian_sweep_matches_oracle_and_full_sweep_per_member(qoc, oracle, monkeypatch, N, K, variant):
    E = 5
    A, B, Xi, Xt, wts, x = _problem(E, N, K, seed=100 * N + 10 * K + variant)
    F_ref, G_ref, foms_ref, grads_ref = oracle.ensemble_eval("UnitaryGate", A, B, Xi, Xt, wts, x, T, variant=variant, per_member=True)

    def run(eng):
        F, G = eng.eval(x)
        foms, grads = eng.member_results()
        F2, G2 = eng.eval(x)
        assert F == F2 and np.array_equal(G, G2)             # bitwise reproducible
        return F, G, np.array(foms), np.array(grads)
    res = _both(qoc, monkeypatch, run, ops=("UnitaryGate", A, B, Xi, Xt, wts), N=N,
                engine=dict(variant=variant, member_results=True))
    for tag, (F, G, foms, grads) in res.items():
        assert_parity(F, G, F_ref, G_ref, 4, what=tag)
        for m in range(E):
            assert_parity(foms[m], grads[m], foms_ref[m], grads_ref[m], 4, what=f"{tag} member {m}")
    for a, b in zip(res["antiherm"], res["full"]):
        assert _close(a, b), np.abs(np.asarray(a) - np.asarray(b)).max()


def test_antihermitian_sweep_batch_of_three_control_arrays(qoc, oracle, monkeypatch):
    E, N, K = 5, 37, 3
    A, B, Xi, Xt, wts, x = _problem(E, N, K, seed=7)
    xs = np.stack([x, 0.5 * x, -0.3 * x])
    refs = [oracle.ensemble_eval("UnitaryGate", A, B, Xi, Xt, wts, xb, T) for xb in xs]

    def run(eng):
        Fb, Gb = eng.eval_batch(xs)
        F1, G1 = eng.eval(xs[1])
        assert Fb[1] == F1 and np.array_equal(Gb[1], G1)
        return np.array(Fb), np.array(Gb)
    res = _both(qoc, monkeypatch, run, ops=("UnitaryGate", A, B, Xi, Xt, wts), N=N, engine=dict(max_batch=3))
    for tag, (Fb, Gb) in res.items():
        for i, (F_ref, G_ref) in enumerate(refs):
            assert_parity(Fb[i], Gb[i], F_ref, G_ref, 4, what=f"{tag} array {i}")
    assert _close(res["antiherm"][0], res["full"][0]) and _close(res["antiherm"][1], res["full"][1])


@pytest.mark.parametrize("E", [3, 5])
def test_antihermitian_sweep_with_penalties_takes_the_reduce_path(qoc, oracle, monkeypatch, E):
    """E = 3 fits one workgroup, whose sweep publishes [G, F] itself -- unless penalties are on: the reduce kernel adds them."""
    from test_gpu_penalties import penalty_ref
    N, K = 37, 4
    A, B, Xi, Xt, wts, x = _problem(E, N, K, seed=11 + E)
    amp, var = np.linspace(0.3, 0.9, K), np.linspace(0.8, 0.2, K)
    F_ref, G_ref = oracle.ensemble_eval("UnitaryGate", A, B, Xi, Xt, wts, x, T)
    Fp, Gp = penalty_ref(x, amp, var)

    def run(eng):
        eng.set_penalties(amp, var)
        F, G = eng.eval(x)
        assert any(k.startswith("reduce_rows") for k in eng.kernel_names()), eng.kernel_names()
        return F, G
    res = _both(qoc, monkeypatch, run, ops=("UnitaryGate", A, B, Xi, Xt, wts), N=N)
    for tag, (F, G) in res.items():
        assert_parity(F, G, F_ref + Fp, G_ref + Gp, 4, what=tag)
    assert _close(res["antiherm"][0], res["full"][0]) and _close(res["antiherm"][1], res["full"][1])


def test_one_triangle_off_by_an_ulp_still_takes_the_unitary_flow(qoc, oracle, monkeypatch):
    """B_c Hermitian only to rounding: the upper triangle of every control moved by one ulp.  The gradient image is built from
    (B' - B'^H) / 2, so both triangles enter alike.  E = 3: one workgroup, direct publication."""
    E, N, K = 3, 37, 3
    A, B, Xi, Xt, wts, x = _problem(E, N, K, seed=23)
    iu = np.triu_indices(4, 1)
    for k in range(E):
        for c in range(K):
            B[k, c].real[iu] = np.nextafter(B[k, c].real[iu], np.inf)
            B[k, c].imag[iu] = np.nextafter(B[k, c].imag[iu], -np.inf)
    assert not np.array_equal(B, np.conj(np.swapaxes(B, -1, -2)))
    F_ref, G_ref, foms_ref, grads_ref = oracle.ensemble_eval("UnitaryGate", A, B, Xi, Xt, wts, x, T, per_member=True)

    def run(eng):
        F, G = eng.eval(x)
        foms, grads = eng.member_results()
        return F, G, np.array(foms), np.array(grads)
    res = _both(qoc, monkeypatch, run, ops=("UnitaryGate", A, B, Xi, Xt, wts), N=N, engine=dict(member_results=True))
    for tag, (F, G, foms, grads) in res.items():
        assert_parity(F, G, F_ref, G_ref, 4, what=tag)
        for m in range(E):
            assert_parity(foms[m], grads[m], foms_ref[m], grads_ref[m], 4, what=f"{tag} member {m}")
    for a, b in zip(res["antiherm"], res["full"]):
        assert _close(a, b)


def test_exact_gradient_keeps_the_full_sweep(qoc, oracle, monkeypatch):
    """gradient="exact" dumps W_t = M_t P_t' from the full M_t (the DUMPW instantiation of the kernel)."""
    monkeypatch.delenv("GRAPE_PAIR_AH", raising=False)
    E, N, K = 5, 37, 3
    A, B, Xi, Xt, wts, x = _problem(E, N, K, seed=31)
    F_ref, G_ref = oracle.ensemble_exact("UnitaryGate", A, B, Xi, Xt, wts, x, T)[:2]
    with qoc.GrapeEngine("UnitaryGate", A, B, Xi, Xt, wts, T, N, gradient="exact") as eng:
        F, G = eng.eval(x)
        info = eng.info
        assert "sweep_pair_kernel" in eng.kernel_names(), eng.kernel_names()
    assert info["lane_pair"] == 1 and info["unitary_flow"] == 1 and info["pair_antiherm"] == 0, info
    assert_parity(F, G, F_ref, G_ref, 4, what="exact")


def test_two_by_two_pairs_keep_the_full_sweep(qoc, oracle, monkeypatch):
    """n = 2 on lane pairs (GRAPE_SMALL_KERNEL=pair) stays on PMODE_UNITARY: the new routines serve n = 4."""
    monkeypatch.delenv("GRAPE_PAIR_AH", raising=False)
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", "pair")
    E, N, K = 5, 37, 3
    A, B, Xi, Xt, wts, x = _problem(E, N, K, seed=41, n=2)
    F_ref, G_ref, foms_ref, grads_ref = oracle.ensemble_eval("UnitaryGate", A, B, Xi, Xt, wts, x, T, per_member=True)
    with qoc.GrapeEngine("UnitaryGate", A, B, Xi, Xt, wts, T, N, member_results=True) as eng:
        F, G = eng.eval(x)
        foms, grads = eng.member_results()
        info = eng.info
        assert "sweep_pair_kernel" in eng.kernel_names(), eng.kernel_names()
    assert info["lane_pair"] == 1 and info["unitary_flow"] == 1 and info["pair_antiherm"] == 0, info
    assert_parity(F, G, F_ref, G_ref, 2, what="n = 2")
    for m in range(E):
        assert_parity(foms[m], grads[m], foms_ref[m], grads_ref[m], 2, what=f"n = 2 member {m}")
