"""GPU: grape_info.workspace_bytes across grape_set_operators uploads that change the data flow on one context.  The device
buffers only ever grow, so once every flow of a cycle has been seen the figure depends on the flow alone: a double count or a
lost subtraction in the host layer's buffer bookkeeping shows up as a drift from one cycle to the next.  Every evaluation in
between is held to the oracle at the 1e-10 bar."""
import numpy as np
import pytest

from conftest import assert_parity

pytestmark = pytest.mark.gpu

E, N, K, T = 2, 16, 2, 1.1
UPLOADS = 6                                               # flows a, b, a, b, a, b: three cycles


def _gen(rng, n, herm, scale):
    M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return ((M + M.conj().T) / 2 if herm else M) * scale


def _cycle(qoc, make_engine, problems, reference, n, expect):
    """uploads problems[0], [1], [0], ... on one context; returns workspace_bytes after every upload"""
    refs = [reference(p) for p in problems]               # the oracle, once per operator set
    sizes = []
    A, B, Xi, Xt, wts, x = problems[0]
    with make_engine(A, B, Xi, Xt, wts) as eng:
        for u in range(UPLOADS):
            A, B, Xi, Xt, wts, x = problems[u % 2]
            if u:
                eng.set_operators(A, B, Xi, Xt, wts)
            info = eng.info
            expect(info, u % 2)
            sizes.append(info["workspace_bytes"])
            F, G = eng.eval(x)
            assert_parity(F, G, *refs[u % 2], n, what=f"upload {u}")
            assert eng.info["workspace_bytes"] == sizes[-1], "an evaluation changed workspace_bytes"
    print("workspace_bytes after each upload:", sizes)
    assert sizes[1] == sizes[3] == sizes[5], sizes        # the 2nd, 4th and 6th upload: the same flow, the same buffers
    assert sizes[2] == sizes[4], sizes                    # the 3rd and 5th: the first flow again, the first cycle past
    assert sizes[0] <= sizes[2], sizes                    # (nothing is handed back that the first flow keeps)
    return sizes


def test_rank_one_and_full_rank_states_alternate(qoc, oracle):
    """n = 16 sandwich: rank-one Xi / Xt run the vector chain (small record buffer in d_states), full-rank ones the dense
    chain (state dumps in the same buffer)."""
    n = 16
    rng = np.random.default_rng(16)

    def problem(rank_one):
        A = np.array([_gen(rng, n, False, 0.6) for _ in range(E)])
        B = np.array([[_gen(rng, n, True, 0.4) for _ in range(K)] for _ in range(E)])

        def rho():
            vs = [rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(1 if rank_one else 3)]
            return sum(p * np.outer(v, v.conj()) / np.vdot(v, v).real for p, v in zip((1.0,) if rank_one else (0.6, 0.3, 0.1), vs))
        Xi, Xt = np.array([rho() for _ in range(E)]), np.array([rho() for _ in range(E)])
        return A, B, Xi, Xt, rng.uniform(0.2, 1.0, E), rng.uniform(-1, 1, (K, N))

    def expect(info, which):
        assert info["kernel_family"] == 1 and info["rank_one_chain"] == (1 if which == 0 else 0), info

    _cycle(qoc, lambda *ops: qoc.GrapeEngine("CoherenceTransfer", *ops, T, N), [problem(True), problem(False)],
           lambda p: oracle.ensemble_eval("CoherenceTransfer", *p[:5], p[5], T), n, expect)


def test_exact_gradient_releases_and_regains_the_costates(qoc, oracle):
    """n = 4, gradient = exact: Hermitian generators take the unitary flow's W_t dump and hand the costate array back,
    non-Hermitian ones need it again."""
    n = 4
    rng = np.random.default_rng(4)

    def problem(herm):
        A = np.array([_gen(rng, n, herm, 0.6) for _ in range(E)])
        B = np.array([[_gen(rng, n, herm, 0.4) for _ in range(K)] for _ in range(E)])
        Xi = np.array([np.eye(n, dtype=complex)] * E)
        Xt = np.array([np.linalg.qr(_gen(rng, n, False, 1.0))[0] for _ in range(E)])
        return A, B, Xi, Xt, rng.uniform(0.2, 1.0, E), rng.uniform(-1, 1, (K, N))

    def expect(info, which):
        assert info["kernel_family"] == 0 and info["unitary_flow"] == (1 if which == 0 else 0), info

    sizes = _cycle(qoc, lambda *ops: qoc.GrapeEngine("UnitaryGate", *ops, T, N, gradient="exact"),
                   [problem(True), problem(False)], lambda p: oracle.ensemble_exact("UnitaryGate", *p[:5], p[5], T), n, expect)
    assert sizes[2] < sizes[3], sizes                     # the costate array is counted only while it exists
