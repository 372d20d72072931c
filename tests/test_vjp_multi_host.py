"""grape_eval_vjp_multi without a GPU: the header and the ctypes prototypes, the set-slowest layout the GPU tests rely on
(stacking the reference per set = the reference on the stacked sets), and trajectory_jacobian_rows' block bookkeeping and its
transpose identity with trajectory_jacobian on a stub engine backed by the NumPy references."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import rc_reference as rcr  # noqa: E402
import vjp_reference as vr  # noqa: E402
from conftest import ROOT  # noqa: E402


def header():
    hdr = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def prototype(name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header(), flags=re.S)
    assert m, f"{name} is not declared in include/grape_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_limit():
    hdr = header()
    assert re.search(r"#define GRAPE_MAX_VJP_COTANGENTS 8\b", hdr)
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", hdr).group(1)) == 8           # additive: the version stays
    host = prototype("grape_eval_vjp_multi")
    dev = prototype("grape_eval_vjp_multi_device")
    assert host == ["grape_ctx *ctx", "const double *x", "int32_t n_set", "int32_t n_obs", "int32_t per_member",
                    "const double *O", "const double *ybar", "const double *Xbar_final", "double *G"]
    assert dev == ["grape_ctx *ctx", "const double *d_x", "int32_t n_set", "int32_t n_obs", "int32_t per_member",
                   "const double *d_O", "const double *d_ybar", "const double *d_Xbar_final", "double *d_G", "void *stream"]


def test_ctypes_prototypes_mirror_the_header(qoc):
    lib = qoc.load_library()
    assert qoc.engine.MAX_VJP_COTANGENTS == 8
    for name in ("grape_eval_vjp_multi", "grape_eval_vjp_multi_device"):
        assert name in qoc.engine.EXPORTS
        fn = getattr(lib, name)
        want = [C.c_int32 if a.startswith("int32_t") else C.c_void_p for a in prototype(name)]
        assert list(fn.argtypes) == want, name
        assert fn.restype == C.c_int


def multi_reference(A, B, Xi, x, T, O, ybars, xbars, per_member=False, variant=0):
    """the reference per cotangent set, stacked set-slowest (n_set, K, N): the layout of GrapeEngine.observe_vjp_multi"""
    return np.stack([vr.vjp_ref(A, B, Xi, x, T, O, yb, xb, per_member, variant) for yb, xb in zip(ybars, xbars)])


@pytest.mark.parametrize("per_member", [False, True])
def test_stacking_the_reference_is_the_reference_on_stacked_sets(per_member):
    rng = np.random.default_rng(9121)
    n, m, K, E, N, T = 3, 2, 2, 2, 9, 1.5
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=False)
    x = rng.standard_normal((K, N))
    O = rng.standard_normal((E, 2, n, m) if per_member else (2, n, m)) + 0j
    ybars = rng.standard_normal((3, E, 2, N + 1)) + 1j * rng.standard_normal((3, E, 2, N + 1))
    xbars = rng.standard_normal((3, E, n, m)) + 1j * rng.standard_normal((3, E, n, m))
    G = multi_reference(A, B, Xi, x, T, O, ybars, xbars, per_member)
    assert G.shape == (3, K, N)
    many = vr.vjp_ref_many(A, B, Xi, x, T, vr.probes_per_member(O, E, per_member), ybars, xbars)      # all sets in one pass
    assert np.abs(G - many).max() <= 1e-13 * np.abs(many).max()
    for r in range(3):
        G1 = vr.vjp_recurrence(A, B, Xi, x, T, O, ybars[r], xbars[r], per_member)
        assert np.abs(G[r] - G1).max() <= 1e-13 * np.abs(G1).max()
    # linear in the cotangents: a combination of the blocks is the reference of the combined set
    w = np.array([0.5, -2.0, 0.25])
    Gc = vr.vjp_ref(A, B, Xi, x, T, O, np.tensordot(w, ybars, 1), np.tensordot(w, xbars, 1), per_member)
    assert np.abs(np.tensordot(w, G, 1) - Gc).max() <= 1e-13 * np.abs(Gc).max()
    # the C layout: (N+1, n_obs, E, n_set) column-major is the C-contiguous (n_set, E, n_obs, N+1) array -- block r is the
    # single call's array, whole and contiguous; likewise G (K, N, n_set) column-major = (n_set, N, K) C-contiguous
    flat = np.ascontiguousarray(ybars).reshape(-1)
    per = E * 2 * (N + 1)
    assert np.array_equal(flat[per:2 * per].reshape(E, 2, N + 1), ybars[1])
    Gf = np.ascontiguousarray(np.swapaxes(G, 1, 2)).reshape(-1)
    assert np.array_equal(Gf[K * N:2 * K * N].reshape(N, K).T, G[1])


class StubEngine:
    """what trajectory_jacobian_rows and trajectory_jacobian need of an engine, backed by the NumPy references of one small
    problem: the rows' blocks from vjp_reference, the columns' blocks from jvp_reference"""

    def __init__(self, chunked=False):
        rng = np.random.default_rng(9221)
        self.n, self.m, self.K, self.E, self.N, self.T = 2, 2, 2, 2, 5, 1.5
        self._cols = self.N
        self.A, self.B, self.Xi, _ = rcr.random_problem(rng, self.n, self.m, self.K, self.E, hermitian=False)
        self.x = rng.standard_normal((self.K, self.N))
        self.O = rng.standard_normal((3, self.n, self.m)) + 1j * rng.standard_normal((3, self.n, self.m))
        self.chunked = chunked
        self.blocks = []

    def _jacobian_reuse(self):
        return not self.chunked

    def _jacobian_rows_block(self, x, carry_x, ybars, ops, per_member):
        assert ybars.shape[1:] == (self.E, 3, self.N + 1) and 1 <= ybars.shape[0] <= 8
        self.blocks.append((carry_x, ybars.copy()))
        return np.stack([vr.vjp_ref(self.A, self.B, self.Xi, x, self.T, ops, yb, None, per_member) for yb in ybars])

    def _jacobian_block(self, x, carry_x, dirs, ops, per_member):
        return np.stack([jr.jvp_ref(self.A, self.B, self.Xi, x, d, self.T, ops, per_member)[0] for d in dirs])


ROWS5 = [(0, 0, 5), (1, 2, 3), (0, 1, 1), (1, 0, 0), (1, 1, 5)]


@pytest.mark.parametrize("n_rows,sets", [(1, [2]), (4, [8]), (5, [8, 2])])
def test_jacobian_rows_block_bookkeeping_on_a_stub_engine(qoc, n_rows, sets):
    GE = qoc.GrapeEngine
    eng = StubEngine()
    rows = ROWS5[:n_rows]
    J = GE.trajectory_jacobian_rows(eng, eng.x, eng.O, rows)
    assert J.shape == (n_rows, eng.K, eng.N) and J.dtype == np.complex128
    assert [b[1].shape[0] for b in eng.blocks] == sets       # two cotangent sets per row, at most 8 per block
    assert [b[0] for b in eng.blocks] == [True] + [False] * (len(sets) - 1)          # the first block carries x, the rest reuse
    sent = np.concatenate([b[1] for b in eng.blocks])
    for r, (k, j, s) in enumerate(rows):                      # the unit cotangents 1 and i at the row's entry, zero elsewhere
        for part, unit in ((0, 1.0), (1, 1.0j)):
            want = np.zeros((eng.E, 3, eng.N + 1), complex)
            want[k, j, s] = unit
            assert np.array_equal(sent[2 * r + part], want)
    # a member-chunked context holds no whole trajectory: every block carries x
    eng = StubEngine(chunked=True)
    GE.trajectory_jacobian_rows(eng, eng.x, eng.O, rows)
    assert [b[0] for b in eng.blocks] == [True] * len(sets)


def test_jacobian_rows_are_the_transposed_columns_on_a_stub_engine(qoc):
    """J_rows[r] = d y[k, j, s] / d x is entry (k, j, s) of every column of trajectory_jacobian: the transpose identity of the
    two references, to rounding"""
    GE = qoc.GrapeEngine
    eng = StubEngine()
    Jr = GE.trajectory_jacobian_rows(eng, eng.x, eng.O, ROWS5)
    Jc = GE.trajectory_jacobian(eng, eng.x, eng.O)            # (K N, E, n_obs, N+1)
    assert Jc.shape == (eng.K * eng.N, eng.E, 3, eng.N + 1)
    want = np.stack([Jc[:, k, j, s].reshape(eng.K, eng.N) for k, j, s in ROWS5])
    assert np.abs(want).max() > 0 and not Jr[3].any()         # (y at s = 0 does not depend on x)
    assert np.abs(Jr - want).max() <= 1e-12 * np.abs(want).max()
    for bad in ([], [(0, 0)], [(2, 0, 1)], [(0, 3, 1)], [(0, 0, 6)], [(0, 0, -1)]):
        with pytest.raises(ValueError):
            GE.trajectory_jacobian_rows(StubEngine(), eng.x, eng.O, bad)
    with pytest.raises(ValueError):
        GE.trajectory_jacobian_rows(StubEngine(), np.zeros((eng.K, eng.N + 1)), eng.O, ROWS5)
