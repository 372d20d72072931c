"""grape_eval_jvp_multi without a GPU: the header and the ctypes prototypes, the direction-slowest layout the GPU tests rely on
(stacking the reference per direction = the reference on the stacked directions), and trajectory_jacobian's column
bookkeeping on a stub engine."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import rc_reference as rcr  # noqa: E402
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
    assert re.search(r"#define GRAPE_MAX_JVP_DIRECTIONS 8\b", hdr)
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", hdr).group(1)) == 8           # additive: the version stays
    host = prototype("grape_eval_jvp_multi")
    dev = prototype("grape_eval_jvp_multi_device")
    assert host == ["grape_ctx *ctx", "const double *x", "int32_t n_dir", "const double *xdot", "int32_t n_obs",
                    "int32_t per_member", "const double *O", "double *ydot", "double *Xdot_final"]
    assert dev == ["grape_ctx *ctx", "const double *d_x", "int32_t n_dir", "const double *d_xdot", "int32_t n_obs",
                   "int32_t per_member", "const double *d_O", "double *d_ydot", "double *d_Xdot_final", "void *stream"]


def test_ctypes_prototypes_mirror_the_header(qoc):
    lib = qoc.load_library()
    assert qoc.engine.MAX_JVP_DIRECTIONS == 8
    for name in ("grape_eval_jvp_multi", "grape_eval_jvp_multi_device"):
        assert name in qoc.engine.EXPORTS
        fn = getattr(lib, name)
        want = [C.c_int32 if a.startswith("int32_t") else C.c_void_p for a in prototype(name)]
        assert list(fn.argtypes) == want, name
        assert fn.restype == C.c_int


def stack_directions(per_direction):
    """[(ydot (E, n_obs, N+1), Xdot_final (E, n, m))] per direction -> (n_dir, E, n_obs, N+1), (n_dir, E, n, m): the layout
    of GrapeEngine.observe_jvp_multi"""
    return np.stack([y for y, _ in per_direction]), np.stack([X for _, X in per_direction])


def multi_reference(A, B, Xi, x, xdots, T, O, per_member=False, variant=0):
    """the reference on a stacked direction array (n_dir, K, N): one tangent walk per direction"""
    return stack_directions([jr.jvp_ref(A, B, Xi, x, xd, T, O, per_member, variant) for xd in xdots])


@pytest.mark.parametrize("per_member", [False, True])
def test_stacking_the_reference_is_the_reference_on_stacked_directions(per_member):
    rng = np.random.default_rng(9101)
    n, m, K, E, N, T = 3, 2, 2, 2, 9, 1.5
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=False)
    x = rng.standard_normal((K, N))
    xdots = rng.standard_normal((3, K, N))
    O = rng.standard_normal((E, 2, n, m) if per_member else (2, n, m)) + 0j
    yd, Xd = multi_reference(A, B, Xi, x, xdots, T, O, per_member)
    assert yd.shape == (3, E, 2, N + 1) and Xd.shape == (3, E, n, m)
    for d in range(3):
        y1, X1 = jr.jvp_recurrence(A, B, Xi, x, xdots[d], T, O, per_member)
        assert np.abs(yd[d] - y1).max() <= 1e-13 * np.abs(y1).max()
        assert np.abs(Xd[d] - X1).max() <= 1e-13 * np.abs(X1).max()
    # linear in the directions: a combination of the blocks is the reference of the combined direction
    w = np.array([0.5, -2.0, 0.25])
    yc, Xc = jr.jvp_ref(A, B, Xi, x, np.tensordot(w, xdots, 1), T, O, per_member)
    assert np.abs(np.tensordot(w, yd, 1) - yc).max() <= 1e-13 * np.abs(yc).max()
    assert np.abs(np.tensordot(w, Xd, 1) - Xc).max() <= 1e-13 * np.abs(Xc).max()
    # the C layout: (N+1, n_obs, E, n_dir) column-major is the C-contiguous (n_dir, E, n_obs, N+1) array -- block d is the
    # single call's array, whole and contiguous
    flat = np.ascontiguousarray(yd).reshape(-1)
    per = E * 2 * (N + 1)
    assert np.array_equal(flat[per:2 * per].reshape(E, 2, N + 1), yd[1])


class StubEngine:
    """what trajectory_jacobian needs of an engine: y[k, j, s] = sum_i M[k, j, s, i] x.flat[i], whose Jacobian column i is
    M[..., i]"""

    def __init__(self, K, cols, chunked=False):
        self.K, self._cols, self.E = K, cols, 2
        self.M = np.random.default_rng(9201).standard_normal((2, 3, 5, K * cols))
        self.chunked = chunked
        self.blocks = []

    def _jacobian_reuse(self):
        return not self.chunked

    def _jacobian_block(self, x, carry_x, dirs, ops, per_member):
        assert dirs.shape[1:] == (self.K, self._cols) and 1 <= dirs.shape[0] <= 8
        self.blocks.append((carry_x, dirs.copy()))
        return np.einsum("kjsi,di->dkjs", self.M, dirs.reshape(dirs.shape[0], -1))


def test_jacobian_column_bookkeeping_on_a_stub_engine(qoc):
    GE = qoc.GrapeEngine
    K, cols = 3, 7                                           # 21 columns: blocks of 8, 8, 5
    x = np.zeros((K, cols))
    eng = StubEngine(K, cols)
    J = GE.trajectory_jacobian(eng, x, None)
    assert J.shape == (21, 2, 3, 5)
    assert np.array_equal(J, np.moveaxis(eng.M, -1, 0))
    assert [b[1].shape[0] for b in eng.blocks] == [8, 8, 5]
    assert [b[0] for b in eng.blocks] == [True, False, False]        # the first block carries x, the rest reuse
    for b, (_, dirs) in enumerate(eng.blocks):               # unit directions, row-major flat index
        flat = dirs.reshape(dirs.shape[0], -1)
        assert np.array_equal(flat, np.eye(21)[8 * b:8 * b + flat.shape[0]])
    # listed columns come back in the caller's order; negative indices count from the end
    eng = StubEngine(K, cols)
    J = GE.trajectory_jacobian(eng, x, None, columns=[20, 0, -2, 5])
    assert np.array_equal(J, np.moveaxis(eng.M[..., [20, 0, 19, 5]], -1, 0)) and len(eng.blocks) == 1
    # a member-chunked context holds no whole trajectory: every block carries x
    eng = StubEngine(K, cols, chunked=True)
    GE.trajectory_jacobian(eng, x, None, columns=range(9))
    assert [b[0] for b in eng.blocks] == [True, True]
    for bad in ([21], [-22], [1, 1], [], [0.5]):
        with pytest.raises(ValueError):
            GE.trajectory_jacobian(StubEngine(K, cols), x, None, columns=bad)
    with pytest.raises(ValueError):
        GE.trajectory_jacobian(StubEngine(K, cols), np.zeros((K, cols + 1)), None)
    assert qoc.engine.jacobian_blocks(list(range(17))) == [list(range(8)), list(range(8, 16)), [16]]
    assert qoc.engine.jacobian_columns(4) == [0, 1, 2, 3]
