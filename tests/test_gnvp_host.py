"""grape_eval_gnvp on the host: the NumPy reference of tests/gnvp_reference.py (jvp_recurrence -> weight blocks ->
vjp_of_propagators) against the dense J' W J built from unit directions through the double sum; the dense matrix's symmetry
and definiteness; and the visibility of every weight plane and of wf above the GPU tests' tolerance.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnvp_cases as gc  # noqa: E402
import gnvp_reference as gr  # noqa: E402
import rc_reference as rcr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402

T = 1.5
BAR = 1e-12                                                       # of |ref|_inf: two routes through the same f64 model

# n, m, N, E, hermitian, per-member probes, per-member weights  (N <= 8, K N <= 16: the dense matrix is 16 x 16 at most)
TINY = [(3, 2, 7, 3, False, False, False), (3, 2, 7, 3, False, True, True), (2, 2, 8, 2, True, False, True),
        (4, 1, 5, 2, False, True, False), (4, 4, 3, 2, True, False, False), (2, 1, 1, 1, True, False, True)]


def tiny_case(n, m, N, E, herm, pm, wpm, K=2, J=3):
    rng = np.random.default_rng(4100 + 100 * n + 10 * m + N + 2 * herm + pm)
    A, B, Xi, _ = rcr.random_problem(rng, n, m, K, E, hermitian=herm)
    O = gc.cplx(rng, E, J, n, m) if pm else gc.cplx(rng, J, n, m)
    w = gc.psd_blocks(rng, E, J, N + 1) if wpm else gc.psd_blocks(rng, J, N + 1)
    return dict(A=A, B=B, Xi=Xi, x=rng.standard_normal((K, N)), xdot=rng.standard_normal((K, N)), O=O, w=w,
                wf=rng.uniform(0.2, 1.5, E), pm=pm)


_DENSE = {}


def dense(row):
    if row not in _DENSE:
        c = tiny_case(*row)
        M = gr.gn_dense(c["A"], c["B"], c["Xi"], c["x"], T, c["O"], c["w"], c["wf"], c["pm"], blocks=True)
        M.setflags(write=False)
        _DENSE[row] = (c, M)
    return _DENSE[row]


@pytest.mark.parametrize("row", TINY)
def test_the_composition_is_the_dense_operator_applied(row):
    c, M = dense(row)
    ref = gr.gnvp_ref(c["A"], c["B"], c["Xi"], c["x"], c["xdot"], T, c["O"], c["w"], c["wf"], c["pm"], blocks=True)
    want = (M @ c["xdot"].reshape(-1)).reshape(ref.shape)
    err, amax = np.abs(ref - want).max(), np.abs(ref).max()
    print(f"{row}: |gnvp_ref - gn_dense v|_inf={err:.3e} |ref|_inf={amax:.3e}")
    assert amax > 0 and err <= BAR * amax


@pytest.mark.parametrize("row", TINY)
def test_the_dense_operator_is_symmetric_and_positive(row):
    _, M = dense(row)
    asym, amax = np.abs(M - M.T).max(), np.abs(M).max()
    lam = np.linalg.eigvalsh(0.5 * (M + M.T))
    print(f"{row}: |M - M'|_inf={asym:.3e} |M|_inf={amax:.3e} eigenvalues in [{lam[0]:.3e}, {lam[-1]:.3e}]")
    assert amax > 0 and asym <= BAR * amax
    assert lam[-1] > 0 and lam[0] >= -BAR * lam[-1]               # PSD blocks, wf >= 0


@pytest.mark.parametrize("row", TINY[:3])
def test_scalar_weights_are_the_blocks_w_0_w(row):
    c, _ = dense(row)
    w = c["w"][0]
    args = (c["A"], c["B"], c["Xi"], c["x"], c["xdot"], T, c["O"])
    a = gr.gnvp_ref(*args, w, None, c["pm"], blocks=False)
    b = gr.gnvp_ref(*args, np.stack([w, np.zeros_like(w), w]), None, c["pm"], blocks=True)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("row", TINY)
def test_every_plane_and_wf_is_visible_above_the_gpu_tolerance(row):
    """zeroing one plane (or wf) moves Gn by far more than the bar of the GPU tests: no term can hide under it"""
    c, _ = dense(row)
    args = (c["A"], c["B"], c["Xi"], c["x"], c["xdot"], T, c["O"])
    full = gr.gnvp_ref(*args, c["w"], c["wf"], c["pm"], blocks=True)
    amax = np.abs(full).max()
    for plane in range(3):
        w = c["w"].copy()
        w[plane] = 0.0
        moved = np.abs(gr.gnvp_ref(*args, w, c["wf"], c["pm"], blocks=True) - full).max()
        print(f"{row}: without plane {plane}: moved by {moved / amax:.3e} of |Gn|_inf")
        assert moved > 1e3 * PARITY_RTOL * amax
    moved = np.abs(gr.gnvp_ref(*args, c["w"], None, c["pm"], blocks=True) - full).max()
    print(f"{row}: without wf: moved by {moved / amax:.3e} of |Gn|_inf")
    assert moved > 1e3 * PARITY_RTOL * amax


@pytest.mark.parametrize("row", [gc.SHAPES[1], gc.SHAPES[5]])
def test_the_gpu_parity_cases_have_visible_terms(row):
    """on parity cases of the GPU tests: the wf term and the weighted read-out both stand far above the tolerance"""
    ref = gc.shape_reference(row)
    both, final = ref[("scalar_shared_wf", 3, 1)], ref[("final_only", 0, 0)]
    amax = np.abs(both).max()
    assert np.abs(final).max() > 1e3 * PARITY_RTOL * amax and np.abs(both - final).max() > 1e3 * PARITY_RTOL * amax
