"""grape_set_basis / grape_get_controls without a GPU: both entry points are declared and exported under the unchanged
ABI version 8, refuse a null context, and fourier_basis spans exactly the ansatz dcrab_pulse synthesises."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_basis_entry_points_under_abi_8(qoc):
    hdr = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    assert re.search(r"int grape_set_basis\(grape_ctx \*ctx, int32_t n_params, int32_t n_bases, const double \*phi, "
                     r"const double \*x0\);", hdr)
    assert re.search(r"int grape_get_controls\(grape_ctx \*ctx, const double \*theta, double \*x\);", hdr)
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", hdr).group(1)) == 8 == qoc.engine.ABI_VERSION
    assert "grape_set_basis" in qoc.engine.EXPORTS and "grape_get_controls" in qoc.engine.EXPORTS
    assert "slice space" in hdr                              # what stays in (K, N) is documented


def test_basis_entry_points_refuse_a_null_context(qoc):
    lib = qoc.load_library()
    assert lib.grape_abi_version() == 8
    phi, th, x = np.ones(6), np.zeros(4), np.zeros(6)
    assert lib.grape_set_basis(None, 2, 1, phi.ctypes.data, None) == -1
    assert lib.grape_set_basis(None, 0, 1, None, None) == -1
    assert lib.grape_get_controls(None, th.ctypes.data, x.ctypes.data) == -1
    assert lib.grape_get_controls(None, None, None) == -1


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("N,T", [(1, 1.0), (10, 1.0), (25, 5.0), (500, 10.0)])
def test_fourier_basis_spans_the_dcrab_ansatz(qoc, K, N, T):
    rng = np.random.default_rng(100 * K + N)
    coeffs = rng.uniform(-1, 1, 2 * K)                       # control j's pair at [2j, 2j + 1]
    freqs = rng.random(K) * 5
    pulse = qoc.dcrab_pulse(coeffs, freqs, N, T)
    for j in range(K):
        phi = qoc.fourier_basis(N, T, [freqs[j]])
        assert phi.shape == (N, 2)
        assert np.allclose(coeffs[2 * j:2 * j + 2] @ phi.T, pulse[j], rtol=1e-15, atol=1e-15)
    # several frequencies: columns cos(w_0 t), sin(w_0 t), cos(w_1 t), sin(w_1 t), ... -- the flat coefficient order
    phi = qoc.fourier_basis(N, T, freqs)
    assert phi.shape == (N, 2 * K)
    for j in range(K):
        assert np.array_equal(phi[:, 2 * j:2 * j + 2], qoc.fourier_basis(N, T, [freqs[j]]))
    assert np.allclose(coeffs @ phi.T, pulse.sum(axis=0), rtol=1e-15, atol=4e-15)   # (a 2K-term sum: K - 1 more roundings)
    assert np.array_equal(phi[0], np.tile([1.0, 0.0], K))    # t = 0


def test_engine_checks_parameter_shapes_before_the_library(qoc):
    eng = object.__new__(qoc.GrapeEngine)
    eng.K, eng.N, eng.E, eng._h = 2, 5, 1, None
    assert eng.n_params == 0
    for bad in (np.zeros((4, 3)), np.zeros((2, 4, 3)), np.zeros((2, 2, 5, 3)), np.zeros(5)):
        with pytest.raises(ValueError):
            qoc.GrapeEngine.set_basis(eng, bad)
    with pytest.raises(ValueError):
        qoc.GrapeEngine.set_basis(eng, np.zeros((5, 3)), x0=np.zeros((5, 2)))
    eng.n_params = 3                                         # parameter mode: theta is (K, M)
    for call in (qoc.GrapeEngine.eval, qoc.GrapeEngine.fom, qoc.GrapeEngine.lbfgs, qoc.GrapeEngine.controls):
        with pytest.raises(ValueError):
            call(eng, np.zeros((2, 5)))
    with pytest.raises(ValueError):
        qoc.GrapeEngine.eval_batch(eng, np.zeros((1, 2, 5)))


def test_grape_options_carry_a_basis(qoc):
    alg = qoc.GRAPE(n_slices=10)
    assert alg.basis is None and alg.basis_offset is None
    phi = qoc.fourier_basis(10, 1.0, [1.0, 2.0])
    assert qoc.GRAPE(n_slices=10, basis=phi).basis is phi
    res = qoc.SolutionResult(None, 0.0, None, None, alg)
    assert res.parameters is None
