"""grape_eval_fom (ABI v8) and the dCRAB solver without a GPU: the C entry point is declared, exported and refuses a null
context; the dCRAB pulse synthesis is the ansatz of src/dCRAB.jl:26 on the grid of :42; the options are validated."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_eval_fom_and_abi_8(qoc):
    hdr = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    assert re.search(r"int grape_eval_fom\(grape_ctx \*ctx, int32_t n_x, const double \*x, double \*F, double \*member_F\);", hdr)
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", hdr).group(1)) == 8 == qoc.engine.ABI_VERSION
    assert "grape_eval_fom" in qoc.engine.EXPORTS


def test_eval_fom_refuses_a_null_context(qoc):
    lib = qoc.load_library()
    assert lib.grape_abi_version() == 8
    assert lib.grape_eval_fom(None, 1, None, None, None) == -1
    x, F = np.zeros(4), np.zeros(1)
    assert lib.grape_eval_fom(None, 1, x.ctypes.data, F.ctypes.data, None) == -1


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("N,T", [(1, 1.0), (10, 1.0), (25, 5.0)])
def test_dcrab_pulse_is_the_ansatz(qoc, K, N, T):
    rng = np.random.default_rng(10 * K + N)
    coeffs = rng.uniform(-1, 1, 2 * K)                   # control j's pair at [2j, 2j + 1], n_coeff = 2
    freqs = rng.random(K)
    got = qoc.dcrab_pulse(coeffs, freqs, N, T)
    assert got.shape == (K, N)
    dt = T / N
    for j in range(K):
        for i in range(N):
            t = i * dt                                   # 0, dt, ..., T - dt
            want = coeffs[2 * j] * np.cos(freqs[j] * t) + coeffs[2 * j + 1] * np.sin(freqs[j] * t)
            assert got[j, i] == pytest.approx(want, rel=1e-14, abs=1e-15)
    assert np.array_equal(got, qoc.dcrab_pulse(coeffs.reshape(K, 2), freqs, N, T))
    assert np.array_equal(got[:, 0], coeffs[0::2])       # t = 0: the cosine coefficients
    assert np.array_equal(qoc.dcrab_pulse(np.zeros(2 * K), freqs, N, T), np.zeros((K, N)))


def test_dcrab_options(qoc):
    alg = qoc.dCRAB(n_slices=10)
    assert (alg.n_freq, alg.n_coeff, alg.seed, alg.options) == (2, 2, None, None)
    assert qoc.dCRAB(10, 3, 2, seed=7, options={"maxiter": 5}).options == {"maxiter": 5}
    for bad in (dict(n_freq=0), dict(n_freq=-1), dict(n_coeff=3), dict(n_coeff=1)):
        with pytest.raises(ValueError):
            qoc.dCRAB(n_slices=10, **bad)
    with pytest.raises(ValueError):
        qoc.dCRAB(n_slices=0)


def test_engine_fom_checks_shapes_before_the_library(qoc):
    eng = object.__new__(qoc.GrapeEngine)
    eng.K, eng.N, eng.E, eng._h = 2, 5, 1, None
    for bad in (np.zeros((5, 2)), np.zeros((3, 5, 2)), np.zeros(10), np.zeros((1, 1, 2, 5))):
        with pytest.raises(ValueError):
            qoc.GrapeEngine.fom(eng, bad)
