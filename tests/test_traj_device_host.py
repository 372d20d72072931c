"""The device forms of the trajectory read-out and its VJP, without a GPU: the exports, the null-context answer, the argument
checks of the Python wrappers and of autograd.trajectory_device on a stand-in engine, and the torch-free package import."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_library_exports_both_symbols(qoc):
    lib = qoc.load_library()
    for name in ("grape_eval_observables_device", "grape_eval_vjp_device"):
        assert name in qoc.engine.EXPORTS and getattr(lib, name) is not None
    assert lib.grape_abi_version() == 8                       # additive: the ABI version stays


def test_null_context_is_an_invalid_argument_without_a_device(qoc):
    lib = qoc.load_library()
    v = C.c_void_p(64)
    assert lib.grape_eval_observables_device(None, v, 1, 0, v, v, v, None, None) == -1
    assert b"grape_eval_observables_device: null context" in lib.grape_last_error(None)
    assert lib.grape_eval_vjp_device(None, None, 1, 0, v, v, v, v, None) == -1
    assert b"grape_eval_vjp_device: null context" in lib.grape_last_error(None)


class StandInEngine:
    """the attributes trajectory_device reads; the device calls must never be reached by a refused argument"""
    n, m, E, K, N, n_params, calls = 3, 2, 2, 2, 6, 0, 0

    def observe_device(self, *a):
        raise AssertionError("reached the library")

    observe_vjp_device = observe_device


def test_trajectory_device_checks_its_arguments_first(qoc):
    import torch
    from quoptimalcontrol_jl_amd import autograd
    eng = StandInEngine()
    ops = np.ones((1, eng.n, eng.m), complex)
    x = torch.zeros(eng.K, eng.N, dtype=torch.float64)
    with pytest.raises(TypeError):
        autograd.trajectory_device(eng, x, ops)               # a CPU tensor
    with pytest.raises(TypeError):
        autograd.trajectory_device(eng, x.to(torch.float32), ops)
    with pytest.raises(TypeError):
        autograd.trajectory_device(eng, np.zeros((eng.K, eng.N)), ops)
    with pytest.raises(ValueError):
        autograd.trajectory_device(eng, x, None)
    with pytest.raises(ValueError):
        autograd.trajectory_device(eng, x[:, :5], ops)
    for bad in (np.ones((17, eng.n, eng.m), complex), np.ones((1, eng.m, eng.n), complex), np.ones((eng.n, eng.m), complex)):
        with pytest.raises(ValueError):
            autograd.trajectory_device(eng, x, bad)
    with pytest.raises(ValueError):
        autograd.trajectory_device(eng, x, np.ones((1, eng.n, eng.m), complex), per_member=True)
    eng.n_params = 4                                          # parameter mode: x is (K, M)
    with pytest.raises(ValueError):
        autograd.trajectory_device(eng, x, ops)


def test_raw_pointer_wrappers_check_before_the_library_is_called(qoc):
    class NoLib:
        def __getattr__(self, name):
            raise AssertionError("reached the library")

    eng = object.__new__(qoc.GrapeEngine)
    eng._h, eng._lib = None, NoLib()
    for call in (lambda: eng.observe_device(8, 17, False, 8, 8, 8), lambda: eng.observe_device(8, -1, False, 8, 8, 8),
                 lambda: eng.observe_device(0, 1, False, 8, 8, 8), lambda: eng.observe_device(8, 1, False, 8, 0, 0),
                 lambda: eng.observe_device(8, 1, False, 0, 8, 8), lambda: eng.observe_vjp_device(8, 1, False, 8, 0, 0, 8),
                 lambda: eng.observe_vjp_device(0, 1, False, 8, 8, 0, 0), lambda: eng.observe_vjp_device(0, 17, False, 8, 8, 0, 8)):
        with pytest.raises(ValueError):
            call()


def test_engine_counts_the_calls_that_touch_the_context(qoc):
    class Lib:
        grape_eval = grape_get_info = grape_get_controls = grape_last_error = grape_set_risk = staticmethod(lambda *a: 0)

    eng = object.__new__(qoc.GrapeEngine)
    lib = qoc.engine._CountingLib(Lib(), eng)
    assert eng.calls == 0
    lib.grape_get_info, lib.grape_last_error
    assert eng.calls == 0                                     # read-only accessors do not count
    lib.grape_eval, lib.grape_set_risk, lib.grape_get_controls
    assert eng.calls == 3


def test_package_import_does_not_pull_torch_in():
    code = ("import sys; sys.path.insert(0, %r); import quoptimalcontrol_jl_amd as q; assert 'torch' not in sys.modules; "
            "assert 'grape_eval_vjp_device' in q.engine.EXPORTS and hasattr(q.GrapeEngine, 'observe_device') "
            "and hasattr(q.GrapeEngine, 'observe_vjp_device')" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)
