"""grape_eval_hvp_device on the GPU: the device-resident form of the directional derivative of the trajectory pull-back.  The
oracle is bit-for-bit identity with the host form (which tests/test_gpu_hvp.py holds to the NumPy reference at the parity
bar); then the reuse of the stored trajectory, the flag it keeps, and the NOT_READY refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_running_cost import _chunk_budget, engine, make_case  # noqa: E402
from test_gpu_traj_device import _cm, _probes_cm, dev, ptr, vjp_dev  # noqa: E402
from test_gpu_vjp import cplx  # noqa: E402

pytestmark = pytest.mark.gpu

# n, m, N, E, hermitian, kernel
CASES = [(4, 4, 65, 3, True, "pair"), (3, 1, 64, 3, False, "lane"), (2, 2, 130, 5, True, "lane")]


def swept(names):
    return any(k.startswith("sweep_") for k in names)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def problem(n, m, N, E, herm):
    c = make_case(7100 + 10 * n + m, n, m, N, E, hermitian=herm)
    rng = np.random.default_rng(7101 + n)
    return c, dict(O=cplx(rng, 3, n, m), xdot=rng.standard_normal((c["K"], N)), yb=cplx(rng, E, 3, N + 1), xb=cplx(rng, E, n, m),
                   ybd=cplx(rng, E, 3, N + 1), xbd=cplx(rng, E, n, m))


def hvp_dev(torch, eng, x, d, reuse=False, dots=True, stream=0):
    """observe_hvp_device on a NaN-filled CUDA tensor -> Gdot (K, cols) as numpy, after a synchronise; x=None with reuse"""
    xd = None if reuse else dev(torch, np.asarray(x).T)
    t = [dev(torch, np.asarray(d["xdot"]).T), dev(torch, _probes_cm(d["O"], False)), dev(torch, d["yb"]), dev(torch, _cm(d["xb"])),
         dev(torch, d["ybd"]) if dots else None, dev(torch, _cm(d["xbd"])) if dots else None]
    G = torch.full((eng._cols, eng.K), float("nan"), dtype=torch.float64, device="cuda")
    eng.observe_hvp_device(ptr(xd), ptr(t[0]), d["O"].shape[0], False, ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(t[4]), ptr(t[5]), ptr(G), stream)
    torch.cuda.synchronize()
    return np.ascontiguousarray(G.cpu().numpy().T)


@pytest.mark.parametrize("n,m,N,E,herm,kernel", CASES)
def test_device_form_and_reuse_are_bitwise_the_host_form(qoc, torch, monkeypatch, n, m, N, E, herm, kernel):
    monkeypatch.setenv("GRAPE_SMALL_KERNEL", kernel)
    c, d = problem(n, m, N, E, herm)
    with engine(qoc, c) as eng:
        calls = eng.calls
        for dots in (True, False):
            Gh = eng.observe_hvp(c["x"], d["xdot"], d["O"], d["yb"], d["xb"], d["ybd"] if dots else None, d["xbd"] if dots else None)
            Gd = hvp_dev(torch, eng, c["x"], d, dots=dots)
            names = eng.kernel_names()
            assert "trajectory_hvp_kernel" in names and swept(names), names
            assert not np.isnan(Gd).any() and np.array_equal(Gd, Gh)
            Gr = hvp_dev(torch, eng, None, d, reuse=True, dots=dots)
            names = eng.kernel_names()
            assert "trajectory_hvp_kernel" in names and "vjp_sum_kernel" in names and not swept(names), names
            assert np.array_equal(Gr, Gh)
            # the reuse call leaves the flag set: a pull-back along the same trajectory follows directly
            Gv = vjp_dev(torch, eng, None, d["O"], d["yb"], d["xb"], False, reuse=True)
            assert not swept(eng.kernel_names())
            assert np.array_equal(Gv, eng.observe_vjp(c["x"], d["O"], ybar=d["yb"], xbar_final=d["xb"]))
        assert eng.calls > calls                              # (the device form counts as a call on the engine)


def reuse_refused(torch, qoc, eng, d, word=None):
    with pytest.raises(qoc.GrapeError) as ei:
        hvp_dev(torch, eng, None, d, reuse=True)
    assert ei.value.status == -5 and "reuse" in str(ei.value) and "grape_eval_hvp_device" in str(ei.value), str(ei.value)
    if word:
        assert word in str(ei.value), str(ei.value)


def test_reuse_is_refused_without_a_trajectory(qoc, torch, monkeypatch):
    c, d = problem(3, 1, 64, 3, False)
    with engine(qoc, c) as eng:
        F0, G0 = eng.eval(c["x"])
        reuse_refused(torch, qoc, eng, d)                     # a fresh context (one eval, no device form)
        Gd = hvp_dev(torch, eng, c["x"], d)
        eng.eval(c["x"])                                      # an intervening evaluation
        reuse_refused(torch, qoc, eng, d)
        reuse_refused(torch, qoc, eng, d)                     # (a refused call leaves the flag clear)
        F, G = eng.eval(c["x"])
        assert F == F0 and np.array_equal(G, G0)
    c, d = problem(3, 1, 64, 10, False)                       # (ten members: a budget for four leaves a ragged chunking)
    with engine(qoc, c) as eng:
        Gd = hvp_dev(torch, eng, c["x"], d)
        info = eng.info
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(_chunk_budget(c, info, False, 4)))
    with engine(qoc, c) as eng:
        assert 0 < eng.info["member_chunk"] < c["E"]
        assert np.array_equal(hvp_dev(torch, eng, c["x"], d), Gd)         # member-chunked: the unchunked bits
        reuse_refused(torch, qoc, eng, d, "member_chunk")
