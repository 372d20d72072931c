"""GPU: pulses restricted to a basis on the device (grape_set_basis / grape_get_controls, "parameter mode").

x[c,t] = x0[c,t] + sum_m theta[c,m] phi_b[t,m] is expanded by basis_expand_kernel in front of every evaluation and the complete
summed row { G_tot, F } folded onto the basis by basis_project_kernel behind it.  What is checked, and against what:

  expansion    eng.controls(theta) against NumPy's x0 + theta @ phi.T, element-wise within 2 M 2^-53 (|x0| + |theta| @ |phi|.T)
               -- the standard rounding bound of an M-term dot product, once for each side;
  F            BIT FOR BIT the F a second context WITHOUT a basis returns for that expanded pulse (the flows are untouched);
  G_theta      against that context's G_x @ phi, element-wise within 2 N 2^-53 (|G_x| @ |phi|) -- the same bound for the N-term
               sums of the projection;
  penalties    evaluated on the physical pulse: F bitwise the slice-mode F_tot, G_theta within the bound of G_tot @ phi.

The bounds are derived from the number format, not measured."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_parity
from settings_sequences import compare_lbfgs_iterates
from test_gpu_fom import random_problem as fom_problem
from test_gpu_tile import _random_problem

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def engine(qoc, w, **kw):
    return qoc.GrapeEngine(w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N, **kw)


def expand(phi, x0, theta):
    """NumPy's x0 + theta @ phi.T and the element-wise bound of the two M-term sums"""
    if phi.ndim == 2:
        x, mag = theta @ phi.T, np.abs(theta) @ np.abs(phi).T
    else:
        x = np.array([theta[c] @ phi[c].T for c in range(theta.shape[0])])
        mag = np.array([np.abs(theta[c]) @ np.abs(phi[c]).T for c in range(theta.shape[0])])
    if x0 is not None:
        x, mag = x0 + x, np.abs(x0) + mag
    return x, 2 * phi.shape[-1] * U * mag


def project(phi, G):
    """G @ phi and the element-wise bound of the two N-term sums"""
    N = phi.shape[-2]
    if phi.ndim == 2:
        return G @ phi, 2 * N * U * (np.abs(G) @ np.abs(phi))
    return (np.array([G[c] @ phi[c] for c in range(G.shape[0])]),
            2 * N * U * np.array([np.abs(G[c]) @ np.abs(phi[c]) for c in range(G.shape[0])]))


def draw(w, M, seed, per_control=False, offset=True):
    rng = np.random.default_rng(seed)
    phi = rng.standard_normal((w.K, w.N, M) if per_control else (w.N, M))
    x0 = 0.3 * rng.standard_normal((w.K, w.N)) if offset else None
    theta = rng.uniform(-1, 1, (w.K, M)) / np.sqrt(M)
    return phi, x0, theta


def chain_rule(qoc, w, phi, x0, theta, what, penalties=None, **kw):
    """parameter mode on one context against slice mode on another; returns (F, G_theta, kernel names)"""
    with engine(qoc, w, **kw) as eng:
        if penalties:
            eng.set_penalties(*penalties)
        eng.set_basis(phi, x0)
        assert eng.n_params == phi.shape[-1]
        x = eng.controls(theta)
        F, G = eng.eval(theta)
        names = eng.kernel_names()
        F2, G2 = eng.eval(theta)
        info = eng.info
    assert F == F2 and np.array_equal(G, G2), f"{what}: not reproducible"
    x_np, x_tol = expand(phi, x0, theta)
    print(f"{what}: max |x - x_np| / bound = {(np.abs(x - x_np) / np.maximum(x_tol, 1e-300)).max():.3f}")
    assert x.shape == (w.K, w.N) and np.all(np.abs(x - x_np) <= x_tol), f"{what}: expansion"
    with engine(qoc, w, **kw) as ref:
        if penalties:
            ref.set_penalties(*penalties)
        Fx, Gx = ref.eval(x)
        ref_names = ref.kernel_names()
    print(f"{what}: F = {F!r}, slice mode {Fx!r}")
    assert F == Fx, f"{what}: F {F!r} is not the slice-mode F {Fx!r}"
    want, tol = project(phi, Gx)
    print(f"{what}: max |G_theta - G_x phi| / bound = {(np.abs(G - want) / np.maximum(tol, 1e-300)).max():.3f}")
    assert G.shape == theta.shape and np.all(np.abs(G - want) <= tol), f"{what}: projection"
    assert names[0] == "basis_expand_kernel" and names[-1] == "basis_project_kernel", names
    assert "basis_expand_kernel" not in ref_names and "basis_project_kernel" not in ref_names, ref_names
    return F, G, names, info


def sized(qoc, n, sys_type, seed):
    big = n >= 32
    w = _random_problem(qoc, n, 3, 5 if big else 12, 2 if big else 3, sys_type, seed=seed, hermitian=True, mixed=True)
    s = 0.6 if n == 1 else min(1.0, 2.0 / n)
    w.A *= s
    w.B *= s
    return w


# ---- 1. chain rule, every kernel family -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 16, 32, 40, 70])
@pytest.mark.parametrize("sys_type", ["UnitaryGate", "StateTransfer"])
@pytest.mark.parametrize("variant", [0, 1])
def test_chain_rule_in_every_family(qoc, n, sys_type, variant):
    w = sized(qoc, n, sys_type, 300 + n)
    M = 3 if w.N == 5 else 5
    phi, x0, theta = draw(w, M, 7 * n + variant)
    chain_rule(qoc, w, phi, x0, theta, f"n={n} {sys_type} variant {variant}", variant=variant)


def test_chain_rule_with_the_exact_gradient(qoc):
    w = sized(qoc, 4, "UnitaryGate", 41)
    phi, x0, theta = draw(w, 4, 42)
    chain_rule(qoc, w, phi, x0, theta, "exact gradient", variant=1, gradient="exact", objective="c1")


def test_chain_rule_with_n_by_1_states(qoc):
    w = fom_problem(qoc, 4, 2, 24, 5, "UnitaryGate", seed=43, hermitian=False, m=1)
    phi, x0, theta = draw(w, 6, 44)
    chain_rule(qoc, w, phi, x0, theta, "n x 1 states")


def test_chain_rule_on_a_member_chunked_context(qoc, monkeypatch):
    w = _random_problem(qoc, 70, 3, 4, 5, "UnitaryGate", seed=12, hermitian=True)
    w.A *= 0.2
    w.B *= 0.2
    phi, x0, theta = draw(w, 3, 45)
    F0, G0, _, info0 = chain_rule(qoc, w, phi, x0, theta, "unchunked")
    monkeypatch.setenv("GRAPE_MAX_WORKSPACE_BYTES", str(2 * 2 * w.N * 70 * 70 * 16 + 1000))       # two members' P_t and X_t
    F1, G1, _, info1 = chain_rule(qoc, w, phi, x0, theta, "member-chunked")
    assert info1["member_chunk"] == 2 and info0["member_chunk"] != 2
    assert F1 == F0 and np.array_equal(G1, G0)               # member-chunked = unchunked, bit for bit, here too


# ---- 2. penalties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C3", "C4"])
def test_penalties_act_on_the_physical_pulse(qoc, cfg):
    w = qoc.workloads.config("C3", E=8, N=100) if cfg == "C3" else qoc.workloads.config("C4", E=3, N=12)
    amp, var = np.linspace(0.3, 0.9, w.K), np.linspace(0.8, 0.2, w.K)
    phi, x0, theta = draw(w, 6, 46)
    F, G, _, _ = chain_rule(qoc, w, phi, x0, theta, f"{cfg} with C3 / C4 weights", penalties=(amp, var))
    F_plain, _, _, _ = chain_rule(qoc, w, phi, x0, theta, f"{cfg} without")
    x = expand(phi, x0, theta)[0]
    Fp = float(np.sum(amp[:, None] * x ** 2) + np.sum(var[:, None] * np.diff(x, axis=1) ** 2))
    assert abs((F - F_plain) - Fp) <= 1e-10 * max(1.0, Fp)  # (the penalty of the PHYSICAL pulse is what was added)


# ---- 3. special cases -----------------------------------------------------------------------------------------------------
def test_identity_basis_is_slice_mode(qoc):
    w = qoc.workloads.config("C3", E=8, N=60)
    with engine(qoc, w) as eng:
        F0, G0 = eng.eval(w.x)
        eng.set_basis(np.eye(w.N))
        assert np.array_equal(eng.controls(w.x), w.x)        # 1 * theta + 0 * (...) is exact
        F, G = eng.eval(w.x)
    assert F == F0
    want, tol = project(np.eye(w.N), G0)
    assert np.all(np.abs(G - want) <= tol)


@pytest.mark.parametrize("cfg", ["C3", "C4"])
def test_one_basis_per_control(qoc, cfg):
    w = qoc.workloads.config("C3", E=8, N=100) if cfg == "C3" else qoc.workloads.config("C4", E=3, N=12)
    phi, x0, theta = draw(w, 7, 47, per_control=True)
    assert not np.array_equal(phi[0], phi[1])
    chain_rule(qoc, w, phi, x0, theta, f"{cfg}, n_bases = K")
    chain_rule(qoc, w, phi, None, theta, f"{cfg}, n_bases = K, no offset")


@pytest.mark.parametrize("cfg", ["C3", "C4"])
def test_clearing_the_basis_restores_slice_mode_bitwise(qoc, cfg):
    w = qoc.workloads.config("C3", E=8, N=100) if cfg == "C3" else qoc.workloads.config("C4", E=3, N=12)
    phi, x0, theta = draw(w, 5, 48)
    with engine(qoc, w, max_batch=2) as eng:
        F0, G0 = eng.eval(w.x)
        names0 = eng.kernel_names()
        f0 = eng.fom(w.x)
        Fb0, Gb0 = eng.eval_batch(np.array([w.x, 0.5 * w.x]))
        eng.set_basis(phi, x0)
        eng.eval(theta)
        eng.fom(theta)
        eng.set_basis(None)
        assert eng.n_params == 0
        F1, G1 = eng.eval(w.x)
        names1 = eng.kernel_names()
        f1 = eng.fom(w.x)
        Fb1, Gb1 = eng.eval_batch(np.array([w.x, 0.5 * w.x]))
        assert np.array_equal(eng.controls(w.x), w.x)
    assert F1 == F0 and np.array_equal(G1, G0) and names1 == names0 and f1 == f0
    assert np.array_equal(Fb1, Fb0) and np.array_equal(Gb1, Gb0)


def test_basis_persists_across_set_operators(qoc):
    w = qoc.workloads.config("C3", E=8, N=60)
    phi, x0, theta = draw(w, 5, 49)
    with engine(qoc, w) as eng:
        eng.set_basis(phi, x0)
        F0, G0 = eng.eval(theta)
        eng.set_operators(w.A, w.B, w.Xi, w.Xt, w.wts)
        F1, G1 = eng.eval(theta)
    assert F1 == F0 and np.array_equal(G1, G0)


# ---- 4. batches, fom, device pointers, groups -----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C3", "C4", "exact"])
def test_batches_fom_and_device_pointers(qoc, cfg):
    import torch
    kw = {}
    if cfg == "C3":
        w = qoc.workloads.config("C3", E=8, N=100)
    elif cfg == "C4":
        w = qoc.workloads.config("C4", E=3, N=12)
    else:                                                    # the arrays of a batch run one behind the other
        w, kw = sized(qoc, 4, "UnitaryGate", 50), dict(variant=1, gradient="exact", objective="c1")
    phi, x0, _ = draw(w, 6, 51)
    M = phi.shape[1]
    rng = np.random.default_rng(52)
    thetas = rng.uniform(-0.5, 0.5, (3, w.K, M))
    with engine(qoc, w, max_batch=3, **kw) as eng:
        eng.set_basis(phi, x0)
        eng.set_penalties(0.2, 0.1)
        single = [eng.eval(th) for th in thetas]
        Fb, Gb = eng.eval_batch(thetas)
        F2, G2 = eng.eval_batch(thetas[:2])
        foms = [eng.fom(th) for th in thetas]
        fom_names = eng.kernel_names()
        fom_b, mF = eng.fom(thetas, members=True) if cfg == "C3" else (eng.fom(thetas), None)
        td = torch.as_tensor(np.ascontiguousarray(thetas[1].T), device="cuda:0")
        fg = torch.zeros(w.K * M + 1, dtype=torch.float64, device="cuda:0")
        eng.eval_device(td.data_ptr(), fg.data_ptr(), torch.cuda.current_stream(0).cuda_stream)
        torch.cuda.synchronize(0)
        h = fg.cpu().numpy()
        F_after, G_after = eng.eval(thetas[1])               # host path right behind the device path
        tb = torch.as_tensor(np.ascontiguousarray(np.swapaxes(thetas, 1, 2)), device="cuda:0")
        fgb = torch.zeros(3 * (w.K * M + 1), dtype=torch.float64, device="cuda:0")
        eng.eval_batch_device(3, tb.data_ptr(), fgb.data_ptr(), torch.cuda.current_stream(0).cuda_stream)
        torch.cuda.synchronize(0)
        hb = fgb.cpu().numpy().reshape(3, -1)
        if cfg == "C3":
            _, mF1 = eng.fom(thetas[1], members=True)
            x1 = eng.controls(thetas[1])
    assert Gb.shape == (3, w.K, M)
    for b in range(3):                                       # entry b of a batch = the single call, bit for bit
        assert Fb[b] == single[b][0] and np.array_equal(Gb[b], single[b][1]), b
        assert hb[b, -1] == Fb[b] and np.array_equal(hb[b, :-1].reshape(M, w.K).T, Gb[b]), b
    assert np.array_equal(F2, Fb[:2]) and np.array_equal(G2, Gb[:2])
    assert h[-1] == single[1][0] and np.array_equal(h[:-1].reshape(M, w.K).T, single[1][1])
    assert F_after == single[1][0] and np.array_equal(G_after, single[1][1])
    if cfg == "C3":                                          # fast path (tests/test_gpu_fom.py: close at 1e-10, fast kernels ran)
        assert any(k in ("fom_lane_kernel", "fom_pair_kernel") for k in fom_names), fom_names
        assert fom_names[0] == "basis_expand_kernel" and not any(k.startswith("sweep_") for k in fom_names), fom_names
        for b in range(3):
            assert abs(foms[b] - single[b][0]) <= 1e-10 * max(1.0, abs(single[b][0])), b
            assert fom_b[b] == foms[b]
        # member_F stays in slice space: the members' unweighted F_k of the physical pulse, no penalty
        with engine(qoc, w) as ref:
            _, mF_ref = ref.fom(x1, members=True)
        assert np.array_equal(mF1, mF_ref)
        assert mF.shape == (3, w.E) and np.abs(mF[1] - mF_ref).max() <= 1e-10 * max(1.0, np.abs(mF_ref).max())
    else:                                                    # fallback: the full evaluation's F bit for bit
        for b in range(3):
            assert foms[b] == single[b][0] and fom_b[b] == single[b][0], b


def _run_ranks(tmp_path, E, N, data):
    out, inp = str(tmp_path / "basis"), str(tmp_path / "basis_in.npz")
    np.savez(inp, **data)
    port = 29600 + (os.getpid() + 23) % 300
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "workers", "ipc_basis_rank.py"), out, str(E), str(N), inp]
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return [np.load(f"{out}.rank{r}.npz") for r in range(2)]


def test_groups_and_mailbox_ranks_project_the_summed_row(qoc, tmp_path, monkeypatch):
    """A device_ids = [0, 0] peer-sum group and two processes exchanging through mailboxes on the one GPU: the same shards, the
    same rows, the same order of summation, one projection of the complete row -- the same bits; against the single-device
    context, the comparison tests/test_gpu_collective.py / test_gpu_ipc.py make between sharded and unsharded evaluations
    (assert_parity at 1e-10).  The penalties are set everywhere and counted once."""
    w = qoc.workloads.config("C3", E=10, N=60)
    phi, x0, _ = draw(w, 8, 53)
    rng = np.random.default_rng(54)
    thetas = rng.uniform(-0.5, 0.5, (3, w.K, 8))
    amp, var = np.linspace(0.3, 0.9, w.K), np.linspace(0.8, 0.2, w.K)
    with engine(qoc, w) as eng:
        eng.set_penalties(amp, var)
        eng.set_basis(phi, x0)
        one = [eng.eval(th) for th in thetas]
    group = {}
    for mode in ("0", "1"):                                  # arrive-and-sum is the slice-mode default; parameter mode sums in stream order
        monkeypatch.setenv("GRAPE_GROUP_STREAM_SUM", mode)
        with engine(qoc, w, devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM, max_batch=3) as eng:
            eng.set_penalties(amp, var)
            eng.set_basis(phi, x0)
            group[mode] = [eng.eval(th) for th in thetas]
            names = eng.kernel_names()
            xg = eng.controls(thetas[0])
            Fb, Gb = eng.eval_batch(thetas)
            fom = eng.fom(thetas[2])
            x_min, info = eng.lbfgs(thetas[0], iterations=3)
        assert names[0] == "basis_expand_kernel" and names[-1] == "basis_project_kernel", names
        for b in range(3):
            assert Fb[b] == group[mode][b][0] and np.array_equal(Gb[b], group[mode][b][1])
        assert fom == group[mode][2][0] and x_min.shape == (w.K, 8) and info["minimum"] < group[mode][0][0]
    monkeypatch.delenv("GRAPE_GROUP_STREAM_SUM")
    for a, b in zip(group["0"], group["1"]):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for (Fg, Gg), (F1, G1) in zip(group["0"], one):
        assert_parity(Fg, Gg, F1, G1, w.n, what="two shards against one device")
    res = _run_ranks(tmp_path, w.E, w.N, dict(phi=phi, x0=x0, thetas=thetas, amp=amp, var=var))
    assert all(str(r["collective"]) == "ipc" for r in res), [str(r["error"]) for r in res]
    for r in res:
        assert np.array_equal(r["x"], xg)
        assert str(r["names"]).startswith("basis_expand_kernel") and str(r["names"]).endswith("ipc_allreduce_kernel;basis_project_kernel")
        for i in range(3):
            assert float(r["F"][i]) == group["0"][i][0] and np.array_equal(r["G"][i], group["0"][i][1]), i


# ---- 5. grape_lbfgs in parameter mode -------------------------------------------------------------------------------------
def _lbfgs_case(qoc, name):
    if name == "c3_state_transfer":
        w = qoc.workloads.config("C3", E=16, N=60)
        rho0 = np.zeros((4, 4), complex)
        rho0[0, 0] = 1
        psi = np.array([1, 1j, -1, 0.5]) / np.linalg.norm([1, 1j, -1, 0.5])
        Xi = np.broadcast_to(rho0, (w.E, 4, 4)).copy()
        Xt = np.broadcast_to(np.outer(psi, psi.conj()), (w.E, 4, 4)).copy()
        return ("StateTransfer", w.A, w.B, Xi, Xt, w.wts, w.T, w.N), w.x, w
    w = qoc.workloads.reference_ensemble("StateTransfer", 5, 25, 5.0)
    return (w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N), w.x, w


@pytest.mark.parametrize("case", ["reference_2x2", "c3_state_transfer"])
def test_lbfgs_iterates_match_the_host_restatement_in_parameter_mode(qoc, case):
    """grape_lbfgs(line_search = 1) over theta against oracle/optim_lbfgs.py driven with the COMPOSED objective -- a context in
    slice mode, expansion and projection in NumPy -- iteration by iteration with the comparison and the bars of
    tests/test_gpu_lbfgs.py::test_iterates_match_the_host_restatement: accepted step length to 1e-6, iterate to 1e-9,
    evaluations per iteration equal."""
    from oracle import optim_lbfgs
    args, x_guess, w = _lbfgs_case(qoc, case)
    phi = qoc.fourier_basis(w.N, w.T, 2 * np.pi / w.T * np.array([0.5, 1.0, 1.5, 2.0]))
    x0 = np.array(x_guess, dtype=np.float64)
    theta0 = np.zeros((w.K, phi.shape[1]))
    n_it = 10

    def composed(theta):
        F, Gx = ref_eng.eval(x0 + theta @ phi.T)
        return F, Gx @ phi

    with qoc.GrapeEngine(*args) as ref_eng:
        ref = optim_lbfgs.lbfgs(composed, theta0, iterations=n_it)
    with qoc.GrapeEngine(*args) as eng:
        eng.set_basis(phi, x0)
        compare_lbfgs_iterates(eng, ref, theta0, n_it, case, min_compared=8)


# ---- 6. solve() over Fourier coefficients ---------------------------------------------------------------------------------
def _problem(qoc, sys_type, N, T):
    wl = qoc.workloads
    ug = sys_type == "UnitaryGate"
    return qoc.Problem(B=[wl.Sx, wl.Sy], A=wl.Sz, Xi=wl.U_init if ug else wl.rho_init,
                       Xt=wl.U_fin if ug else wl.rho_fin, T=T, n_controls=2, guess=wl.controls(2, N),
                       sys_type=qoc.UnitaryGate() if ug else qoc.StateTransfer())


@pytest.mark.parametrize("sys_type", ["StateTransfer", "UnitaryGate"])
@pytest.mark.parametrize("optimizer", ["host", "device"])
def test_solve_over_fourier_coefficients(qoc, sys_type, optimizer):
    """The reference's single-problem testsets (test/state_transfer_tests.jl:4-37, test/unitary_gate_tests.jl:3-37; N = 10,
    T = 1) with GRAPE(basis=fourier_basis(...)), eight columns at the frequencies 2 pi / T x (0.5, 1, 1.5, 2), the problem's
    guess as basis_offset.  The floor is not a constant: the slice-mode host-optimiser run on the same problem gives the
    optimum x*, its least-squares projection onto the basis is evaluated in slice mode, and the parameter-mode run -- which
    searches the space that projection lies in -- must end no higher.
    Recorded on an MI355X (slice-mode minimum / F of its projection / parameter-mode minimum, host and device optimiser):
      StateTransfer   0.7499999999999997 / 0.7500000000019371 / 0.7500000000000004 (host), 0.7499999999999998 (device)
      UnitaryGate    -4.000000000000025  / -3.999999999946345 / -3.9999999999999964 (host), -3.999999999999993 (device)
    (the guess itself gives 0.998315 and -0.242572)."""
    N, T = 10, 1.0
    prob = _problem(qoc, sys_type, N, T)
    guess = np.asarray(prob.guess, dtype=np.float64)
    phi = qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0, 1.5, 2.0]))
    slice_sol = qoc.solve(prob, qoc.GRAPE(n_slices=N))
    theta_proj = np.linalg.lstsq(phi, (slice_sol.opti_pulses - guess).T, rcond=None)[0].T
    with qoc.api.make_engine(prob, qoc.GRAPE(n_slices=N)) as eng:
        F_proj = eng.eval(guess + theta_proj @ phi.T)[0]
        F_guess = eng.eval(guess)[0]
    sol = qoc.solve(prob, qoc.GRAPE(n_slices=N, basis=phi, basis_offset=guess, optimizer=optimizer))
    print(f"{sys_type} / {optimizer}: slice-mode minimum {slice_sol.result.minimum!r}, its projection {F_proj!r}, "
          f"parameter mode {sol.result.minimum!r} (guess {F_guess!r})")
    assert isinstance(sol, qoc.SolutionResult)
    assert sol.parameters.shape == (2, 8) and sol.opti_pulses.shape == (2, N) and sol.fidelity == sol.result.minimum
    x_np, tol = expand(phi, guess, sol.parameters)
    assert np.all(np.abs(sol.opti_pulses - x_np) <= tol)     # opti_pulses is the physical pulse of `parameters`
    assert slice_sol.parameters is None
    assert sol.result.minimum <= F_proj


def test_solve_an_ensemble_over_a_basis(qoc):
    wl = qoc.workloads
    N, T = 25, 5.0
    prob = _problem(qoc, "StateTransfer", N, T)
    ens = qoc.EnsembleProblem(prob=prob, n_ens=5, A_g=lambda k: (k - 2.5) / 2.5 * wl.Sz * 5, B_g=lambda k: [wl.Sx, wl.Sy],
                              XiG=lambda k: wl.rho_init, XtG=lambda k: wl.rho_fin if k % 2 else wl.rho_init,
                              wts=np.ones(5) / 5)
    phi = qoc.fourier_basis(N, T, 2 * np.pi / T * np.array([0.5, 1.0, 1.5, 2.0]))
    for optimizer in ("host", "device"):
        sol = qoc.solve(ens, qoc.GRAPE(n_slices=N, basis=phi, optimizer=optimizer, optim_options={"iterations": 30}))
        assert isinstance(sol, qoc.EnsembleSolutionResult) and sol.parameters.shape == (2, 8) and sol.opti_pulses.shape == (2, N)
        with qoc.api.make_engine(ens, qoc.GRAPE(n_slices=N)) as eng:
            F_start = eng.eval(np.linalg.lstsq(phi, np.asarray(prob.guess, float).T, rcond=None)[0].T @ phi.T)[0]
            F_end = eng.eval(sol.opti_pulses)[0]
        assert F_end == sol.result.minimum and sol.result.minimum < F_start


# ---- 7. errors ------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_previous_basis_in_force(qoc):
    w = qoc.workloads.config("C3", E=8, N=60)
    phi, x0, theta = draw(w, 5, 55)
    pf, xf = np.ascontiguousarray(phi.T), np.ascontiguousarray(x0.T)
    with engine(qoc, w) as eng:
        eng.set_basis(phi, x0)
        F0, G0 = eng.eval(theta)
        lib, h, p = eng._lib, eng._h, lambda a: a.ctypes.data
        big = np.ones((w.N + 1) * w.N)
        assert lib.grape_set_basis(h, w.N + 1, 1, p(big), None) == -1         # M outside 1..N
        assert lib.grape_set_basis(h, -1, 1, p(pf), None) == -1
        assert lib.grape_set_basis(h, 5, 2, p(np.ones(2 * 5 * w.N)), None) == -1          # n_bases outside {1, K}; K = 4
        assert lib.grape_set_basis(h, 5, 0, p(pf), None) == -1
        for bad in (np.nan, np.inf):
            q = pf.copy()
            q[2, 7] = bad
            assert lib.grape_set_basis(h, 5, 1, p(q), p(xf)) == -1
            assert "phi" in lib.grape_last_error(h).decode()
            y = xf.copy()
            y[3, 1] = -bad
            assert lib.grape_set_basis(h, 5, 1, p(pf), p(y)) == -1
            assert "x0" in lib.grape_last_error(h).decode()
        assert lib.grape_get_controls(h, None, None) == -1
        F1, G1 = eng.eval(theta)
        assert F1 == F0 and np.array_equal(G1, G0) and eng.n_params == 5
        for bad in (np.zeros((w.K, w.N)), np.zeros((5, w.K)), np.zeros(5 * w.K)):          # theta of the wrong shape: Python refuses
            for call in (eng.eval, eng.fom, eng.lbfgs, eng.controls):
                with pytest.raises(ValueError):
                    call(bad)
        with pytest.raises(ValueError):
            eng.eval_batch(np.zeros((1, w.K, w.N)))
        with pytest.raises(ValueError):
            eng.set_basis(np.zeros((w.N + 1, 3)))
        with pytest.raises(qoc.GrapeError):
            eng.set_basis(np.full((w.N, 3), np.nan))
        assert eng.n_params == 5 and eng.eval(theta)[0] == F0


# ---- 8. what else the header promises ---------------------------------------------------------------------------------------
def test_ladder_search_probes_batches_of_theta(qoc):
    """grape_lbfgs line_search = "ladder" in parameter mode: every launch evaluates a batch of `probes` trial points theta
    (batched expansion, batched projection) -- on one device and on a two-shard group, which must walk the same iterates
    (the comparison of tests/test_gpu_ipc.py::test_ladder_search_on_a_group_with_batched_probes)."""
    w = qoc.workloads.reference_ensemble("StateTransfer", 5, 25, 5.0)
    phi = qoc.fourier_basis(w.N, w.T, 2 * np.pi / w.T * np.array([0.5, 1.0, 1.5, 2.0]))
    theta0 = np.zeros((w.K, phi.shape[1]))
    runs = []
    for kw in ({}, dict(devices=[0, 0], flags=qoc.engine.FLAG_GROUP_PEER_SUM)):
        with engine(qoc, w, max_batch=4, **kw) as eng:
            eng.set_basis(phi, w.x)
            F0 = eng.eval(theta0)[0]
            th, info = eng.lbfgs(theta0, iterations=10, line_search="ladder", probes=4)
            F_end = eng.eval(th)[0]
            names = eng.kernel_names()
        assert info["probes"] == 4 and info["line_search"] == 2 and th.shape == theta0.shape
        assert names[0] == "basis_expand_kernel" and names[-1] == "basis_project_kernel"
        assert abs(info["minimum"] - F_end) <= 1e-12 and info["minimum"] < F0
        runs.append((th, info))
    (t1, i1), (t2, i2) = runs
    assert i1["iterations"] == i2["iterations"] and i1["evaluations"] == i2["evaluations"]
    assert abs(i1["minimum"] - i2["minimum"]) <= 1e-10 and np.abs(t1 - t2).max() <= 1e-7


@pytest.mark.parametrize("cfg", ["C3", "C4"])
def test_member_results_and_trajectory_stay_in_slice_space(qoc, cfg):
    w = qoc.workloads.config("C3", E=8, N=60) if cfg == "C3" else qoc.workloads.config("C4", E=3, N=12)
    phi, x0, theta = draw(w, 5, 56)
    kw = dict(member_results=True, flags=qoc.engine.FLAG_KEEP_COSTATES)
    with engine(qoc, w, **kw) as eng:
        eng.set_basis(phi, x0)
        x = eng.controls(theta)
        eng.eval(theta)
        foms, grads = eng.member_results()
        P, X, L = eng.trajectory(w.E - 1, costates=True)
    with engine(qoc, w, **kw) as ref:
        ref.eval(x)
        foms_r, grads_r = ref.member_results()
        Pr, Xr, Lr = ref.trajectory(w.E - 1, costates=True)
    assert grads.shape == (w.E, w.K, w.N) and P.shape == (w.N, w.n, w.n)
    assert np.array_equal(foms, foms_r) and np.array_equal(grads, grads_r)
    assert np.array_equal(P, Pr) and np.array_equal(X, Xr) and np.array_equal(L, Lr)


def test_more_coefficients_than_one_tile_of_the_expansion(qoc):
    """M = 300 > 256: basis_expand_kernel passes the coefficients through LDS in two tiles; many projection workgroups."""
    w = qoc.workloads.config("C3", E=4, N=600)
    phi, x0, theta = draw(w, 300, 57)
    chain_rule(qoc, w, phi, x0, theta, "M = 300")
    phi, x0, theta = draw(w, 600, 58, per_control=True)
    chain_rule(qoc, w, phi, x0, theta, "M = N = 600, one basis per control")
