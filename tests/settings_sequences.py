"""Random walks over the settings that live on a context -- grape_set_penalties, grape_set_basis, grape_set_running_cost, the
gradient-free grape_eval_fom -- across grape_set_operators re-uploads that flip the data flow, and the reference they are
held to.  Shared by test_gpu_settings_soak.py (runs the walks on the device), test_settings_sequences_host.py (checks on the
CPU that the walks cover what they claim) and tools/soak_settings.py (long runs).  No test functions here.

  composed_reference   oracle.ensemble_eval + penalty_ref (test_penalties_host.py) + running_cost_ref (rc_reference.py), then
                       parameter mode in NumPy: x = x0 + theta phi', G_theta = G_x phi.  No device result enters it.
  draw_context / draw_steps   pure functions of the generator state: they never touch the library.
  State                what the settings are after each step -- the walk both tests make.
  run_context          one context and its steps on the device, every check through conftest.assert_parity.
  compare_lbfgs_iterates   the iterate-by-iterate comparison of grape_lbfgs with oracle/optim_lbfgs.py.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rc_reference as rcr  # noqa: E402
from conftest import assert_parity  # noqa: E402
from test_penalties_host import penalty_ref  # noqa: E402

SEEDS = range(24)
CONTEXTS_PER_SEED = 6
U = 2.0 ** -53
SETTING_OPS = ("upload", "pen_on", "pen_change", "pen_off", "basis_on", "basis_per_control", "basis_off", "rc_on", "rc_change",
               "rc_off")
CHECK_OPS = ("eval", "F_only", "batch", "device", "fom", "fom_members", "fom_batch", "members", "controls")


# ---- operators ------------------------------------------------------------------------------------------------------------
def _sparsify(rng, B, hermitian):
    """a few entries per control operator, as tools/soak_api.py draws them (the pattern stays symmetric)"""
    n = B.shape[-1]
    for k in range(B.shape[0]):
        for c in range(B.shape[1]):
            mask = np.zeros((n, n), bool)
            for _ in range(int(rng.integers(1, 2 * n))):
                a, b = rng.integers(0, n, 2)
                mask[a, b] = mask[b, a] = True
            B[k, c] = B[k, c] * mask
    return B


def full_operators(rng, ctx):
    """UnitaryGate n x m problem at the scales of rc_reference.random_problem; the target a perturbed-pulse propagation away"""
    herm, sparse = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    return _full_operators(rng, ctx, herm, sparse)


def _full_operators(rng, ctx, herm, sparse):
    n, m, K, E, N, T = (ctx[k] for k in ("n", "m", "K", "E", "N", "T"))
    A, B, Xi, wts = rcr.random_problem(rng, n, m, K, E, hermitian=herm, scale=ctx["scale"])
    if sparse:
        B = _sparsify(rng, B, herm)
    wts = wts * N                                         # dG/dx[c,t] is of order dt = T / N: weights that keep it of order 1
    xg = rng.uniform(-1, 1, (K, N))
    Xt = rcr.perturbed_target(A, B, Xi, xg, T, rng, ctx["variant"])
    return dict(A=A, B=B, Xi=Xi, Xt=Xt, wts=wts, herm=herm, sparse=sparse)


def partial_operators(rng, ctx):
    """any system type and size, the operators of tools/soak_api.py: non-Hermitian means a general complex matrix"""
    n, K, E = ctx["n"], ctx["K"], ctx["E"]
    herm = bool(rng.integers(0, 2)) and n > 1            # (n = 1: Hermitian controls only turn a phase, G would be 0)
    mixed, sparse = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    sand = ctx["sys_type"] != "UnitaryGate"

    def mat(h):
        M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        return (M + M.conj().T) / 2 if h else M
    g = min(1.0, 4.0 / n)
    A = np.array([mat(herm) for _ in range(E)]) * 0.6 * g
    B = np.array([[mat(herm) for _ in range(K)] for _ in range(E)]) * 0.4 * g
    if sparse and n > 1:
        B = _sparsify(rng, B, herm)

    def vec():
        v = rng.standard_normal((n, 1)) + 1j * rng.standard_normal((n, 1))
        return v / np.linalg.norm(v)

    def dens():
        if mixed:
            return sum(p * (lambda v: v @ v.conj().T)(vec()) for p in (0.5, 0.3, 0.2))
        v = vec()
        return v @ v.conj().T
    if sand:
        Xi, Xt = np.array([dens() for _ in range(E)]), np.array([dens() for _ in range(E)])
    else:
        Xi = np.array([np.eye(n, dtype=complex)] * E)
        Xt = np.array([np.linalg.qr(mat(False))[0] for _ in range(E)])
    wts = rng.uniform(0.2, 1.0, E) * ctx["N"]             # (dG/dx[c,t] is of order dt = T / N)
    return dict(A=A, B=B, Xi=Xi, Xt=Xt, wts=wts, herm=herm, sparse=sparse)


# ---- contexts and steps ---------------------------------------------------------------------------------------------------
def draw_context(rng):
    """One context: its shape, its launch geometry, its first operators and a pool of three pulses."""
    full = bool(rng.random() < 0.7)
    ctx = dict(full=full, variant=int(rng.integers(0, 2)), max_batch=int(rng.choice([1, 3])), S=0, W=0, kernel=None,
               budget=None, chunked=False)
    ctx["K"] = int(rng.choice([1, 2, 3, 5]))
    ctx["E"] = int(rng.choice([1, 2, 3, 7]))
    ctx["N"] = int(rng.choice([1, 3, 8, 20, 65, 130]))
    long_T = bool(rng.random() < 1.0 / 6.0)
    ctx["T"] = 24.0 if long_T else float(rng.uniform(0.3, 1.5))
    ctx["scale"] = float(rng.uniform(0.3, 0.5)) if long_T else float(rng.uniform(0.5, 1.0))
    if full:
        ctx["sys_type"] = "UnitaryGate"
        n = ctx["n"] = int(rng.choice([2, 3, 4]))
        ctx["m"] = int(rng.integers(1, n + 1))
        ctx["kernel"] = "lane" if n == 3 else str(rng.choice(["lane", "pair"]))
        if rng.random() < 0.3:                            # forced geometries, as test_gpu_running_cost.py::SHAPES
            ctx["S"], ctx["W"] = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        if rng.random() < 0.25:
            # Member-chunked.  Seven members; W forced so that a workgroup takes two of them (four waves per lane-kernel
            # workgroup, eight per pair-kernel one), the granule of a chunk.  The budget holds two and a half members'
            # propagators and states: chunks of two in the general flow, of four in the unitary one (one array), 7 = 2+2+2+1
            # = 4+3 -- chunked, and the last chunk short, whichever flow an upload selects.
            ctx["chunked"], ctx["E"], ctx["max_batch"] = True, 7, 3
            ctx["W"] = 2 if ctx["kernel"] == "lane" else 4
            cpw = 64 if ctx["kernel"] == "lane" else 32
            ctx["N"] = min(ctx["N"], 65)
            S = max(ctx["S"], -(-ctx["N"] // (cpw * ctx["W"])))
            ctx["budget"] = int(2.5 * 2 * 16 * S * n * n * cpw * ctx["W"])
        if ctx["N"] == 130 and ctx["E"] == 7:             # (the running-cost reference is a double sum over the slices)
            ctx["N"] = 65
    else:
        small = bool(rng.integers(0, 2))
        if small:
            ctx["sys_type"] = str(rng.choice(["StateTransfer", "CoherenceTransfer"]))
            ctx["n"] = int(rng.choice([2, 3, 4]))
        else:
            ctx["sys_type"] = str(rng.choice(["UnitaryGate", "StateTransfer", "CoherenceTransfer"]))
            ctx["n"] = int(rng.choice([1, 8, 16, 40]))
            if ctx["n"] == 1:                             # (a scalar commutes with every state: the sandwich's G is 0 exactly)
                ctx["sys_type"] = "UnitaryGate"
            if ctx["n"] >= 16:
                ctx["N"] = int(rng.choice([1, 3, 8, 12]))
                ctx["E"] = min(ctx["E"], 3)
        ctx["m"] = ctx["n"]
        ctx["T"] = float(rng.uniform(0.3, 1.5))           # (T = 24 belongs to the running cost's contexts)
        ctx["scale"] = 1.0
    ctx["ops"] = (full_operators if full else partial_operators)(rng, ctx)
    ctx["pool"] = rng.uniform(-1, 1, (3, ctx["K"], ctx["N"]))
    return ctx


def context_line(ctx):
    return (f"{'full' if ctx['full'] else 'partial'} {ctx['sys_type']} n={ctx['n']} m={ctx['m']} K={ctx['K']} E={ctx['E']} "
            f"N={ctx['N']} T={ctx['T']:.3f} v{ctx['variant']} max_batch={ctx['max_batch']} kernel={ctx['kernel']} "
            f"S={ctx['S']} W={ctx['W']} budget={ctx['budget']} herm={ctx['ops']['herm']} sparse={ctx['ops']['sparse']}")


def step_line(step):
    extra = {k: step[k] for k in ("i", "J", "kind", "M", "herm", "sparse", "offset") if k in step}
    return step["op"] + (" " + str(extra) if extra else "")


def _draw_rc(rng, ctx, Xt, J):
    n, m, E, N = ctx["n"], ctx["m"], ctx["E"], ctx["N"]
    kind = str(rng.choice(["random", "mixed", "single"]))
    R = rng.standard_normal((J, E, n, m)) + 1j * rng.standard_normal((J, E, n, m))
    if R.shape[1:] == Xt.shape:
        R[0] = Xt                                         # (term 0: the C6 / C7 probe)
    rho = rng.uniform(0.5, 1.5, (J, N)) * min(1.0, 4.0 / N)
    if kind == "mixed" and N >= 4:
        rho[:, ::3] = 0.0
        rho[:, 1::4] *= -1.0
    elif kind == "single":
        rho[:] = 0.0
        rho[:, (N - 1) // 2] = 1.7
    return dict(R=R, rho=rho, J=J, kind=kind)


def _draw_basis(rng, ctx, per_control):
    K, N = ctx["K"], ctx["N"]
    M = min(int(rng.choice([1, 4, N])), N)
    offset = bool(rng.integers(0, 2))
    phi = rng.standard_normal((K, N, M) if per_control else (N, M))
    x0 = 0.3 * rng.standard_normal((K, N)) if offset else None
    thetas = rng.uniform(-1, 1, (3, K, M)) / np.sqrt(M)
    return dict(phi=phi, x0=x0, thetas=thetas, M=M, offset=offset)


def _draw_pen(rng, K):
    amp, var = rng.uniform(0.1, 0.5, K), rng.uniform(0.05, 0.3, K)
    which = int(rng.integers(0, 4))
    if which == 0:
        return dict(amp=amp, var=None)
    if which == 1:
        return dict(amp=None, var=var)
    if K > 1:
        amp[int(rng.integers(0, K))] = 0.0
    return dict(amp=amp, var=var)


def draw_steps(rng, ctx):
    """3 to 9 steps; a check behind the last setting change, so that no change goes unobserved."""
    steps = []
    st = State(ctx)
    n_steps = int(rng.integers(3, 10))
    checks = ["eval", "eval", "F_only", "batch", "batch", "device", "fom", "fom", "fom_members", "fom_batch", "members"]
    while len(steps) < n_steps:
        last = len(steps) == n_steps - 1
        if not last and rng.random() < (0.75 if 3 * len(steps) < n_steps else 0.45):
            menu = ["upload", "upload", "rc_on", "rc_on", "basis_on", "pen_on"]
            if st.rc is not None:
                menu += ["upload", "upload", "rc_change", "rc_off"]
                menu += ["pen_on"] * (3 if st.pen is None else 0) + ["basis_on"] * (3 if st.basis is None else 0)
            if st.pen is not None:
                menu += ["upload", "pen_change", "pen_off"]
            if st.basis is not None:
                menu += ["basis_off", "basis_off", "basis_per_control"]
            else:
                menu += ["basis_per_control"]
            op = str(rng.choice(menu))
            step = dict(op=op)
            if op == "upload":
                if ctx["full"]:
                    herm, sparse = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
                    if st.rc is not None and rng.random() < 0.6:
                        herm = not st.ops["herm"]        # the flip a standing running cost has to survive
                    step["ops"] = _full_operators(rng, ctx, herm, sparse)
                else:
                    step["ops"] = partial_operators(rng, ctx)
                step["herm"], step["sparse"] = step["ops"]["herm"], step["ops"]["sparse"]
            elif op in ("pen_on", "pen_change"):
                step.update(_draw_pen(rng, ctx["K"]))
            elif op in ("basis_on", "basis_per_control"):
                step.update(_draw_basis(rng, ctx, op == "basis_per_control"))
            elif op in ("rc_on", "rc_change"):
                J = int(rng.choice([1, 2, 3, 4, 4]))
                if op == "rc_change" and st.rc is not None:
                    J = int(rng.choice([j for j in (1, 2, 3, 4) if j != st.rc["J"]]))
                step.update(_draw_rc(rng, ctx, st.ops["Xt"], J))
        else:
            menu = list(checks)
            if st.rc is not None and ctx["max_batch"] == 3 and (ctx["chunked"] or not st.ops["herm"]):
                menu += ["batch"] * 4
            if st.basis is not None:
                menu += ["controls", "controls"]
            step = dict(op=str(rng.choice(menu)), i=int(rng.integers(0, 3)))
        st.apply(step)
        steps.append(step)
    return steps


class State:
    """The settings in force after the steps applied so far.  A running cost on a partial-class context is refused by the
    library, so it never comes into force here either."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.ops, self.gen = ctx["ops"], 0
        self.pen = self.basis = self.rc = None
        self.rc_gen = 0
        self.refused = False                              # the last step was a refused running cost

    def apply(self, step):
        op = step["op"]
        self.refused = False
        if op == "upload":
            self.ops, self.gen = step["ops"], self.gen + 1
        elif op in ("pen_on", "pen_change"):
            self.pen = dict(amp=step["amp"], var=step["var"])
        elif op == "pen_off":
            self.pen = None
        elif op in ("basis_on", "basis_per_control"):
            self.basis = step
        elif op == "basis_off":
            self.basis = None
        elif op in ("rc_on", "rc_change"):
            if self.ctx["full"]:
                self.rc, self.rc_gen = step, self.rc_gen + 1
            else:
                self.refused = True
        elif op == "rc_off":
            self.rc = None

    def pulses(self):
        """what the evaluation calls take: the pool of pulses, or of coefficient arrays in parameter mode"""
        return self.ctx["pool"] if self.basis is None else self.basis["thetas"]

    def expand(self, theta):
        """(x, element-wise rounding bound) of a coefficient array: the bound of test_gpu_basis.py::expand"""
        if self.basis is None:
            return np.asarray(theta), np.zeros_like(theta)
        phi, x0 = self.basis["phi"], self.basis["x0"]
        if phi.ndim == 2:
            x, mag = theta @ phi.T, np.abs(theta) @ np.abs(phi).T
        else:
            x = np.array([theta[c] @ phi[c].T for c in range(theta.shape[0])])
            mag = np.array([np.abs(theta[c]) @ np.abs(phi[c]).T for c in range(theta.shape[0])])
        if x0 is not None:
            x, mag = x0 + x, np.abs(x0) + mag
        return x, 2 * phi.shape[-1] * U * mag

    def project(self, G):
        if self.basis is None:
            return G
        phi = self.basis["phi"]
        if phi.ndim == 2:
            return G @ phi
        return np.array([G[c] @ phi[c] for c in range(G.shape[0])])


# ---- the reference --------------------------------------------------------------------------------------------------------
_CACHE = {}


def composed_reference(oracle, ops, x, T, variant, penalties=None, rc=None, sys_type="UnitaryGate", key=None):
    """(F, G_x, parts): the plain evaluation + penalties + running cost of the pulse x (K, N).  parts = dict of the three
    (F, G) pairs and the oracle's per-member values.  key: (context id, operator generation, running-cost generation) --
    with it the oracle's and the double sum's results are kept per (key, x bytes); without it nothing is cached."""
    x = np.ascontiguousarray(x, dtype=np.float64)

    def cached(kind, k, make):
        if key is None:
            return make()
        kk = (kind,) + k + (x.tobytes(),)
        if kk not in _CACHE:
            val = make()
            for a in val:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            _CACHE[kk] = val
        return _CACHE[kk]

    args = (ops["A"], ops["B"], ops["Xi"], ops["Xt"], ops["wts"])
    F0, G0, mF, mG = cached("plain", key[:2] if key else (), lambda: oracle.ensemble_eval(sys_type, *args, x, T, variant,
                                                                                            per_member=True))
    parts = dict(plain=(F0, G0), members=(mF, mG))
    F, G = F0, np.array(G0)
    if penalties is not None:
        Fp, Gp = penalty_ref(x, penalties["amp"], penalties["var"])
        parts["pen"] = (Fp, Gp)
        F, G = F + Fp, G + Gp
    if rc is not None:
        FJ, GJ = cached("rc", key if key else (), lambda: rcr.running_cost_ref(ops["A"], ops["B"], ops["Xi"], ops["wts"], x, T,
                                                                              rc["R"], rc["rho"], variant))
        parts["rc"] = (FJ, GJ)
        F, G = F + FJ, G + GJ
    return F, G, parts


def state_reference(oracle, st, theta, cid=None):
    """(F, G in the space the calls work in, parts, x) of the state's settings at the pulse / coefficient array theta"""
    ctx = st.ctx
    x, _ = st.expand(theta)
    key = None if cid is None else (cid, st.gen, st.rc_gen)
    F, G, parts = composed_reference(oracle, st.ops, x, ctx["T"], ctx["variant"], st.pen, st.rc, ctx["sys_type"], key)
    return F, st.project(G), parts, x


# ---- on the device --------------------------------------------------------------------------------------------------------
def _refused_rc(qoc, eng, step):
    try:
        eng.set_running_cost(step["R"], step["rho"])
    except qoc.GrapeError as exc:
        assert exc.status == -2, f"running cost refused with status {exc.status}, not -2: {exc}"
        return
    raise AssertionError("grape_set_running_cost was not refused on a context it does not serve")


def run_context(qoc, oracle, ctx, steps, setenv, cid, log):
    """Creates the context and walks the steps; every check against the reference.  setenv(name, value or None) sets the
    environment the way the caller wants it undone (monkeypatch in the suite).  log(line) receives each step before it runs.
    Returns the number of checked operations."""
    import torch
    setenv("GRAPE_SMALL_KERNEL", ctx["kernel"])
    setenv("GRAPE_MAX_WORKSPACE_BYTES", None if ctx["budget"] is None else str(ctx["budget"]))
    n, K, N, E, T, mb = ctx["n"], ctx["K"], ctx["N"], ctx["E"], ctx["T"], ctx["max_batch"]
    st = State(ctx)
    o = ctx["ops"]
    checks = 0
    log("context: " + context_line(ctx))
    with qoc.GrapeEngine(ctx["sys_type"], o["A"], o["B"], o["Xi"], o["Xt"], o["wts"], T, N, variant=ctx["variant"],
                         member_results=True, max_batch=mb, slices_per_lane=ctx["S"], waves_per_member=ctx["W"]) as eng:
        def plan():
            info = eng.info
            if ctx["full"]:
                assert info["unitary_flow"] == (1 if st.ops["herm"] else 0), info
                assert info["lane_pair"] == (1 if ctx["kernel"] == "pair" else 0), info
            if ctx["chunked"]:
                assert 0 < info["member_chunk"] < E, info["member_chunk"]
        plan()
        for si, step in enumerate(steps):
            op = step["op"]
            log(f"step {si}: {step_line(step)}")
            was_refused = False
            if op == "upload":
                so = step["ops"]
                eng.set_operators(so["A"], so["B"], so["Xi"], so["Xt"], so["wts"])
            elif op in ("pen_on", "pen_change"):
                eng.set_penalties(step["amp"], step["var"])
            elif op == "pen_off":
                eng.set_penalties(None, None)
            elif op in ("basis_on", "basis_per_control"):
                eng.set_basis(step["phi"], step["x0"])
            elif op == "basis_off":
                eng.set_basis(None)
            elif op in ("rc_on", "rc_change"):
                if ctx["full"]:
                    eng.set_running_cost(step["R"], step["rho"])
                else:
                    _refused_rc(qoc, eng, step)
                    was_refused = True
            elif op == "rc_off":
                eng.set_running_cost(None)
            st.apply(step)
            if op == "upload":
                plan()
            if op in SETTING_OPS and not was_refused:
                continue
            what = f"step {si} {op}"
            if was_refused:                               # the refusal left the evaluation what it was
                op, step, what = "eval", dict(op="eval", i=si % 3), what + " refused, then eval"
            checks += 1
            th = st.pulses()[step["i"]]
            F_ref, G_ref, parts, x = state_reference(oracle, st, th, cid)
            cols = th.shape[1]
            if op == "eval":
                F, G = eng.eval(th)
                assert_parity(F, G, F_ref, G_ref, n, what=what)
            elif op == "F_only":
                F, G = eng.eval(th, want_G=False)
                assert G is None
                assert_parity(F, G_ref, F_ref, G_ref, n, what=what)
            elif op == "device":
                xd = torch.as_tensor(np.ascontiguousarray(th.T), device="cuda")
                fg = torch.zeros(K * cols + 1, dtype=torch.float64, device="cuda")
                eng.eval_device(xd.data_ptr(), fg.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                h = fg.cpu().numpy()
                assert_parity(h[-1], h[:-1].reshape(cols, K).T, F_ref, G_ref, n, what=what)
            elif op in ("batch", "fom_batch"):
                ths = np.array([st.pulses()[(step["i"] + b) % 3] for b in range(mb)])
                refs = [state_reference(oracle, st, t, cid) for t in ths]
                if op == "batch":
                    Fs, Gs = eng.eval_batch(ths)
                    for b in range(mb):
                        assert_parity(Fs[b], Gs[b], refs[b][0], refs[b][1], n, what=f"{what} entry {b}")
                else:
                    Fs = eng.fom(ths)
                    assert Fs.shape == (mb,)
                    for b in range(mb):
                        assert_parity(Fs[b], refs[b][1], refs[b][0], refs[b][1], n, what=f"{what} entry {b}")
            elif op == "fom":
                F = eng.fom(th)
                assert_parity(F, G_ref, F_ref, G_ref, n, what=what)
            elif op == "fom_members":
                F, mF = eng.fom(th, members=True)
                assert_parity(F, G_ref, F_ref, G_ref, n, what=what)
                for k in range(E):                        # the members' unweighted F_k: no penalty, no running cost
                    assert_parity(mF[k], parts["members"][1][k], parts["members"][0][k], parts["members"][1][k], n,
                                  what=f"{what} member {k}")
            elif op == "members":
                F, G = eng.eval(th)
                assert_parity(F, G, F_ref, G_ref, n, what=what)
                foms, grads = eng.member_results()       # slice space; neither penalty nor running cost
                assert grads.shape == (E, K, N)
                for k in range(E):
                    assert_parity(foms[k], grads[k], parts["members"][0][k], parts["members"][1][k], n, what=f"{what} member {k}")
            elif op == "controls":
                x_np, tol = st.expand(th)
                xc = eng.controls(th)
                assert xc.shape == (K, N) and np.all(np.abs(xc - x_np) <= tol), f"{what}: expansion"
            else:
                raise AssertionError(f"unknown step {op}")
    return checks


def run_seed(qoc, oracle, seed, setenv, log, contexts=CONTEXTS_PER_SEED):
    """the contexts of one seed; returns (contexts walked, checked operations)"""
    rng = np.random.default_rng(1000 + seed)
    checks = 0
    for ci in range(contexts):
        ctx = draw_context(rng)
        steps = draw_steps(rng, ctx)
        checks += run_context(qoc, oracle, ctx, steps, setenv, (seed, ci), log)
    return contexts, checks


def walk_seed(seed, contexts=CONTEXTS_PER_SEED):
    """exactly the (context, steps) pairs run_seed runs"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for _ in range(contexts):
        ctx = draw_context(rng)
        out.append((ctx, draw_steps(rng, ctx)))
    return out


# ---- grape_lbfgs iterate by iterate -----------------------------------------------------------------------------------------
def compare_lbfgs_iterates(eng, ref, start, n_it, what, min_compared=8):
    """grape_lbfgs(line_search = "optim") on `eng` from `start`, re-run with 1..n_it iterations, against the trace `ref` of
    oracle/optim_lbfgs.py: the accepted step length to 1e-6, the iterate to 1e-9, the evaluations of every iteration equal --
    the bars of tests/test_gpu_lbfgs.py::test_iterates_match_the_host_restatement.  Returns the number of iterations compared."""
    xs = []
    for k in range(1, n_it + 1):
        xk, info = eng.lbfgs(start, iterations=k, line_search="optim")
        xs.append(xk)
        if info["status"] != 2:                          # converged / stopped before k iterations: the trace ends here
            break
    al, ev = eng.lbfgs_trace()
    tr = ref["trace"]
    assert len(al) == len(xs) and len(al) >= min(len(tr), n_it) and len(al) > 3
    per_dev = np.diff(np.concatenate([[1], ev]))
    per_ref = np.diff([1] + [t["evaluations"] for t in tr])
    compared = 0
    for i in range(len(al)):
        a_ref, x_ref = tr[i]["alpha"], tr[i]["x"].reshape(np.shape(start))
        print(f"{what} iteration {i}: alpha {al[i]!r} vs {a_ref!r}, |dx| = {np.abs(xs[i] - x_ref).max():.3e}, "
              f"evaluations {per_dev[i]} vs {per_ref[i]}")
        assert abs(al[i] - a_ref) <= 1e-6 * abs(a_ref), (what, i, al[i], a_ref)
        assert xs[i].shape == np.shape(start) and np.abs(xs[i] - x_ref).max() <= 1e-9 * max(1.0, np.abs(x_ref).max()), (what, i)
        compared += 1
        if per_ref[i] <= 15:
            assert per_dev[i] == per_ref[i], (what, i, list(per_dev), list(per_ref))
        else:                                            # a bisection down to eps(b): see test_gpu_lbfgs.py
            assert per_dev[i] > 30 and abs(int(per_dev[i]) - int(per_ref[i])) <= 12, (what, i, list(per_dev), list(per_ref))
            break
    assert compared >= min_compared, (what, compared)
    return compared
