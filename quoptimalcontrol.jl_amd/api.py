"""Host-side mirror of the reference's user surface for the GRAPE path.

Names, fields and argument meaning follow /root/reference so that the parity tests read like
the reference's own tests (test/state_transfer_tests.jl, test/unitary_gate_tests.jl):

  Problem(B, A, Xi, Xt, T, n_controls, guess, sys_type)        src/problems.jl:19-28
  EnsembleProblem(prob, n_ens, A_g, B_g, XiG, XtG, wts)        src/problems.jl:33-41
  StateTransfer() / UnitaryGate() / CoherenceTransfer()        src/problems.jl:8-10
  GRAPE(n_slices=..., isinplace=True, optim_options=...)       src/solve.jl:33-42
  solve(prob, alg) -> SolutionResult / EnsembleSolutionResult  src/solve.jl:63-143, :145-250
  init_ensemble(ens)                                           src/tools.jl:42-53
  C1(KT, KN)                                                   src/cost_functions.jl:13-17
  C3(u), C4(u), PenaltyFunctionals(weights, functions)         src/cost_functions.jl:29-39, :66-69
  C5(psiF, psij), C6(KT, KJ, N, D), C7(psiT, psiJ, N)          src/cost_functions.jl:44-61; on the device through
  ForbiddenStates(states, weight), EvolutionTime(weight)       GRAPE(running_costs=[...]) (grape_set_running_cost)
  dCRAB(n_slices=..., n_freq=2, n_coeff=2)                     src/dCRAB.jl:2-5, :13-89
  fourier_basis(n_slices, duration, freqs), GRAPE(basis=...)   new: gradient-based optimisation over the coefficients of
                                                               dCRAB's ansatz (or any other basis), grape_set_basis

What differs, on purpose: the body of the (F, G, x) closure is one call into libgrape_hip.so
(engine.GrapeEngine) instead of _fom_and_gradient_GRAPE!, and the L-BFGS driver is SciPy's
(the optimiser is outside the hot path; Optim.jl is a third-party dependency of the
reference).  Generator callables A_g/B_g/XiG/XtG receive the 1-based member index k, as in
Julia.
"""
from dataclasses import dataclass, field
from typing import Any, Callable, Optional

import json

import numpy as np

from .bounds import bounds_start
from .engine import GrapeEngine


class _SysType:
    name = ""

    def __repr__(self):
        return f"{self.name}()"

    def __eq__(self, other):
        return type(self) is type(other)

    def __hash__(self):
        return hash(self.name)


class StateTransfer(_SysType):
    name = "StateTransfer"


class UnitaryGate(_SysType):
    name = "UnitaryGate"


class CoherenceTransfer(_SysType):
    name = "CoherenceTransfer"


@dataclass
class Problem:
    B: Any                 # list of K control operators (n x n)
    A: Any                 # drift operator (n x n)
    Xi: Any                # initial state / operator
    Xt: Any                # target state / operator
    T: float               # pulse duration
    n_controls: int
    guess: Any             # (K, N) initial controls
    sys_type: _SysType


@dataclass
class EnsembleProblem:
    prob: Problem
    n_ens: int
    A_g: Callable[[int], Any]
    B_g: Callable[[int], Any]
    XiG: Callable[[int], Any]
    XtG: Callable[[int], Any]
    wts: Any


@dataclass
class GRAPE:
    n_slices: int
    expm_method: str = "fast"      # stored and never read, like the reference (src/solve.jl:39-41,66)
    isinplace: bool = True
    optim_options: dict = field(default_factory=dict)
    device: int = -1               # HIP device ordinal (new: the reference has no devices)
    optimizer: str = "host"        # "host": SciPy L-BFGS-B drives grape_eval (stand-in for Optim.jl on the host);
                                   # "device": grape_lbfgs, the library's device-resident L-BFGS (Hager-Zhang line search;
                                   # optim_options["line_search"]: "hagerzhang" | "optim" | "ladder")
    devices: Optional[list] = None  # HIP ordinals: the library shards the ensemble over them (grape_config.n_devices /
                                    # device_ids, as julia/GrapeHIP.jl's `devices`) and all-reduces [G, F] once per evaluation
    peer_sum: bool = False         # with `devices`: GRAPE_FLAG_GROUP_PEER_SUM (sum on the first device, ids may repeat)
    penalties: Any = None          # PenaltyFunctionals of C3 / C4 (new: the reference's solvers call none): added to the
                                   # objective on the device (grape_set_penalties); res.minimum / fidelity then include them
    basis: Any = None              # (N, M) or (K, N, M) basis functions (new; e.g. fourier_basis): the optimiser -- host or
                                   # device -- runs over the coefficients theta (K, M) of x = basis_offset + theta @ basis.T,
                                   # expanded and projected on the device (grape_set_basis).  The start is the least-squares
                                   # fit of the problem's guess; the result carries the physical pulse and `parameters`
    basis_offset: Any = None       # (K, N) pulse the expansion is added to; None: zero
    bounds: Any = None             # (lo, hi), scalars or K-vectors (new): smooth amplitude bounds on the device
                                   # (grape_set_bounds).  The optimiser -- host or device -- runs over raw variables u with
                                   # x = mid + half tanh((u - mid) / half) strictly inside (lo, hi).  The start is the inverse
                                   # map of the problem's guess, first clipped to mid +- 0.999 half (a start in saturation has
                                   # a vanishing gradient; the guess object is not modified).  With a basis the bounds apply to
                                   # the expanded pulse and the start is the fit of that raw pulse.  `opti_pulses` is the
                                   # physical pulse, `parameters` the raw variables (theta with a basis)
    running_costs: Any = None      # list of ForbiddenStates / EvolutionTime (new: the reference's C5 / C6 / C7 are called by none
                                   # of its solvers): costs on the intermediate states, added to the objective on the device
                                   # (grape_set_running_cost; n = 2..4, UnitaryGate-type problems, one device)
    running_cost_derivative: str = "first_order"   # "exact": the gradient of the running costs differentiates the sweep's own
                                   # expm evaluation per slice (grape_set_running_cost_derivative) instead of taking
                                   # dP_t/dx as (-i dt B) P_t -- what few, coarse slices need; the figure of merit's own
                                   # gradient stays the reference's first-order one (ADGRAPE: both exact)
    risk: float = 0.0              # beta of grape_set_risk (new): the optimiser -- host or device -- minimises the soft worst case
                                   # F_beta = (W / beta) log((1 / W) sum_k w_k exp(beta F_k)) over the ensemble instead of its
                                   # weighted mean; res.minimum is F_beta.  0: the mean.  One device, no running costs


@dataclass
class ADGRAPE:
    """src/solve.jl:44-52: the functional path.  The reference differentiates
    functional(x) = sum_k w_k C1(Xt_k, U Xi_k [U']) (src/solve.jl:268-361, U = pw_evolve) with Zygote; here the same
    functional and its exact gradient come from the device (objective "c1", gradient "exact")."""
    n_slices: int
    expm_method: str = "fast"
    optim_options: dict = field(default_factory=dict)
    device: int = -1
    optimizer: str = "host"
    devices: Optional[list] = None
    peer_sum: bool = False
    penalties: Any = None
    running_costs: Any = None      # list of ForbiddenStates / EvolutionTime, as GRAPE's: added to the functional on the device
                                   # with their EXACT gradient (grape_set_running_cost_derivative, which make_engine sets
                                   # before the costs: an exact-gradient context takes them in that mode only)


@dataclass
class dCRAB:
    """src/dCRAB.jl:2-5 (dCRAB_options) and :13-89: the gradient-free solver.  n_freq super-iterations; each draws one
    frequency per control in [0, 1) and minimises the functional over n_coeff coefficients per control of the ansatz
    c1 cos(w t) + c2 sin(w t) added to the current pulse, with Nelder-Mead; the pulse is updated after each.  The
    functional is the one the reference's `_solve` wrappers (:97-142) and ADGRAPE use, sum_k w_k C1(Xt_k, U Xi_k [U']),
    evaluated on the device WITHOUT its gradient (GrapeEngine.fom).  `options`: SciPy Nelder-Mead options (maxiter,
    xatol, fatol, ...); `seed`: numpy.random.default_rng(seed) draws the frequencies and the initial coefficients."""
    n_slices: int
    n_freq: int = 2
    n_coeff: int = 2
    seed: Any = None
    options: Optional[dict] = None
    device: int = -1
    devices: Optional[list] = None
    peer_sum: bool = False
    penalties: Any = None

    def __post_init__(self):
        if int(self.n_freq) < 1:
            raise ValueError("dCRAB: n_freq must be at least 1")
        if int(self.n_coeff) != 2:       # the ansatz reads coeffs[1] and coeffs[2] and nothing else (src/dCRAB.jl:26)
            raise ValueError("dCRAB: the ansatz c1 cos(w t) + c2 sin(w t) has n_coeff = 2 coefficients per control")
        if int(self.n_slices) < 1:
            raise ValueError("dCRAB: n_slices must be at least 1")


def dcrab_pulse(coeffs, freqs, n_slices, duration):
    """The pulse the ansatz of src/dCRAB.jl:26 adds: row j is c[j,0] cos(w_j t) + c[j,1] sin(w_j t) on the grid
    t = 0, dt, ..., T - dt (`0:dt:duration-dt`, :42), dt = T / n_slices.  coeffs: K x 2, or flat with control j's pair
    at [2j, 2j + 1] (first(j):second(j), :45-46); freqs: K.  Returns (K, n_slices)."""
    freqs = np.asarray(freqs, dtype=np.float64).reshape(-1)
    c = np.asarray(coeffs, dtype=np.float64).reshape(freqs.shape[0], 2)
    t = np.arange(int(n_slices), dtype=np.float64) * (float(duration) / int(n_slices))
    wt = freqs[:, None] * t[None, :]
    return c[:, 0:1] * np.cos(wt) + c[:, 1:2] * np.sin(wt)


def fourier_basis(n_slices, duration, freqs):
    """The functions of dCRAB's ansatz as a basis for GRAPE(basis=...): (n_slices, 2 len(freqs)) with columns
    cos(w_0 t), sin(w_0 t), cos(w_1 t), sin(w_1 t), ... on dcrab_pulse's grid t = 0, dt, ..., T - dt.  Row j of
    dcrab_pulse(c, w, N, T) is c[j] @ fourier_basis(N, T, [w[j]]).T."""
    freqs = np.asarray(freqs, dtype=np.float64).reshape(-1)
    t = np.arange(int(n_slices), dtype=np.float64) * (float(duration) / int(n_slices))
    wt = freqs[:, None] * t[None, :]
    out = np.empty((int(n_slices), 2 * freqs.shape[0]))
    out[:, 0::2] = np.cos(wt).T
    out[:, 1::2] = np.sin(wt).T
    return out


@dataclass
class SolutionResult:
    result: Any
    fidelity: float
    opti_pulses: Any
    problem: Problem
    alg: GRAPE
    parameters: Any = None         # GRAPE(basis=...): the optimal coefficients theta (K, M); opti_pulses is their pulse


@dataclass
class EnsembleSolutionResult:
    result: Any
    fidelity: float
    opti_pulses: Any
    problem: EnsembleProblem
    alg: GRAPE
    parameters: Any = None


def C1(KT, KN):
    """Density-matrix infidelity, src/cost_functions.jl:13-17."""
    KT = np.asarray(KT, complex)
    KN = np.asarray(KN, complex)
    D = KT.shape[0]
    return 1.0 - abs(np.trace(KT.conj().T @ KN) / D) ** 2


def C3(u):
    """Control amplitudes, src/cost_functions.jl:29-31: sum(abs2.(u))."""
    return float(np.sum(np.abs(np.asarray(u, dtype=np.float64)) ** 2))


def C4(u):
    """Control variations, src/cost_functions.jl:36-39: sum(abs2.(diff(u, dims = 2))) -- along the time axis of (K, N)."""
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    return float(np.sum(np.abs(np.diff(u, axis=1)) ** 2))


def C5(psiF, psij):
    """Occupation of forbidden states, src/cost_functions.jl:44-47: sum(abs2(psiF' * psi) for psi in psij)."""
    f = np.asarray(psiF, complex).reshape(-1)
    return float(sum(abs(np.vdot(f, np.asarray(psi, complex).reshape(-1))) ** 2 for psi in psij))


def C6(KT, KJ, N, D):
    """Evolution time (target gate), src/cost_functions.jl:52-54: 1 - 1/N sum(abs2(tr(KT' * Kj) / D) for Kj in KJ)."""
    KT = np.asarray(KT, complex)
    return 1.0 - sum(abs(np.trace(KT.conj().T @ np.asarray(Kj, complex)) / D) ** 2 for Kj in KJ) / N


def C7(psiT, psiJ, N):
    """Evolution time (target state), src/cost_functions.jl:59-61: 1 - 1/N sum(abs2(tr(psiT * psij)) for psij in psiJ) --
    density matrices."""
    psiT = np.asarray(psiT, complex)
    return 1.0 - sum(abs(np.trace(psiT @ np.asarray(pj, complex))) ** 2 for pj in psiJ) / N


class ForbiddenStates:
    """weight x C5 on the device: `states` are forbidden kets (a list of length-n vectors, or one vector), at most four; the
    problem holds its states as n x 1 kets (Xi, Xt of shape (n, 1)) under UnitaryGate.  The cost of a pulse is
    weight * sum_F C5(psiF, [psi_1 .. psi_N]) over the states after every slice, ensemble-weighted like F."""

    def __init__(self, states, weight=1.0):
        s = np.asarray(states, dtype=np.complex128)
        self.states = s.reshape(1, -1) if s.ndim == 1 else s.reshape(s.shape[0], -1)
        self.weight = float(weight)

    def terms(self, members, N):
        n, m = np.asarray(members[0].Xi).shape
        if m != 1 or self.states.shape[1] != n:
            raise ValueError("ForbiddenStates: the problem must hold n x 1 kets and the forbidden states n entries")
        R = np.broadcast_to(self.states[:, None, :, None], (self.states.shape[0], len(members), n, 1))
        return R, np.full((self.states.shape[0], N), self.weight), 0.0

    def to_json(self):
        return {"kind": "ForbiddenStates", "weight": self.weight,
                "states": [[[float(v.real), float(v.imag)] for v in s] for s in self.states]}


class EvolutionTime:
    """weight x C6 (n x m operator states, D = n) or, for n x 1 kets, weight x (1 - 1/N sum_s tr(rhoT rho_s)) with
    tr(rhoT rho) = |psiT' psi|^2 for pure states -- C7's overlap, summed as it is (the reference's one-liner takes abs2 of that
    trace once more) -- on the device, against every member's own target XtG(k).  The constant `weight` (times the sum of the ensemble weights)
    is added by solve()."""

    def __init__(self, weight=1.0):
        self.weight = float(weight)

    def terms(self, members, N):
        Xt = np.array([np.asarray(p.Xt, complex) for p in members])
        n, m = Xt.shape[1:]
        scale = 1.0 / N if m == 1 else 1.0 / (N * n * n)
        return Xt[None], np.full((1, N), -self.weight * scale), self.weight

    def to_json(self):
        return {"kind": "EvolutionTime", "weight": self.weight}


def running_cost_from_json(d):
    if d["kind"] == "ForbiddenStates":
        return ForbiddenStates([[complex(re, im) for re, im in s] for s in d["states"]], d["weight"])
    if d["kind"] == "EvolutionTime":
        return EvolutionTime(d["weight"])
    raise ValueError(f"unknown running cost {d['kind']!r}")


def running_cost_terms(members, costs, N, wts=None):
    """The descriptors of GRAPE(running_costs=...) as grape_set_running_cost takes them: R (n_terms, E, n, m), rho
    (n_terms, N) and the constant solve() adds to the minimum (C6 / C7: weight x sum of the ensemble weights)."""
    wsum = float(len(members)) if wts is None else float(np.sum(wts))
    Rs, rhos, const = [], [], 0.0
    for c in costs:
        R, rho, k = c.terms(members, int(N))
        Rs.append(np.broadcast_to(R, (R.shape[0], len(members)) + R.shape[2:]))
        rhos.append(rho)
        const += k * wsum
    R, rho = np.concatenate(Rs, axis=0), np.concatenate(rhos, axis=0)
    if R.shape[0] > 4:
        raise ValueError("running_costs: at most four terms in all (every forbidden state is one)")
    return np.ascontiguousarray(R), rho, const


class PenaltyFunctionals:
    """src/cost_functions.jl:66-69: relative weights and the penalty functionals they scale.  Only C3 and C4 -- the
    functionals of the pulse alone, which the device adds to every evaluation (grape_set_penalties).  A weight is a
    scalar (every control) or a length-K vector (per control); a functional may appear once."""

    def __init__(self, weights, functions):
        if len(weights) != len(functions):
            raise ValueError("PenaltyFunctionals: one weight per functional")
        self.weights, self.functions = list(weights), list(functions)
        seen = set()
        for f in self.functions:
            if f not in (C3, C4):
                raise ValueError("PenaltyFunctionals: only C3 and C4 are supported")
            if f in seen:
                raise ValueError("PenaltyFunctionals: each functional may appear once")
            seen.add(f)

    def device_weights(self, K):
        """(amp, var) for grape_set_penalties: K-vectors of weights, or None for a term that is absent."""
        out = {C3: None, C4: None}
        for w, f in zip(self.weights, self.functions):
            w = np.asarray(w, dtype=np.float64)
            w = np.full(K, float(w)) if w.ndim == 0 else np.array(w, dtype=np.float64)
            if w.shape != (K,):
                raise ValueError(f"PenaltyFunctionals: a weight must be a scalar or have {K} entries")
            out[f] = w
        return out[C3], out[C4]

    def __call__(self, u):
        """sum of weight x functional, each control scaled by its own weight."""
        u = np.atleast_2d(np.asarray(u, dtype=np.float64))
        amp, var = self.device_weights(u.shape[0])
        total = 0.0
        for c in range(u.shape[0]):
            if amp is not None:
                total += amp[c] * C3(u[c])
            if var is not None:
                total += var[c] * C4(u[c:c + 1])
        return total

    def to_json(self):
        return {"weights": [np.asarray(w, dtype=np.float64).tolist() for w in self.weights],
                "functions": ["C3" if f is C3 else "C4" for f in self.functions]}

    @classmethod
    def from_json(cls, d):
        return cls(d["weights"], [{"C3": C3, "C4": C4}[f] for f in d["functions"]])


def init_ensemble(ens):
    """src/tools.jl:42-53: one Problem per member with A, B, Xi, Xt from the generators."""
    out = []
    for k in range(1, ens.n_ens + 1):
        p = ens.prob
        out.append(Problem(B=ens.B_g(k), A=ens.A_g(k), Xi=ens.XiG(k), Xt=ens.XtG(k), T=p.T,
                           n_controls=p.n_controls, guess=p.guess, sys_type=p.sys_type))
    return out


def _pack(problems):
    A = np.array([np.asarray(p.A, complex) for p in problems])
    B = np.array([[np.asarray(b, complex) for b in p.B] for p in problems])
    Xi = np.array([np.asarray(p.Xi, complex) for p in problems])
    Xt = np.array([np.asarray(p.Xt, complex) for p in problems])
    return A, B, Xi, Xt


def make_engine(prob, alg, **engine_kw):
    """Build the device context for a Problem (E = 1) or an EnsembleProblem."""
    if isinstance(prob, EnsembleProblem):
        members = init_ensemble(prob)
        wts = np.asarray(prob.wts, dtype=np.float64)
    else:
        members = [prob]
        wts = np.ones(1)
    first = members[0]
    if len(first.B) != first.n_controls:
        raise ValueError("n_controls does not match the number of control operators")
    A, B, Xi, Xt = _pack(members)
    if getattr(alg, "devices", None):
        from .engine import FLAG_GROUP_PEER_SUM
        engine_kw = dict(engine_kw, devices=list(alg.devices))
        if getattr(alg, "peer_sum", False):
            engine_kw["flags"] = engine_kw.get("flags", 0) | FLAG_GROUP_PEER_SUM
    if isinstance(alg, (ADGRAPE, dCRAB)):   # pw_evolve adds A first (src/timeevolution.jl:32-35): the static summation order
        eng = GrapeEngine(first.sys_type.name, A, B, Xi, Xt, wts, first.T, alg.n_slices, variant=1, device=alg.device,
                          gradient="exact", objective="c1", **engine_kw)
    else:
        eng = GrapeEngine(first.sys_type.name, A, B, Xi, Xt, wts, first.T, alg.n_slices,
                          variant=0 if alg.isinplace else 1, device=alg.device, **engine_kw)
    pen = getattr(alg, "penalties", None)
    if pen is not None:                     # on the device: the host optimiser, grape_lbfgs and every shard see them
        try:
            eng.set_penalties(*pen.device_weights(first.n_controls))
        except Exception:
            eng.close()
            raise
    eng.running_cost_constant = 0.0
    costs = getattr(alg, "running_costs", None)
    if costs:
        try:
            R, rho, const = running_cost_terms(members, costs, alg.n_slices, wts)
            mode = "exact" if isinstance(alg, ADGRAPE) else getattr(alg, "running_cost_derivative", "first_order")
            if mode != "first_order":       # the mode BEFORE the costs: an exact-gradient context refuses them otherwise
                eng.set_running_cost_derivative(mode)
            eng.set_running_cost(R, rho)
            eng.running_cost_constant = const
        except Exception:
            eng.close()
            raise
    return eng


def fom_and_gradient(prob, alg, x, engine=None):
    """One call of the closure `topt(F, G, x)` (src/solve.jl:75-100 / :164-196)."""
    own = engine is None
    eng = engine or make_engine(prob, alg)
    try:
        return eng.eval(x)
    finally:
        if own:
            eng.close()


def _observe_setup(prob, pulse_or_solres, engine):
    """(engine, owned, pulse, weights) for the read-out functions: a plain engine of the problem (no penalties, basis, bounds or
    running costs: the pulse is the physical one) unless the caller brings one, whose evaluations then take `pulse` as it is"""
    if isinstance(pulse_or_solres, (SolutionResult, EnsembleSolutionResult)):
        pulse, base = pulse_or_solres.opti_pulses, pulse_or_solres.alg
    else:
        pulse, base = pulse_or_solres, None
    pulse = np.asarray(pulse, dtype=np.float64)
    if pulse.ndim != 2:
        raise ValueError("the pulse must be a (K, N) array")
    wts = np.asarray(prob.wts, dtype=np.float64) if isinstance(prob, EnsembleProblem) else np.ones(1)
    if engine is not None:
        return engine, False, pulse, wts
    alg = GRAPE(n_slices=pulse.shape[1], isinplace=getattr(base, "isinplace", True), device=getattr(base, "device", -1))
    return make_engine(prob, alg), True, pulse, wts


def test_pulse(prob, pulse_or_solres, engine=None):
    """What src/tools.jl:32-36 names and leaves unimplemented: simulate the pulse again and return the output, so that the
    gate can be checked.  prob: a Problem or an EnsembleProblem; pulse_or_solres: a (K, N) pulse or what solve() returned
    (its opti_pulses).  Returns (X_final (E, n, m), member_F (E,), F): the final state of every member from the device
    (grape_eval_observables), its figure of merit computed here from X_final and Xt with fom_func's formulas
    (src/cost_functions.jl:99-111: Re z^2 for UnitaryGate, 1 - |z / n|^2 for the sandwich types, z = tr(Xt' X_final)) and
    their weighted sum."""
    eng, own, pulse, wts = _observe_setup(prob, pulse_or_solres, engine)
    try:
        _, Xf = eng.observe(pulse, None, final=True)
    finally:
        if own:
            eng.close()
    members = init_ensemble(prob) if isinstance(prob, EnsembleProblem) else [prob]
    Xt = np.array([np.asarray(p.Xt, complex).reshape(Xf.shape[1:]) for p in members])
    z = np.einsum("kab,kab->k", Xt.conj(), Xf)
    if isinstance(members[0].sys_type, UnitaryGate):
        member_F = np.real(z * z)
    else:
        member_F = 1.0 - np.abs(z / Xf.shape[1]) ** 2
    return Xf, member_F, float(wts @ member_F)


test_pulse.__test__ = False                    # (a library function, not a test: keep pytest from collecting it)


def expectation_values(prob, pulse, ops, engine=None, mean=False):
    """What src/visualisation.jl:13-51 computes (commented out there): the expectation values of `ops` along the pulse.
    ops: (n_obs, n, m) matrices (or one (n, m) matrix), at most 16.  Returns (times (N+1,), y (E, n_obs, N+1)) with
    y[k, j, s] = tr(ops[j]' X_ks) from the device; y.real is what visualise_expt_vals plots against the times.
    mean=True: (times, y_mean (n_obs, N+1)) with y_mean = sum_k wts_k y[k], the curve of an EnsembleProblem under its own
    weights, summed on the device (GrapeEngine.observe_mean): the member axis is never copied to the host."""
    eng, own, pulse, _ = _observe_setup(prob, pulse, engine)
    try:
        y = eng.observe_mean(pulse, ops) if mean else eng.observe(pulse, ops)
        times = np.linspace(0.0, eng.T, eng.N + 1)
    finally:
        if own:
            eng.close()
    return times, y


def _json_default(v):
    """Values `json` does not know inside alg.optim_options: NumPy scalars / arrays become numbers / lists, anything else
    (callables, objects) its repr -- a solve that succeeded must stay savable (the reference's BSON takes any value)."""
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (set, frozenset, tuple)):
        return list(v)
    return repr(v)


def save(solres, file_path):
    """src/tools.jl:59-72: every field of a SolutionResult / EnsembleSolutionResult but the optimiser's own result object
    (the reference drops it too: `fieldnames(...)[2:end]`) into one file -- NumPy's .npz here instead of BSON.  The
    problem's operators and states are stored as arrays; generator closures of an EnsembleProblem are stored as the
    members they generate."""
    prob = solres.problem
    ens = isinstance(prob, EnsembleProblem)
    base = prob.prob if ens else prob
    alg = solres.alg
    data = {
        "kind": np.array("ensemble" if ens else "single"),
        "fidelity": np.array(float(solres.fidelity)),
        "opti_pulses": np.asarray(solres.opti_pulses, dtype=np.float64),
        "sys_type": np.array(base.sys_type.name), "T": np.array(float(base.T)), "n_controls": np.array(int(base.n_controls)),
        "A": np.asarray(base.A, complex), "B": np.asarray(base.B, complex), "Xi": np.asarray(base.Xi, complex),
        "Xt": np.asarray(base.Xt, complex), "guess": np.asarray(base.guess, dtype=np.float64),
        "alg_kind": np.array(type(alg).__name__), "n_slices": np.array(int(alg.n_slices)),
        "isinplace": np.array(bool(getattr(alg, "isinplace", True))),
        # the whole alg struct, as the reference's save does (src/tools.jl:59-72): a re-solve from a loaded result must use
        # the optimiser, tolerances and devices of the saved run, not the defaults
        "alg_fields": np.array(json.dumps({"expm_method": alg.expm_method, "optim_options": alg.optim_options,
                                            "device": int(alg.device), "optimizer": alg.optimizer,
                                            "devices": None if alg.devices is None else [int(v) for v in alg.devices],
                                            "peer_sum": bool(alg.peer_sum),
                                            **({"penalties": alg.penalties.to_json()} if alg.penalties is not None else {}),
                                            **({"bounds": [np.asarray(b, dtype=np.float64).tolist() for b in alg.bounds]}
                                               if getattr(alg, "bounds", None) is not None else {}),
                                            **({"running_costs": [c.to_json() for c in alg.running_costs]}
                                               if getattr(alg, "running_costs", None) else {}),
                                            **({"running_cost_derivative": str(alg.running_cost_derivative)}
                                               if getattr(alg, "running_cost_derivative", "first_order") != "first_order" else {}),
                                            **({"risk": float(alg.risk)} if getattr(alg, "risk", 0.0) else {})},
                                           default=_json_default)),
    }
    if ens:
        members = init_ensemble(prob)
        data.update(n_ens=np.array(int(prob.n_ens)), wts=np.asarray(prob.wts, dtype=np.float64),
                    A_members=np.array([np.asarray(m.A, complex) for m in members]),
                    B_members=np.array([np.asarray(m.B, complex) for m in members]),
                    Xi_members=np.array([np.asarray(m.Xi, complex) for m in members]),
                    Xt_members=np.array([np.asarray(m.Xt, complex) for m in members]))
    with open(file_path, "wb") as io:
        np.savez(io, **data)


def load(file_path):
    """src/tools.jl:75-85 (whose own version passes four arguments to a five-field struct): the SolutionResult back,
    with `result = None` as the reference intends."""
    d = np.load(file_path, allow_pickle=False)
    st = {"StateTransfer": StateTransfer, "UnitaryGate": UnitaryGate, "CoherenceTransfer": CoherenceTransfer}[str(d["sys_type"])]()
    base = Problem(B=list(d["B"]), A=d["A"], Xi=d["Xi"], Xt=d["Xt"], T=float(d["T"]), n_controls=int(d["n_controls"]),
                   guess=d["guess"], sys_type=st)
    alg_cls = ADGRAPE if str(d["alg_kind"]) == "ADGRAPE" else GRAPE
    extra = json.loads(str(d["alg_fields"])) if "alg_fields" in d.files else {}      # (files of earlier rounds: defaults)
    if extra.get("penalties") is not None:
        extra["penalties"] = PenaltyFunctionals.from_json(extra["penalties"])
    if extra.get("running_costs") is not None:
        extra["running_costs"] = [running_cost_from_json(c) for c in extra["running_costs"]]
    alg = alg_cls(n_slices=int(d["n_slices"]), **extra) if alg_cls is ADGRAPE else GRAPE(n_slices=int(d["n_slices"]),
                                                                                           isinplace=bool(d["isinplace"]), **extra)
    if str(d["kind"]) == "ensemble":
        Am, Bm, Xim, Xtm = d["A_members"], d["B_members"], d["Xi_members"], d["Xt_members"]
        ens = EnsembleProblem(prob=base, n_ens=int(d["n_ens"]), A_g=lambda k: Am[k - 1], B_g=lambda k: list(Bm[k - 1]),
                              XiG=lambda k: Xim[k - 1], XtG=lambda k: Xtm[k - 1], wts=d["wts"])
        return EnsembleSolutionResult(None, float(d["fidelity"]), d["opti_pulses"], ens, alg)
    return SolutionResult(None, float(d["fidelity"]), d["opti_pulses"], base, alg)


def pulse_to_file(pulse, file_path, duration=None):
    """src/tools.jl:90-104: write a (K, N) pulse as delimited text with time going down the file
    (`writedlm(io, pulse')`, tab separated); with `duration`, a leading time column
    `range(0, duration, length=N)` like the reference's 3-argument method (which takes N = length(pulse),
    i.e. a single-control pulse)."""
    P = np.atleast_2d(np.asarray(pulse, dtype=np.float64))
    rows = P.T
    if duration is not None:
        t = np.linspace(0.0, float(duration), rows.shape[0])
        rows = np.column_stack([t, rows])
    with open(file_path, "w") as io:
        for r in rows:
            io.write("\t".join(repr(float(v)) for v in r) + "\n")


def pulse_from_file(file_path, has_time_column=False):
    """inverse of pulse_to_file: returns the (K, N) pulse (and the time column if present)."""
    data = np.loadtxt(file_path, delimiter="\t", ndmin=2)
    if has_time_column:
        return np.ascontiguousarray(data[:, 1:].T), data[:, 0].copy()
    return np.ascontiguousarray(data.T)


def _lbfgs(topt, x0, options):
    """Stand-in for Optim.optimize(Optim.only_fg!(topt), x0, LBFGS(), opts) (src/solve.jl:138)."""
    from scipy.optimize import minimize

    shape = x0.shape
    opts = {"maxiter": int(options.get("iterations", 1000)), "gtol": float(options.get("g_tol", 1e-8)),
            "ftol": float(options.get("f_tol", 0.0)) or 1e-15, "maxls": 40}

    def fun(xflat):
        F, G = topt(xflat.reshape(shape))
        return F, G.reshape(-1)

    res = minimize(fun, np.asarray(x0, float).reshape(-1), jac=True, method="L-BFGS-B", options=opts)
    res.minimum = float(res.fun)
    res.minimizer = res.x.reshape(shape)
    return res


def _device_lbfgs(eng, x0, options):
    """grape_lbfgs with Optim-style options (iterations, g_tol, f_tol); result mimics the fields solve() reads."""
    from types import SimpleNamespace

    x_min, info = eng.lbfgs(x0, iterations=int(options.get("iterations", 0)), g_tol=float(options.get("g_tol", -1.0)),
                            f_tol=float(options.get("f_tol", 0.0)), line_search=options.get("line_search", "hagerzhang"),
                            probes=int(options.get("probes", 0)))
    return SimpleNamespace(minimum=info["minimum"], minimizer=x_min, x=x_min.reshape(-1), fun=info["minimum"],
                           nit=info["iterations"], nfev=info["evaluations"], message=info["message"],
                           success=info["status"] in (0, 1), device_lbfgs=info)


def _basis_start(eng, guess, basis, offset):
    """GRAPE(basis=...): puts the engine into parameter mode and returns the start theta (K, M), the least-squares fit of
    guess - offset in the basis (per control when every control has its own)."""
    basis = np.asarray(basis, dtype=np.float64)
    off = None if offset is None else np.asarray(offset, dtype=np.float64).reshape(guess.shape)
    eng.set_basis(basis, off)
    r = guess if off is None else guess - off
    if basis.ndim == 2:
        return np.ascontiguousarray(np.linalg.lstsq(basis, r.T, rcond=None)[0].T)
    return np.array([np.linalg.lstsq(basis[c], r[c], rcond=None)[0] for c in range(guess.shape[0])])


def _solve_dcrab(prob, alg, eng):
    """src/dCRAB.jl:13-89 on the device functional.  Deviations, on purpose: the start vector has n_coeff K entries (the
    reference hard-codes `reshape(..., 4)`, :71, i.e. two controls); and Nelder-Mead's first simplex is SciPy's default one
    around the drawn coefficients with its last vertex moved to the origin -- the CURRENT pulse -- so a super-iteration never
    returns a worse pulse than it was given (the reference starts every search from random coefficients only)."""
    from scipy.optimize import minimize

    base = prob.prob if isinstance(prob, EnsembleProblem) else prob
    K, N, T = int(base.n_controls), int(alg.n_slices), float(base.T)
    pulse = np.array(base.guess, dtype=np.float64).reshape(K, N)
    rng = np.random.default_rng(alg.seed)
    freqs = rng.random((alg.n_freq, K))                        # init_freq, :29
    coeffs = rng.random((alg.n_freq, K, alg.n_coeff))          # init_coeffs, :33 (control j's coefficients adjacent)
    results, minima = [], []
    for i in range(alg.n_freq):
        current = pulse

        def to_minimize(c, current=current, w=freqs[i]):
            return eng.fom(current + dcrab_pulse(c, w, N, T))

        x0 = coeffs[i].reshape(-1)
        sim = np.tile(x0, (x0.size + 1, 1))
        for k in range(x0.size - 1):                            # scipy.optimize's default simplex ...
            sim[k + 1, k] = sim[k + 1, k] * 1.05 if sim[k + 1, k] != 0 else 0.00025
        sim[-1] = 0.0                                           # ... but for the vertex that keeps the pulse as it is
        if x0[-1] == 0.0:                                       # (a degenerate simplex otherwise; the draw is in [0, 1))
            sim[0, -1] = 0.00025
        opts = dict(alg.options or {})
        opts["initial_simplex"] = sim
        res = minimize(to_minimize, x0, method="Nelder-Mead", options=opts)
        res.minimum, res.minimizer, res.frequencies = float(res.fun), res.x.copy(), freqs[i].copy()
        pulse = current + dcrab_pulse(res.x, freqs[i], N, T)    # the pulse whose functional is res.fun
        results.append(res)
        minima.append(float(res.fun))
    return results, minima, pulse


def solve(prob, alg: Optional[GRAPE] = None, engine=None):
    """solve(::Problem, ::GRAPE) / solve(::EnsembleProblem, ::GRAPE).  With alg.penalties the minimised objective is the
    figure of merit plus the C3 / C4 penalties, and `fidelity` (res.minimum, as src/solve.jl:139) includes them.  With
    alg.running_costs the device adds weight x C5 / C6 / C7 without the constant 1 of C6 / C7; solve adds it to res.minimum.
    solve(prob, dCRAB(...)): `result` is the list of the super-iterations' Nelder-Mead results, `fidelity` the list of their
    minima and `opti_pulses` the final (K, N) pulse (src/dCRAB.jl:114)."""
    if alg is None:
        raise TypeError("solve(prob) without an algorithm has no integrator in the reference either "
                        "(src/solve.jl:57,66); pass GRAPE(n_slices=...)")
    if isinstance(alg, dCRAB):
        eng = engine or make_engine(prob, alg)
        try:
            results, minima, pulse = _solve_dcrab(prob, alg, eng)
        finally:
            if engine is None:
                eng.close()
        cls = EnsembleSolutionResult if isinstance(prob, EnsembleProblem) else SolutionResult
        return cls(results, minima, pulse, prob, alg)
    own = engine is None
    device_opt = getattr(alg, "optimizer", "host") == "device"
    batched = device_opt and not isinstance(alg, ADGRAPE) and not getattr(alg, "devices", None) and \
        alg.optim_options.get("line_search") == "ladder"          # the ladder search probes several step lengths per launch
    eng = engine or make_engine(prob, alg, **({"max_batch": 4} if batched else {}))
    basis = getattr(alg, "basis", None)
    bounds = getattr(alg, "bounds", None)
    risk = float(getattr(alg, "risk", 0.0) or 0.0)
    params = None
    try:
        guess = np.asarray((prob.prob if isinstance(prob, EnsembleProblem) else prob).guess, float)
        if risk:                                               # every evaluation below returns the risk-weighted [G, F]
            eng.set_risk(risk)
        if bounds is not None:                                 # the optimiser's variables are the raw pulse from here on
            guess = bounds_start(guess, *bounds)
            eng.set_bounds(*bounds)
        try:
            if basis is not None:
                guess = _basis_start(eng, guess, basis, getattr(alg, "basis_offset", None))
            if device_opt:
                res = _device_lbfgs(eng, guess, alg.optim_options)
            else:
                res = _lbfgs(lambda x: eng.eval(x), guess, alg.optim_options)
            res.minimum = float(res.minimum) + float(getattr(eng, "running_cost_constant", 0.0))
            pulse = res.minimizer
            if basis is not None or bounds is not None:        # the physical pulse, from the kernel the evaluations used
                params, pulse = res.minimizer, eng.controls(res.minimizer)
        finally:
            if basis is not None and not own:                  # a caller's engine goes back as it came
                eng.set_basis(None)
            if bounds is not None and not own:
                eng.set_bounds(None)
            if risk and not own:
                eng.set_risk(0.0)
    finally:
        if own:
            eng.close()
    cls = EnsembleSolutionResult if isinstance(prob, EnsembleProblem) else SolutionResult
    return cls(res, res.minimum, pulse, prob, alg, params)
