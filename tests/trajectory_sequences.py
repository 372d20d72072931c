"""Random walks over the calls that keep state on a context behind the trajectory: the read-out (grape_eval_observables), its
pull-back and push-forward (grape_eval_vjp, grape_eval_jvp), the three device forms and their d_x = NULL reuse,
grape_set_trajectory_derivative, grape_set_running_cost_derivative and grape_set_risk -- between the settings the older walks
know (settings_sequences.py, bounds_sequences.py: penalties, basis, bounds, running cost, operator re-uploads that flip the
data flow).  Shared by test_gpu_trajectory_soak.py (runs the walks on the device), test_trajectory_sequences_host.py (shows
on the CPU what the committed seeds cover and that no mix-up can hide) and tools/soak_trajectory.py.  No test functions here.

  draw_context / draw_steps   pure functions of the generator state: they never touch the library.
  TState               bounds_sequences.BState + the two derivative modes, the risk, and the "trajectory valid" flag by the
                       rule of include/grape_hip.h: set by a successful device form with d_x on a context that is not
                       member-chunked, kept by an accepted reuse, cleared by everything else that evaluates or changes a
                       setting, refused calls included.  The model is the reference: a reuse step asserts what it says.
  Refs                 the references, from observe_reference, vjp_reference, jvp_reference, traj_exact_reference,
                       rc_exact_reference, risk_reference, bounds_sequences.sat and settings_sequences.composed_reference
                       alone, cached per context.  No device result enters them.
  run_context          one context and its steps on the device: parity at the project's bar, a bitwise memo of every
                       trajectory result and every [F, G] keyed by what the header says it may depend on, the transpose
                       identity on every Gauss-Newton pair, the refusals with status and reason word.
  coverage             what the walks of a set of seeds observe, from the model alone.
"""
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_sequences as bs  # noqa: E402
import jvp_reference as jr  # noqa: E402
import observe_reference as obr  # noqa: E402
import rc_exact_reference as rxr  # noqa: E402
import risk_reference as rr  # noqa: E402
import settings_sequences as ss  # noqa: E402
import traj_exact_reference as xr  # noqa: E402
import vjp_reference as vr  # noqa: E402
from conftest import PARITY_RTOL, assert_parity  # noqa: E402

SEEDS = range(40)
CONTEXTS_PER_SEED = 4
SETTING_OPS = ("upload", "pen_on", "pen_change", "pen_off", "basis_on", "basis_per_control", "basis_off", "bounds_on",
               "bounds_change", "bounds_off", "rc_on", "rc_change", "rc_off", "traj_exact", "traj_first", "rc_exact", "rc_first",
               "risk_on", "risk_change", "risk_off")
OLD_CHECK_OPS = ("eval", "device", "batch", "fom", "controls")
NEW_CHECK_OPS = ("risk_weights", "observe", "observe_device", "vjp", "vjp_device", "vjp_reuse", "jvp", "jvp_device", "jvp_reuse",
                 "gn_pair", "device_refused", "jvp_linear")
CHECK_OPS = OLD_CHECK_OPS + NEW_CHECK_OPS
REUSE_OPS = ("vjp_reuse", "jvp_reuse", "gn_pair")
DEVICE_FORMS = ("observe_device", "vjp_device", "jvp_device")
PROBE_COUNTS = (0, 1, 3, 8, 9, 16)
BETAS = (0.5, 4.0, 40.0)
UNSUPPORTED, INVALID_ARG, NOT_READY = -2, -1, -5
FRECHET_LOOP_MAX = 600           # (slice, member, control) triples up to which the per-slice expm_frechet loop is taken; above,
                                 # traj_exact_reference.slice_derivatives_eig (pinned to it at 1e-12 by test_traj_exact_host.py)


# ---- contexts -------------------------------------------------------------------------------------------------------------
def _cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _draw_probes(rng, ctx, which):
    """one probe set and its two cotangent draws; O_0 = Xi, so that |y|_inf is of order 1"""
    n, m, E, N = ctx["n"], ctx["m"], ctx["E"], ctx["N"]
    n_obs = int(rng.choice(PROBE_COUNTS))
    per_member = bool(rng.integers(0, 2))
    O = None
    if n_obs:
        O = _cplx(rng, E, n_obs, n, m) if per_member else _cplx(rng, n_obs, n, m)
        if per_member:
            O[:, 0] = ctx["ops"]["Xi"]
        else:
            O[0] = ctx["ops"]["Xi"][0]
    yb = [_cplx(rng, E, n_obs, N + 1) if n_obs else None for _ in range(2)]
    xb = [_cplx(rng, E, n, m) for _ in range(2)]
    if n_obs:                                             # both / ybar only / Xbar only, by the set's place in the pool
        cots = [[(yb[0], xb[0]), (yb[1], None)], [(yb[0], xb[0]), (None, xb[1])], [(yb[0], None), (yb[1], xb[1])]][which]
        if which == 2:
            yb[0][:, :, ::3] = 0.0                        # whole zero rows in s (s = 0 among them; s = 1 stays)
    else:
        cots = [(None, xb[0]), (None, xb[1])]
    return dict(n_obs=n_obs, per_member=per_member, O=O, cots=cots)


def draw_context(rng):
    """One context: shape, launch geometry, first operators, and its pools -- three pulses, three directions, three probe
    sets with two cotangent draws each."""
    served = bool(rng.random() < 0.75)
    ctx = dict(full=served, variant=int(rng.integers(0, 2)), max_batch=int(rng.choice([1, 3])), S=0, W=0, kernel=None,
               budget=None, chunked=False, gexact=None)
    n = ctx["n"] = int(rng.choice([2, 3, 4]))
    ctx["K"] = int(rng.choice([1, 2, 3, 5]))
    ctx["N"] = int(rng.choice([1, 3, 8, 20, 65, 130]))
    ctx["E"] = int(rng.choice([1, 2, 3, 7, 33]))
    ctx["staged"] = [None, "0", "1"][int(rng.integers(0, 3))]
    long_T = bool(rng.random() < 1.0 / 6.0)
    if served:
        ctx["sys_type"] = "UnitaryGate"
        ctx["m"] = int(rng.integers(1, n + 1))
        ctx["T"] = 24.0 if long_T else float(rng.uniform(0.3, 1.5))
        ctx["scale"] = float(rng.uniform(0.3, 0.5)) if long_T else float(rng.uniform(0.5, 1.0))
        ctx["kernel"] = "lane" if n == 3 else str(rng.choice(["lane", "pair"]))
        if rng.random() < 0.3:
            ctx["S"], ctx["W"] = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        kind = rng.random()
        if kind < 0.33:                                   # member-chunked: the recipe of settings_sequences.draw_context
            ctx["chunked"], ctx["E"], ctx["max_batch"] = True, 7, 3
            ctx["W"] = 2 if ctx["kernel"] == "lane" else 4
            cpw = 64 if ctx["kernel"] == "lane" else 32
            ctx["N"] = min(ctx["N"], 65)
            S = max(ctx["S"], -(-ctx["N"] // (cpw * ctx["W"])))
            ctx["budget"] = int(2.5 * 2 * 16 * S * n * n * cpw * ctx["W"])
        elif kind < 0.55:                                 # gradient = exact: the trajectory calls are refused
            ctx["gexact"] = str(rng.choice(["fom", "c1"]))
    else:
        ctx["sys_type"] = str(rng.choice(["StateTransfer", "CoherenceTransfer"]))
        ctx["m"] = n
        ctx["T"], ctx["scale"] = float(rng.uniform(0.3, 1.5)), 1.0
    if ctx["E"] == 33:
        ctx["N"] = min(ctx["N"], 20)                      # (the references are double sums over the slices)
    if ctx["N"] == 130 and ctx["E"] == 7:
        ctx["N"] = 65
    ctx["served"] = served and ctx["gexact"] is None      # VJP, JVP and the exact modes are served
    ctx["ops"] = (ss.full_operators if served else ss.partial_operators)(rng, ctx)
    ctx["pool"] = rng.uniform(-1, 1, (3, ctx["K"], ctx["N"]))
    ctx["xdots"] = rng.standard_normal((3, ctx["K"], ctx["N"]))
    ctx["probes"] = [_draw_probes(rng, ctx, which) for which in range(3)]
    return ctx


def context_line(ctx):
    return (ss.context_line(ctx) + f" gradient={'exact/' + ctx['gexact'] if ctx['gexact'] else 'reference'} "
            f"staged={ctx['staged']} probes=" + ",".join(f"{p['n_obs']}{'m' if p['per_member'] else 's'}" for p in ctx["probes"]))


def step_line(step):
    extra = {k: step[k] for k in ("i", "p", "c", "d", "form", "J", "kind", "M", "herm", "sparse", "offset", "beta", "lo", "hi")
             if k in step}
    return step["op"] + (" " + str(extra) if extra else "")


# ---- the model ------------------------------------------------------------------------------------------------------------
class TState(bs.BState):
    """bounds_sequences.BState, the two derivative modes, the risk and the "trajectory valid" flag"""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.traj_mode = self.rc_mode = "first_order"
        self.risk = None
        self.valid = None                                 # flag set: (device form that set it, pulse index); clear: None
        self.cleared_by = "never set"                     # the class of the call that cleared the flag last
        self.basis_gen = self.bounds_gen = self.pen_gen = 0
        self.refusal = None                               # the last step was refused: (status, reason word)
        self.prev_ops = None

    # what the header refuses, and the word its message carries
    def traj_refusal(self, op="vjp"):
        ctx = self.ctx
        if ctx["sys_type"] != "UnitaryGate":
            return None if op in ("observe", "observe_device") else (UNSUPPORTED, "StateTransfer")
        if ctx["gexact"]:                                 # (the read-out checks the objective first, the pair the gradient)
            return (UNSUPPORTED, "c1" if ctx["gexact"] == "c1" and op in ("observe", "observe_device") else "exact")
        return None

    def setting_refusal(self, op):
        ctx = self.ctx
        sandwich = ctx["sys_type"] != "UnitaryGate"
        if op in ("rc_on", "rc_change"):
            if sandwich:
                return (UNSUPPORTED, "StateTransfer")
            if ctx["gexact"] and self.rc_mode != "exact":
                return (UNSUPPORTED, "exact")
            if self.risk is not None:
                return (UNSUPPORTED, "risk")
        elif op == "rc_exact" and sandwich:
            return (UNSUPPORTED, "StateTransfer")
        elif op == "rc_first" and ctx["gexact"] and self.rc is not None:
            return (UNSUPPORTED, "exact")
        elif op == "traj_exact":
            return self.traj_refusal()
        elif op in ("risk_on", "risk_change") and self.rc is not None:
            return (UNSUPPORTED, "running cost")
        return None

    def reuse_refusal(self):
        """what a d_x = NULL call answers now: None (it runs), or (status, word)"""
        why = self.traj_refusal()
        if why:
            return why
        if self.ctx["chunked"]:
            return (NOT_READY, "member_chunk")
        if self.valid is None:
            return (NOT_READY, "reuse")
        return None

    def clear(self, by):
        if self.valid is not None:                        # (only the call that found the flag set is its invalidator)
            self.cleared_by = by
        self.valid = None

    def apply(self, step):
        op = step["op"]
        self.refusal = None
        self.refused = False
        if op in SETTING_OPS:
            self.clear("upload" if op == "upload" else "setting change")
            self.refusal = self.setting_refusal(op)
            if self.refusal:
                self.refused = True
                return
            if op == "upload":
                self.prev_ops = self.ops
            if op in ("pen_on", "pen_change", "pen_off"):
                self.pen_gen += 1
            if op in ("basis_on", "basis_per_control", "basis_off"):
                self.basis_gen += 1
            if op in ("bounds_on", "bounds_change", "bounds_off"):
                self.bounds_gen += 1
            if op in ("rc_on", "rc_change"):
                self.rc, self.rc_gen = step, self.rc_gen + 1
            elif op == "traj_exact":
                self.traj_mode = "exact"
            elif op == "traj_first":
                self.traj_mode = "first_order"
            elif op == "rc_exact":
                self.rc_mode = "exact"
            elif op == "rc_first":
                self.rc_mode = "first_order"
            elif op in ("risk_on", "risk_change"):
                self.risk = step["beta"]
            elif op == "risk_off":
                self.risk = None
            else:
                super().apply(step)
            return
        # the checks
        if op in DEVICE_FORMS:
            if self.traj_refusal(op):
                self.clear("refused device call")
            elif self.ctx["chunked"]:
                self.clear("chunked context")
            else:
                self.valid = (op, step["i"])
        elif op in REUSE_OPS:
            if self.reuse_refusal():                      # (a failed call of the device forms clears the flag)
                self.clear("refused device call")
        elif op == "device_refused":
            self.clear("refused device call")
        elif op == "risk_weights":
            self.clear("eval")                            # (the step evaluates, then reads p)
        elif op in ("observe", "vjp", "jvp", "jvp_linear"):
            self.clear("host form")
        else:
            self.clear({"device": "eval"}.get(op, op))    # eval, batch, fom, controls; grape_eval_device counts as eval

    def dirs(self):
        """the pool of directions, in the coordinates the calls work in"""
        return self.ctx["xdots"] if self.basis is None else self.basis["tdots"]

    def expand_dir(self, tdot):
        """the expansion without x0"""
        if self.basis is None:
            return np.asarray(tdot)
        phi = self.basis["phi"]
        if phi.ndim == 2:
            return tdot @ phi.T
        return np.array([tdot[c] @ phi[c].T for c in range(tdot.shape[0])])

    def conditions(self):
        """the settings a check observes"""
        on = []
        for name, flag in (("basis", self.basis is not None), ("bounds", self.bounds is not None), ("penalties", self.pen is not None),
                           ("running cost", self.rc is not None), ("exact running cost", self.rc is not None and self.rc_mode == "exact"),
                           ("risk", self.risk is not None), ("exact trajectory mode", self.traj_mode == "exact"),
                           ("chunked", self.ctx["chunked"])):
            if flag:
                on.append(name)
        return on

    def fg_key(self, i):
        """what [F, G] of pulse i may depend on: every setting (not the trajectory mode, and the running cost's only under one)
        -- and not the entry point: grape_eval, grape_eval_device, an entry of a batch and the d_fg of the device read-out
        share the key"""
        rc = (self.rc_gen, self.rc_mode) if self.rc is not None else None
        return ("fg", self.gen, self.basis_gen, self.bounds_gen, self.pen_gen if self.pen is not None else None, rc, self.risk, i)

    def traj_key(self, kind, i, *rest):
        """what a trajectory result may depend on: operators, basis, bounds, (the mode,) the pulse, the probes, the vector"""
        mode = () if kind == "observe" else (self.traj_mode,)
        return (kind, self.gen, self.basis_gen, self.bounds_gen) + mode + (i,) + rest


# ---- steps ----------------------------------------------------------------------------------------------------------------
def _draw_setting(rng, ctx, st, forced=None):
    menu = ["upload", "pen_on", "pen_on", "pen_on", "basis_on", "basis_per_control", "bounds_on", "bounds_on", "rc_on", "rc_on", "risk_on", "risk_on",
            "traj_exact", "traj_exact", "traj_exact", "rc_exact", "rc_exact"]
    if st.basis is None:
        menu += ["basis_on", "basis_per_control"]
    if st.risk is None and st.rc is None:
        menu += ["risk_on"]
    if st.rc is not None:
        menu += ["rc_change", "rc_off", "upload", "risk_on"] + (["rc_exact"] * 3 if st.rc_mode == "first_order" else [])
    if st.pen is not None:
        menu += ["pen_change", "pen_off"]
    if st.basis is not None:
        menu += ["basis_off"]
    if st.bounds is not None:
        menu += ["bounds_change", "bounds_off"]
    if st.risk is not None:
        menu += ["risk_change", "risk_off", "rc_on"]
    if st.traj_mode == "exact":
        menu += ["traj_first"]
    if st.rc_mode == "exact":
        menu += ["rc_first"] + ["rc_on"] * (4 if st.rc is None else 0)
    if st.rc is not None and st.rc_mode == "exact" and st.traj_mode == "first_order" and ctx["served"]:
        menu += ["traj_exact"] * 4                        # (the exact pair and the exact running cost share their scratch)
    if ctx["gexact"]:                                     # (a running cost stands there in the exact mode only)
        menu += ["rc_first"] * 6 if st.rc is not None else ["rc_exact"] * 6 if st.rc_mode == "first_order" else ["rc_on"] * 8
    op = forced or str(rng.choice(menu))
    step = dict(op=op)
    if op == "upload":
        if ctx["full"]:
            herm, sparse = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
            if rng.random() < 0.6:
                herm = not st.ops["herm"]                 # the flip of the data flow
            step["ops"] = ss._full_operators(rng, ctx, herm, sparse)
        else:
            step["ops"] = ss.partial_operators(rng, ctx)
        step["herm"], step["sparse"] = step["ops"]["herm"], step["ops"]["sparse"]
    elif op in ("pen_on", "pen_change"):
        step.update(ss._draw_pen(rng, ctx["K"]))
    elif op in ("basis_on", "basis_per_control"):
        step.update(ss._draw_basis(rng, ctx, op == "basis_per_control"))
        step["tdots"] = rng.standard_normal((3, ctx["K"], step["M"]))
    elif op in ("bounds_on", "bounds_change"):
        step["lo"], step["hi"] = bs.draw_bounds(rng, ctx["K"])
    elif op in ("rc_on", "rc_change"):
        step.update(ss._draw_rc(rng, ctx, st.ops["Xt"], int(rng.choice([1, 2, 3, 4]))))
    elif op in ("risk_on", "risk_change"):
        betas = [s * b for s in (1.0, -1.0) for b in BETAS if s * b != st.risk]
        step["beta"] = float(rng.choice(betas))
    return step


def draw_steps(rng, ctx):
    """14 to 24 steps where the flag can be set, 8 to 14 elsewhere: settings first; while the flag is set mostly a reuse or a
    call that must clear it, and a reuse again behind that call; a check behind the last setting change.  Half of the checks
    take the probes and vectors of the check before, so that the bitwise memo has something to compare.  On a context that
    serves the push-forward the walk ends with its linearity check."""
    steps, st = [], TState(ctx)
    n_steps = int(rng.integers(14, 25)) if ctx["served"] and not ctx["chunked"] else int(rng.integers(8, 15))
    checks = ["eval", "device", "batch", "fom", "controls", "observe", "observe", "observe_device", "observe_device", "vjp", "vjp_device",
              "vjp_device", "jvp", "jvp_device", "jvp_device", "vjp_reuse", "jvp_reuse", "gn_pair", "device_refused", "device_refused"]
    invalidators = ["eval", "device", "batch", "batch", "fom", "controls", "observe", "vjp", "jvp", "device_refused", "upload", "refused setting", None, None]
    cleared, again = False, None                          # the last step cleared a flag that was set; the last check
    # one in three of the contexts that can hold the flag starts under both exact modes: the two users of the shared scratch
    first = ["rc_exact", "rc_on", "traj_exact"] if ctx["served"] and not ctx["chunked"] and rng.random() < 0.35 else []
    while len(steps) < n_steps:
        last = len(steps) == n_steps - 1
        was_valid, r = st.valid is not None, rng.random()
        if first:
            op = first.pop(0)
        elif was_valid and r < 0.5 or cleared and r < 0.7:
            op = str(rng.choice(REUSE_OPS))
        elif was_valid and r < 0.85 and not last:         # the flag is set: something that must clear it
            op = invalidators[int(rng.integers(0, len(invalidators)))]
        elif not last and rng.random() < (0.8 if len(steps) < 3 else 0.3):
            op = None
        else:
            op = str(rng.choice(checks + (["risk_weights"] * 6 if st.risk is not None else [])))
        if op == "refused setting":                       # (a risk under a running cost or the reverse, if either stands)
            op = "rc_on" if st.risk is not None else "risk_on" if st.rc is not None else None
        if op is None or op in SETTING_OPS:
            step = _draw_setting(rng, ctx, st, op)
        else:
            step = dict(op=op, i=int(rng.integers(0, 3)), p=int(rng.integers(0, 3)), c=int(rng.integers(0, 2)), d=int(rng.integers(0, 3)))
            if again is not None and rng.random() < 0.5:  # the probes and vectors of the last check again: the memo compares bits
                step.update(p=again["p"], c=again["c"], d=again["d"])
                if rng.random() < 0.5:
                    step["i"] = again["i"]
            again = step
            if op == "device_refused":
                step["form"] = DEVICE_FORMS[int(rng.integers(0, 3))]
        st.apply(step)
        cleared = was_valid and st.valid is None
        steps.append(step)
    if ctx["served"]:
        step = dict(op="jvp_linear", i=int(rng.integers(0, 3)), p=int(rng.integers(0, 3)), c=0, d=int(rng.integers(0, 3)))
        st.apply(step)
        steps.append(step)
    return steps


def walk_seed(seed, contexts=CONTEXTS_PER_SEED):
    """exactly the (context, steps) pairs run_seed runs"""
    rng = np.random.default_rng(52000 + seed)
    out = []
    for _ in range(contexts):
        ctx = draw_context(rng)
        out.append((ctx, draw_steps(rng, ctx)))
    return out


def drawn_checks(steps):
    return sum(s["op"] in CHECK_OPS for s in steps)


# ---- the references -------------------------------------------------------------------------------------------------------
def close(got, ref, what):
    """|got - ref|_inf <= PARITY_RTOL |ref|_inf, per output array: the close() of test_gpu_vjp.py / test_gpu_traj_exact.py"""
    scale = np.abs(ref).max()
    err = np.abs(np.asarray(got) - ref).max()
    assert scale > 0 and err <= PARITY_RTOL * scale, f"{what}: |got-ref|_inf={err:.3e} > {PARITY_RTOL * scale:.3e}"


class Refs:
    """The references of one context, each computed once per (operator generation, physical pulse, ...) and left unchanged."""

    def __init__(self, oracle, ctx):
        self.oracle, self.ctx, self.c = oracle, ctx, {}

    def cached(self, key, make):
        if key not in self.c:
            val = make()
            for a in val if isinstance(val, tuple) else (val,):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self.c[key] = val
        return self.c[key]

    # -- in physical slice space, of explicit operators and pulse (what the mix-ups of the host test vary) --
    def composed(self, gen, ops, x, rc=None, rc_gen=0):
        """(F0, G0, member F_k, member g_k, J, G_J): the plain evaluation and the first-order running cost"""
        ctx = self.ctx
        x = np.ascontiguousarray(x, dtype=np.float64)

        def make():
            if ctx["gexact"] is None:
                F, G, parts = ss.composed_reference(self.oracle, ops, x, ctx["T"], ctx["variant"], None, rc, ctx["sys_type"])
                FJ, GJ = parts["rc"] if rc is not None else (0.0, np.zeros_like(G))
                return float(parts["plain"][0]), np.array(parts["plain"][1]), np.array(parts["members"][0]), np.array(parts["members"][1]), \
                    float(FJ), np.array(GJ)
            # (the oracle's exact path takes n x n states: n x m ones zero-padded, as test_gpu_rc_exact.py does)
            E, n, m = ops["Xi"].shape
            Xi, Xt = np.zeros((E, n, n), complex), np.zeros((E, n, n), complex)
            Xi[:, :, :m], Xt[:, :, :m] = ops["Xi"], ops["Xt"]
            F, G, mF, mG = self.oracle.ensemble_exact("UnitaryGate", ops["A"], ops["B"], Xi, Xt, ops["wts"], x, ctx["T"],
                                                      variant=ctx["variant"], objective=0 if ctx["gexact"] == "fom" else 1,
                                                      per_member=True)
            return float(F), np.array(G), np.array(mF), np.array(mG), 0.0, np.zeros_like(np.array(G))
        return self.cached(("composed", gen, rc_gen if rc is not None else None, x.tobytes()), make)

    def slices(self, gen, ops, x):
        """(P, L) of traj_exact_reference"""
        ctx = self.ctx
        x = np.ascontiguousarray(x, dtype=np.float64)
        loop = ctx["N"] * ctx["E"] * ctx["K"] <= FRECHET_LOOP_MAX
        return self.cached(("slices", gen, x.tobytes()),
                           lambda: (xr.slice_derivatives if loop else xr.slice_derivatives_eig)(ops["A"], ops["B"], x, ctx["T"], ctx["variant"]))

    def rc_exact(self, gen, ops, x, rc, rc_gen):
        ctx = self.ctx
        x = np.ascontiguousarray(x, dtype=np.float64)
        return self.cached(("rc exact", gen, rc_gen, x.tobytes()),
                           lambda: rxr.rc_exact_ref(ops["A"], ops["B"], ops["Xi"], ops["wts"], x, ctx["T"], rc["R"], rc["rho"],
                                                    ctx["variant"], self.slices(gen, ops, x)))

    def observe(self, gen, ops, x, p):
        """(y or None, X_final)"""
        ctx, probe = self.ctx, self.ctx["probes"][p]
        x = np.ascontiguousarray(x, dtype=np.float64)

        def make():
            O = probe["O"] if probe["n_obs"] else ops["Xi"][0]
            y, Xf = obr.observables_ref(ctx["sys_type"], ops["A"], ops["B"], ops["Xi"], x, ctx["T"], O,
                                        probe["per_member"] and probe["n_obs"] > 0, ctx["variant"])
            return (np.array(y) if probe["n_obs"] else None), np.array(Xf)
        return self.cached(("observe", gen, p, x.tobytes()), make)

    def vjp(self, gen, ops, x, p, mode, weights=None):
        """G (2, K, N) of the probe set's two cotangent draws (one pass: G is linear in them); weights: per-member factors
        on the cotangents (a mix-up of the host test)"""
        ctx, probe = self.ctx, self.ctx["probes"][p]
        x = np.ascontiguousarray(x, dtype=np.float64)
        E, n, m, N = ctx["E"], ctx["n"], ctx["m"], ctx["N"]

        def make():
            w = np.ones(E) if weights is None else np.asarray(weights)
            ybars = Ok = None
            if probe["n_obs"]:
                Ok = vr.probes_per_member(probe["O"], E, probe["per_member"])
                ybars = np.array([np.zeros((E, probe["n_obs"], N + 1), complex) if yb is None else yb * w[:, None, None]
                                  for yb, _ in probe["cots"]])
            xbars = np.array([np.zeros((E, n, m), complex) if xb is None else xb * w[:, None, None] for _, xb in probe["cots"]])
            if mode == "exact":
                return xr.exact_vjp_ref_many(ops["A"], ops["B"], ops["Xi"], x, ctx["T"], Ok, ybars, xbars, ctx["variant"],
                                             self.slices(gen, ops, x))
            return vr.vjp_ref_many(ops["A"], ops["B"], ops["Xi"], x, ctx["T"], Ok, ybars, xbars, ctx["variant"])
        return self.cached(("vjp", gen, p, mode, None if weights is None else np.asarray(weights).tobytes(), x.tobytes()), make)

    def jvp(self, gen, ops, x, xdot, p, mode):
        """(ydot or None, Xdot_final) of the physical direction xdot"""
        ctx, probe = self.ctx, self.ctx["probes"][p]
        x, xdot = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(xdot, dtype=np.float64)

        def tangent():
            if mode == "exact":
                return xr.exact_tangent_states(ops["A"], ops["B"], ops["Xi"], x, xdot, ctx["T"], ctx["variant"], self.slices(gen, ops, x))
            return jr.tangent_states_ref(ops["A"], ops["B"], ops["Xi"], x, xdot, ctx["T"], ctx["variant"])
        D = self.cached(("tangent", gen, mode, x.tobytes(), xdot.tobytes()), tangent)
        if not probe["n_obs"]:
            return None, D[-1]
        return jr.read_out(D, probe["O"], probe["per_member"])

    # -- of a state of the walk, in the coordinates the calls work in --
    def fg(self, st, i, gen_ops=None):
        """(F, G, p or None): plain evaluation (+ running cost by its mode | risk-weighted) + penalties, slope, projection"""
        x, s = st.physical(st.pulses()[i])
        gen, ops = gen_ops if gen_ops else (st.gen, st.ops)
        first = st.rc if st.rc_mode == "first_order" else None
        F, G, mF, mG, FJ, GJ = self.composed(gen, ops, x, first, st.rc_gen)
        G, p = np.array(G), None
        if st.rc is not None:
            if first is None:
                FJ, GJ = self.rc_exact(gen, ops, x, st.rc, st.rc_gen)
            F, G = F + FJ, G + GJ
        if st.risk is not None:
            F, G, p = rr.combine(mF, mG, ops["wts"], st.risk)
        if st.pen is not None:
            Fp, Gp = ss.penalty_ref(x, st.pen["amp"], st.pen["var"])
            F, G = F + Fp, G + Gp
        return F, st.project(G * s), p

    def observe_of(self, st, i, p):
        return self.observe(st.gen, st.ops, st.physical(st.pulses()[i])[0], p)

    def vjp_of(self, st, i, p, c):
        x, s = st.physical(st.pulses()[i])
        return st.project(self.vjp(st.gen, st.ops, x, p, st.traj_mode)[c] * s)

    def jvp_of(self, st, i, p, d, sign=1.0):
        x, s = st.physical(st.pulses()[i])
        return self.jvp(st.gen, st.ops, x, s * st.expand_dir(sign * st.dirs()[d]), p, st.traj_mode)


# ---- on the device --------------------------------------------------------------------------------------------------------
def _cm(a):
    return np.ascontiguousarray(np.swapaxes(np.asarray(a, dtype=np.complex128), -1, -2))


def _probes_cm(probe):
    return _cm(np.swapaxes(probe["O"], 0, 1) if probe["per_member"] else probe["O"])      # column-major (n, m, [E,] n_obs)


def _same(memo, key, arrays, what):
    """a later result with the same key is bit for bit the stored one"""
    arrays = tuple(None if a is None else np.array(a) for a in arrays)
    if key not in memo:
        memo[key] = (arrays, what)
        return
    for a, b in zip(arrays, memo[key][0]):
        if a is not None and b is not None:
            assert np.array_equal(a, b), f"{what}: the bits differ from those of {memo[key][1]} (key {key})"


def _expect(qoc, call, status, word, what):
    try:
        call()
    except qoc.GrapeError as exc:
        assert exc.status == status and word in str(exc), f"{what}: refused with status {exc.status}, not {status} '{word}': {exc}"
        return
    raise AssertionError(f"{what}: not refused (status {status}, '{word}' expected)")


def run_context(qoc, oracle, ctx, steps, setenv, cid, log):
    """Creates the context and walks the steps; every check against the references and the memo.  setenv(name, value or None)
    sets the environment the way the caller wants it undone.  log(line) receives each step before it runs.  Returns the
    number of checked operations (refused settings, which end in an evaluation, not counted)."""
    import torch
    setenv("GRAPE_SMALL_KERNEL", ctx["kernel"])
    setenv("GRAPE_MAX_WORKSPACE_BYTES", None if ctx["budget"] is None else str(ctx["budget"]))
    setenv("GRAPE_TRAJ_STAGED", ctx["staged"])
    n, m, K, N, E, T, mb = ctx["n"], ctx["m"], ctx["K"], ctx["N"], ctx["E"], ctx["T"], ctx["max_batch"]
    st, refs, memo, o, checks = TState(ctx), Refs(oracle, ctx), {}, ctx["ops"], 0
    kw = dict(gradient="exact", objective=ctx["gexact"]) if ctx["gexact"] else {}
    log("context: " + context_line(ctx))

    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def ptr(t):
        return 0 if t is None else t.data_ptr()

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def nan(*shape, dtype=torch.complex128):
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda")

    with qoc.GrapeEngine(ctx["sys_type"], o["A"], o["B"], o["Xi"], o["Xt"], o["wts"], T, N, variant=ctx["variant"], max_batch=mb,
                         slices_per_lane=ctx["S"], waves_per_member=ctx["W"], **kw) as eng:
        def plan():
            info = eng.info
            if ctx["full"] and not ctx["gexact"]:
                assert info["unitary_flow"] == (1 if st.ops["herm"] else 0), info
            if ctx["full"]:
                assert info["lane_pair"] == (1 if ctx["kernel"] == "pair" else 0), info
            if ctx["chunked"]:
                assert 0 < info["member_chunk"] < E, info["member_chunk"]

        # the device forms: every array stays referenced until the synchronise behind the call
        def observe_device(th, probe, bad=False):
            n_obs = probe["n_obs"]
            xd, Od = dev(th.T), dev(_probes_cm(probe)) if n_obs else None
            y = nan(E, max(n_obs, 1), N + 1) if n_obs or bad else None
            Xf, fg = nan(E, m, n), nan(xd.numel() + 1, dtype=torch.float64)
            try:
                eng.observe_device(ptr(xd), 0 if bad else n_obs, probe["per_member"], 0 if bad else ptr(Od), ptr(y), ptr(Xf), ptr(fg),
                                   stream())
            finally:
                torch.cuda.synchronize()
            return (y.cpu().numpy() if n_obs else None), np.ascontiguousarray(np.swapaxes(Xf.cpu().numpy(), -1, -2)), fg.cpu().numpy()

        def vjp_device(th, probe, cot, bad=False):
            yb, xb = probe["cots"][cot]
            n_obs = probe["n_obs"] if yb is not None else 0
            xd = None if th is None else dev(th.T)
            Od = dev(_probes_cm(probe)) if n_obs else None
            ybd = dev(yb) if yb is not None else (torch.zeros((E, 1, N + 1), dtype=torch.complex128, device="cuda") if bad else None)
            xbd = None if xb is None else dev(_cm(xb))
            G = nan(eng._cols, K, dtype=torch.float64)
            try:
                eng.observe_vjp_device(ptr(xd), 0 if bad else n_obs, probe["per_member"], 0 if bad else ptr(Od), ptr(ybd), ptr(xbd),
                                       ptr(G), stream())
            finally:
                torch.cuda.synchronize()
            return np.ascontiguousarray(G.cpu().numpy().T)

        def jvp_device(th, tdot, probe, bad=False):
            n_obs = probe["n_obs"]
            xd, xdd = None if th is None else dev(th.T), dev(tdot.T)
            Od = dev(_probes_cm(probe)) if n_obs else None
            yd = nan(E, max(n_obs, 1), N + 1) if n_obs or bad else None
            Xd = nan(E, m, n)
            try:
                eng.observe_jvp_device(ptr(xd), ptr(xdd), 0 if bad else n_obs, probe["per_member"], 0 if bad else ptr(Od), ptr(yd),
                                       ptr(Xd), stream())
            finally:
                torch.cuda.synchronize()
            return (yd.cpu().numpy() if n_obs else None), np.ascontiguousarray(np.swapaxes(Xd.cpu().numpy(), -1, -2))

        def check_fg(i, F, G, what):
            F_ref, G_ref, _ = refs.fg(st, i)
            assert_parity(F, G, F_ref, G_ref, n, what=what)
            _same(memo, st.fg_key(i), (np.float64(F), G), what)

        def check_observe(i, p, y, Xf, what):
            y_ref, X_ref = refs.observe_of(st, i, p)
            if y_ref is not None:
                close(y, y_ref, what + " y")
            close(Xf, X_ref, what + " X_final")
            _same(memo, st.traj_key("observe", i, p), (y, Xf), what)

        def check_vjp(i, p, c, G, what):
            close(G, refs.vjp_of(st, i, p, c), what + " G")
            _same(memo, st.traj_key("vjp", i, p, c), (G,), what)

        def check_jvp(i, p, d, yd, Xd, what):
            y_ref, X_ref = refs.jvp_of(st, i, p, d)
            if y_ref is not None:
                close(yd, y_ref, what + " ydot")
                assert not yd[:, :, 0].any(), what + ": ydot[0] is zero and written"
            close(Xd, X_ref, what + " Xdot_final")
            _same(memo, st.traj_key("jvp", i, p, d), (yd, Xd), what)

        plan()
        for si, step in enumerate(steps):
            op = step["op"]
            log(f"step {si}: {step_line(step)}")
            what = f"step {si} {op}"
            if op in SETTING_OPS:
                refusal = st.setting_refusal(op)

                def setting():
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
                    elif op in ("bounds_on", "bounds_change"):
                        eng.set_bounds(step["lo"], step["hi"])
                    elif op == "bounds_off":
                        eng.set_bounds(None)
                    elif op in ("rc_on", "rc_change"):
                        eng.set_running_cost(step["R"], step["rho"])
                    elif op == "rc_off":
                        eng.set_running_cost(None)
                    elif op in ("traj_exact", "traj_first"):
                        eng.set_trajectory_derivative("exact" if op == "traj_exact" else "first_order")
                    elif op in ("rc_exact", "rc_first"):
                        eng.set_running_cost_derivative("exact" if op == "rc_exact" else "first_order")
                    elif op in ("risk_on", "risk_change"):
                        eng.set_risk(step["beta"])
                    elif op == "risk_off":
                        eng.set_risk(0.0)
                    else:
                        raise AssertionError(f"unknown step {op}")
                if refusal:
                    _expect(qoc, setting, refusal[0], refusal[1], what)
                else:
                    setting()
                st.apply(step)
                if op == "upload":
                    plan()
                if refusal:                               # the refused call has cleared the flag as every grape_set_* does: a
                    why = st.reuse_refusal()              # reuse right behind it, before anything evaluates
                    _expect(qoc, lambda: vjp_device(None, ctx["probes"][si % 3], 0), why[0], why[1], what + " refused, then a reuse")
                    i = si % 3                            # ... and it left the evaluation what it was
                    F, G = eng.eval(st.pulses()[i])
                    check_fg(i, F, G, what + " refused, then eval")
                    st.clear("eval")
                continue
            checks += 1
            i, p, c, d = step["i"], step["p"], step["c"], step["d"]
            probe = ctx["probes"][p]
            th = st.pulses()[i]
            yb, xb = probe["cots"][c]
            O = probe["O"]
            refusal = st.reuse_refusal() if op in REUSE_OPS else st.traj_refusal(op)
            if op in REUSE_OPS and refusal is None:
                i = st.valid[1]                           # the trajectory in the workspace is that pulse's
                what += f" along pulse {i} of {st.valid[0]}"
            if op == "eval":
                F, G = eng.eval(th)
                check_fg(i, F, G, what)
            elif op == "device":
                xd = dev(th.T)
                fg = torch.zeros(xd.numel() + 1, dtype=torch.float64, device="cuda")
                eng.eval_device(xd.data_ptr(), fg.data_ptr(), stream())
                torch.cuda.synchronize()
                h = fg.cpu().numpy()
                check_fg(i, h[-1], h[:-1].reshape(th.shape[1], K).T, what)
            elif op == "batch":
                idx = [(i + b) % 3 for b in range(mb)]
                Fs, Gs = eng.eval_batch(np.array([st.pulses()[j] for j in idx]))
                for b, j in enumerate(idx):
                    check_fg(j, Fs[b], Gs[b], f"{what} entry {b}")
            elif op == "fom":
                F_ref, G_ref, _ = refs.fg(st, i)
                assert_parity(eng.fom(th), G_ref, F_ref, G_ref, n, what=what)
            elif op == "controls":
                x_ref = st.physical(th)[0]
                xc = eng.controls(th)
                assert xc.shape == (K, N) and np.abs(xc - x_ref).max() <= 1e-10 * max(1.0, np.abs(x_ref).max()), f"{what}: physical pulse"
            elif op == "risk_weights":
                F, G = eng.eval(th)
                check_fg(i, F, G, what)
                p_ref = refs.fg(st, i)[2]
                W = st.ops["wts"].sum()
                pk = eng.risk_weights()
                assert np.abs(pk - p_ref).max() <= 1e-10 * W and abs(pk.sum() - W) <= 1e-10 * W, f"{what}: p"
            elif op == "observe":
                def call():
                    return eng.observe(th, O, per_member=probe["per_member"], final=True, want_F=True)
                if refusal:
                    _expect(qoc, call, refusal[0], refusal[1], what)
                else:
                    y, Xf, F = call()
                    check_observe(i, p, y, Xf, what)
                    F_ref, G_ref, _ = refs.fg(st, i)
                    assert_parity(F, G_ref, F_ref, G_ref, n, what=what + " F")
                    key = st.fg_key(i)
                    assert key not in memo or memo[key][0][0] == F, f"{what}: F is not grape_eval's bit for bit"
            elif op == "observe_device":
                if refusal:
                    _expect(qoc, lambda: observe_device(th, probe), refusal[0], refusal[1], what)
                else:
                    y, Xf, fg = observe_device(th, probe)
                    check_observe(i, p, y, Xf, what)
                    check_fg(i, fg[-1], fg[:-1].reshape(th.shape[1], K).T, what + " fg")
            elif op == "vjp":
                def call():
                    return eng.observe_vjp(th, O if yb is not None else None, ybar=yb, xbar_final=xb, per_member=probe["per_member"])
                if refusal:
                    _expect(qoc, call, refusal[0], refusal[1], what)
                else:
                    check_vjp(i, p, c, call(), what)
            elif op in ("vjp_device", "vjp_reuse"):
                reuse = op == "vjp_reuse"
                if refusal:
                    _expect(qoc, lambda: vjp_device(None if reuse else th, probe, c), refusal[0], refusal[1], what)
                else:
                    check_vjp(i, p, c, vjp_device(None if reuse else th, probe, c), what)
            elif op in ("jvp", "jvp_linear"):
                tdot = st.dirs()[d]

                def call(sign=1.0):
                    return eng.observe_jvp(th, sign * tdot, O, per_member=probe["per_member"], final=True)
                if refusal:
                    _expect(qoc, call, refusal[0], refusal[1], what)
                else:
                    yd, Xd = call()
                    check_jvp(i, p, d, yd, Xd, what)
                    if op == "jvp_linear":                # every operation is linear in xdot: -xdot returns the negated bits
                        ym, Xm = call(-1.0)
                        assert (yd is None or np.array_equal(ym, -yd)) and np.array_equal(Xm, -Xd), f"{what}: -xdot"
            elif op in ("jvp_device", "jvp_reuse"):
                reuse = op == "jvp_reuse"
                tdot = st.dirs()[d]
                if refusal:
                    _expect(qoc, lambda: jvp_device(None if reuse else th, tdot, probe), refusal[0], refusal[1], what)
                else:
                    yd, Xd = jvp_device(None if reuse else th, tdot, probe)
                    check_jvp(i, p, d, yd, Xd, what)
            elif op == "gn_pair":                         # J v, then J' w, along one stored trajectory
                tdot = st.dirs()[d]
                if refusal:
                    _expect(qoc, lambda: jvp_device(None, tdot, probe), refusal[0], refusal[1], what + " J v")
                    _expect(qoc, lambda: vjp_device(None, probe, c), refusal[0], refusal[1], what + " J' w")
                else:
                    yd, Xd = jvp_device(None, tdot, probe)
                    check_jvp(i, p, d, yd, Xd, what + " J v")
                    G = vjp_device(None, probe, c)
                    check_vjp(i, p, c, G, what + " J' w")
                    lhs, mag = jr.pairing(yb, yd, xb, Xd)
                    rhs = float(np.sum(G * tdot))
                    assert abs(lhs - rhs) <= 1e-12 * mag, f"{what}: <cot, J v> = {lhs!r}, <J' cot, v> = {rhs!r}, sum of |terms| {mag!r}"
            elif op == "device_refused":                  # n_obs = 0 with a non-null y / ybar / ydot: INVALID_ARG behind the
                form = step["form"]                       # context's own refusals; a failed device form clears the flag
                status, word = st.traj_refusal(form) or (INVALID_ARG, "n_obs = 0")
                bad = dict(probe, cots=[(None, probe["cots"][0][1] if probe["cots"][0][1] is not None else probe["cots"][1][1])])
                call = {"observe_device": lambda: observe_device(th, probe, bad=True),
                        "vjp_device": lambda: vjp_device(th, bad, 0, bad=True),
                        "jvp_device": lambda: jvp_device(th, st.dirs()[d], probe, bad=True)}[form]
                _expect(qoc, call, status, word, f"{what} {form}")
            else:
                raise AssertionError(f"unknown step {op}")
            st.apply(step)
    return checks


def run_seed(qoc, oracle, seed, setenv, log, contexts=CONTEXTS_PER_SEED):
    """the contexts of one seed; returns (contexts walked, checked operations, checks drawn)"""
    checks = drawn = 0
    for ci, (ctx, steps) in enumerate(walk_seed(seed, contexts)):
        done = run_context(qoc, oracle, ctx, steps, setenv, (seed, ci), log)
        assert done == drawn_checks(steps), (seed, ci, done, drawn_checks(steps))
        checks, drawn = checks + done, drawn + drawn_checks(steps)
    return contexts, checks, drawn


# ---- what the walks cover, from the model alone -----------------------------------------------------------------------------
def runs(st, step):
    """the model's word on a check step: True when the call runs (for device_refused: when the argument check is what refuses
    it), False when the context, the flag or the member chunk refuses it"""
    op = step["op"]
    if op in OLD_CHECK_OPS + ("risk_weights",):
        return True
    if op in REUSE_OPS:
        return st.reuse_refusal() is None
    return st.traj_refusal(step["form"] if op == "device_refused" else op) is None


def coverage(seeds=SEEDS, contexts=CONTEXTS_PER_SEED):
    """Counter over the walks of `seeds`: ("op", op, condition) for the checks that RUN and ("refused", op, condition) for
    those that are refused (the refusal is then the assertion), ("accepted", reuse op, device form behind it),
    ("refused reuse", class of the invalidator), ("refusal", op, word), ("staged", probe count, GRAPE_TRAJ_STAGED),
    ("E=33 vjp",), ("refused setting, flag set",), "contexts", "checks", "checks that run", "refused settings"."""
    cnt = Counter()
    for seed in seeds:
        for ctx, steps in walk_seed(seed, contexts):
            st = TState(ctx)
            cnt["contexts"] += 1
            for step in steps:
                op = step["op"]
                if op in SETTING_OPS:
                    why = st.setting_refusal(op)
                    if why:
                        cnt[("refusal", "rc_on" if op == "rc_change" else "risk_on" if op == "risk_change" else op, why[1])] += 1
                        cnt["refused settings"] += 1
                        if st.valid is not None:
                            cnt[("refused setting, flag set",)] += 1
                    st.apply(step)
                    if why:
                        st.clear("eval")
                    continue
                ok = runs(st, step)
                cnt["checks"] += 1
                cnt["checks that run"] += ok
                for cond in ["any"] + st.conditions():
                    cnt[("op" if ok else "refused", op, cond)] += 1
                probe = ctx["probes"][step["p"]]
                if op in REUSE_OPS:
                    why = st.reuse_refusal()
                    if why is None:
                        cnt[("accepted", op, st.valid[0])] += 1
                    elif why[0] == NOT_READY:
                        cnt[("refused reuse", "chunked context" if ctx["chunked"] else st.cleared_by)] += 1
                    else:
                        cnt[("refusal", op, why[1])] += 1
                elif not ok:
                    cnt[("refusal", op, st.traj_refusal(step["form"] if op == "device_refused" else op)[1])] += 1
                elif op in ("observe_device", "vjp_device") and probe["n_obs"] in (8, 9, 16) and ctx["staged"] is not None:
                    if op == "observe_device" or probe["cots"][step["c"]][0] is not None:
                        cnt[("staged", probe["n_obs"], ctx["staged"])] += 1
                if ok and op in REUSE_OPS and st.traj_mode == "exact" and st.rc is not None and st.rc_mode == "exact":
                    cnt[("exact pair under an exact running cost", op)] += 1      # (the two users of d_traj_w, one stored trajectory)
                if ok and ctx["E"] == 33 and op in ("vjp", "vjp_device", "vjp_reuse", "gn_pair"):
                    cnt[("E=33 vjp",)] += 1
                st.apply(step)
    return cnt
