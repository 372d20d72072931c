"""The family walk: random walks over the trajectory calls as they are today -- the walk of tests/trajectory_sequences.py (its
contexts, settings, old check ops, model, references and bitwise memo) extended by the entry points that came after it:
grape_eval_vjp_multi, grape_eval_jvp_multi, grape_eval_hvp, grape_eval_gnvp (host form, device form and d_x = NULL reuse each)
and the ensemble-averaged host forms grape_eval_observables_mean / _vjp_mean / _jvp_mean.  These calls describe themselves
through the older calls' per-call fields and scratch on the context, so a call is correct only if every such field is set
again or restored: the walk runs them against each other, against the older calls and across setting changes.  Shared by
test_gpu_trajectory_family_soak.py (runs the walks on the device), test_trajectory_family_host.py (shows on the CPU what the
committed seeds cover and that no mix-up can hide) and tools/soak_trajectory.py --family.  No test functions here.
trajectory_sequences.py itself is untouched: its walk draws what it always drew.

  draw_context / draw_steps   pure functions of the generator state: they never touch the library.
  FState               trajectory_sequences.TState + the header's sentences on the new forms: the four new device forms set the
                       "trajectory valid" flag under the conditions of the old ones, the four new reuse forms need it and keep
                       it, the seven new host forms clear it, a failed call of any device form clears it; grape_eval_hvp is
                       refused under bounds, then in the exact mode, grape_eval_gnvp in the exact mode, both behind the
                       context's own refusals and in front of the argument checks and the NOT_READY of a reuse.
  FRefs                trajectory_sequences.Refs + hvp_reference, gnvp_reference, traj_mean_reference.  No device result
                       enters them.
  run_context          one context and its steps on the device.
  coverage             what the walks of a set of seeds observe, from the model alone.
"""
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnvp_reference as gr  # noqa: E402
import hvp_reference as hr  # noqa: E402
import jvp_reference as jr  # noqa: E402
import settings_sequences as ss  # noqa: E402
import traj_exact_reference as xr  # noqa: E402
import traj_mean_reference as tm  # noqa: E402
import trajectory_sequences as ts  # noqa: E402
import vjp_reference as vr  # noqa: E402
from conftest import PARITY_RTOL, assert_parity  # noqa: E402
from gnvp_cases import psd_blocks  # noqa: E402
from rc_reference import propagators  # noqa: E402
from trajectory_sequences import INVALID_ARG, NOT_READY, SETTING_OPS, UNSUPPORTED, _cm, _cplx, _expect, _probes_cm, _same, close  # noqa: E402

# (seed 72 is left out: one of its contexts has N = 1 and a probe set without probes, where every Gauss-Newton product is
# wf tr(V' B' X_1 X_1') with X_1 X_1' next to the identity whatever the pulse -- the host test's named exceptions would pass
# their cap of 10 % of the seed's checks there)
SEEDS = tuple(s for s in range(97) if s != 72)
CONTEXTS_PER_SEED = 4
BASE_SEED = 86000                                         # (trajectory_sequences.walk_seed: 52000)
POOL = 8                                                  # directions, and cotangent pairs per probe set
MULTI_COUNTS = (1, 2, 3, 5, 8)                            # one, a full block for every <n, m>, blocks with a lone remainder
MAX_MULTI = 8                                             # GRAPE_MAX_VJP_COTANGENTS = GRAPE_MAX_JVP_DIRECTIONS
MULTI_MAX_THREADS = 256                                   # kVjpMultiMaxThreads = kJvpMultiMaxThreads (grape_kernels.hpp)
LONG_N = 257                                              # the smallest N with more than 256 time chunks at slices_per_lane = 1
ENV = (None, "0", "1")
HOST_NEW = ("vjp_multi", "jvp_multi", "hvp", "gnvp", "observe_mean", "vjp_mean", "jvp_mean")
DEVICE_NEW = ("vjp_multi_device", "jvp_multi_device", "hvp_device", "gnvp_device")
REUSE_NEW = ("vjp_multi_reuse", "jvp_multi_reuse", "hvp_reuse", "gnvp_reuse")
LOOPS = ("newton_cg", "gn_cg")
FAMILY_CHECK_OPS = HOST_NEW + DEVICE_NEW + REUSE_NEW + LOOPS + ("linear",)
CHECK_OPS = ts.CHECK_OPS + FAMILY_CHECK_OPS
DEVICE_FORMS = ts.DEVICE_FORMS + DEVICE_NEW               # the seven forms that set the flag
REUSE_OPS = ts.REUSE_OPS + REUSE_NEW                      # the seven reuse kinds (gn_pair: the older Gauss-Newton pair)
ALL_REUSE = REUSE_OPS + LOOPS
# the arguments the header lists as GRAPE_ERR_INVALID_ARG for the new device forms, and the words of their messages
BAD_ARGS = {"vjp_multi_device": (("n_set", 0, "n_set = 0"), ("n_set", MAX_MULTI + 1, f"n_set = {MAX_MULTI + 1}")),
            "jvp_multi_device": (("n_dir", 0, "n_dir = 0"), ("n_dir", MAX_MULTI + 1, f"n_dir = {MAX_MULTI + 1}")),
            "hvp_device": (("ybar_dot", 0, "n_obs = 0 with a non-null ybar_dot"),),
            "gnvp_device": (("no weights", 0, "wy and wf are both null"), ("w_per_member", 2, "w_per_member = 2"))}
FAMILY_KERNELS = ("trajectory_hvp_kernel", "trajectory_gnvp_kernel", "traj_mean_reduce_kernel", "traj_mean_combine_kernel",
                  "traj_mean_broadcast_kernel", "trajectory_jvp_kernel", "trajectory_jvp_exact_kernel", "trajectory_jvp_multi_kernel",
                  "trajectory_jvp_multi_exact_kernel", "trajectory_vjp_kernel", "trajectory_vjp_exact_kernel",
                  "trajectory_vjp_multi_kernel", "trajectory_vjp_staged_kernel", "vjp_sum_kernel")


def base(op):
    """the call an op goes through: "hvp_device" -> "hvp" """
    for tail in ("_device", "_reuse"):
        if op.endswith(tail):
            return op[:-len(tail)]
    return op


# ---- contexts -------------------------------------------------------------------------------------------------------------
def _draw_probes(rng, ctx, which, counts):
    """One probe set (O_0 = Xi, so that |y|_inf is of order 1) and its pools: eight cotangent pairs, two cotangent tangents for
    the HVP, the Gauss-Newton weights.  "cots" lists every pair in its three forms -- entry 3 j + f of pair j: both (f = 0),
    ybar only (1), Xbar only (2) -- and without probes the eight Xbar alone.  Pair 0 of the third set has whole zero rows."""
    n, m, E, N = ctx["n"], ctx["m"], ctx["E"], ctx["N"]
    n_obs = int(rng.choice(counts))
    per_member = bool(rng.integers(0, 2))
    O = None
    if n_obs:
        O = _cplx(rng, E, n_obs, n, m) if per_member else _cplx(rng, n_obs, n, m)
        if per_member:
            O[:, 0] = ctx["ops"]["Xi"]
        else:
            O[0] = ctx["ops"]["Xi"][0]
    yb = _cplx(rng, POOL, E, n_obs, N + 1) if n_obs else None
    xb = _cplx(rng, POOL, E, n, m)
    ybd = _cplx(rng, 2, E, n_obs, N + 1) if n_obs else None
    xbd = _cplx(rng, 2, E, n, m)
    wf_pos, wf_mixed = rng.uniform(0.2, 1.5, E), rng.uniform(0.2, 1.5, E)
    wf_mixed[0] = -wf_mixed[0]                                # a negative entry; and with two members or more a zero entry
    if E > 1:
        wf_mixed[1] = 0.0
    if n_obs:
        if which == 2:
            yb[0][:, :, ::3] = 0.0                            # whole zero rows in s (s = 0 among them; s = 1 stays)
        cots = [pair for j in range(POOL) for pair in ((yb[j], xb[j]), (yb[j], None), (None, xb[j]))]
        tans = [(ybd[0], xbd[0]), (ybd[1], None)]             # both, and one alone
        indef = rng.standard_normal((3, n_obs, N + 1))        # indefinite blocks with a non-zero ri plane
        weights = [dict(w=psd_blocks(rng, n_obs, N + 1), blocks=True, member=False, wf=wf_pos, name="psd"),
                   dict(w=indef, blocks=True, member=False, wf=wf_mixed, name="indefinite"),
                   dict(w=rng.uniform(0.2, 1.5, (n_obs, N + 1)), blocks=False, member=False, wf=None, name="scalar"),
                   dict(w=None, blocks=None, member=False, wf=wf_mixed, name="final"),
                   dict(w=psd_blocks(rng, E, n_obs, N + 1), blocks=True, member=True, wf=wf_mixed, name="psd per member")]
    else:
        cots = [(None, xb[j]) for j in range(POOL)]
        tans = [(None, xbd[0]), (None, xbd[1])]
        weights = [dict(w=None, blocks=None, member=False, wf=wf_pos, name="final"),
                   dict(w=None, blocks=None, member=False, wf=wf_mixed, name="final mixed")]
    return dict(n_obs=n_obs, per_member=per_member, O=O, cots=cots, tans=tans, weights=weights)


def draw_context(rng):
    """trajectory_sequences.draw_context, then from the same generator: one context in seven of the more-than-256-chunks kind
    among those that can hold the flag (a lane kernel at n = 2 or 3 -- the only ones whose workgroups pass 256 threads --,
    N = 257 at slices_per_lane = 1, E <= 2, K <= 2, n_obs <= 3), eight directions, the probe sets with their pools, and the
    member weights of the mean forms."""
    ctx = ts.draw_context(rng)
    ctx["long"] = bool(ctx["served"] and not ctx["chunked"] and rng.random() < 0.15)
    if ctx["long"]:
        n = ctx["n"] = int(rng.choice([2, 3]))
        ctx.update(m=int(rng.integers(1, n + 1)), K=int(rng.choice([1, 2])), E=int(rng.choice([1, 2])), N=LONG_N, kernel="lane", S=1, W=0)
        ctx["ops"] = ss.full_operators(rng, ctx)
        ctx["pool"] = rng.uniform(-1, 1, (3, ctx["K"], ctx["N"]))
    ctx["xdots"] = rng.standard_normal((POOL, ctx["K"], ctx["N"]))
    ctx["probes"] = [_draw_probes(rng, ctx, which, (0, 1, 3) if ctx["long"] else ts.PROBE_COUNTS) for which in range(3)]
    v = np.ones(1)
    if ctx["E"] > 1:                                          # a signed draw with one exact zero
        v = rng.standard_normal(ctx["E"])
        v[int(rng.integers(0, ctx["E"]))] = 0.0
    ctx["vs"] = [None, v]                                     # None: the ensemble weights
    return ctx


def context_line(ctx):
    return ts.context_line(ctx) + (" long" if ctx["long"] else "")


def step_line(step):
    op = step["op"]
    keys = ["i", "p"]
    if op in CHECK_OPS:
        b = base(op)
        keys += {"vjp_multi": ["cs", "vm"], "jvp_multi": ["ds", "jm"], "hvp": ["c", "d", "t"], "gnvp": ["d", "w", "wm"],
                 "observe_mean": ["v", "col"], "vjp_mean": ["c", "v"], "jvp_mean": ["d", "v"], "newton_cg": ["c", "d", "t"],
                 "gn_cg": ["d", "w", "wm"], "linear": ["c", "d", "t", "w"], "device_refused": ["form", "arg"]}.get(b, ["c", "d"])
    keys += ["J", "kind", "M", "herm", "sparse", "offset", "beta", "lo", "hi"]
    extra = {k: step[k] for k in keys if k in step and step[k] is not None}
    return op + (" " + str(extra) if extra else "")


# ---- the model ------------------------------------------------------------------------------------------------------------
class FState(ts.TState):
    """trajectory_sequences.TState and the header's sentences on the new forms"""

    def family_refusal(self, op):
        """what the context and the settings answer a call of the family, whatever its arguments: None, or (status, word).
        grape_eval_hvp: "Served: the contexts grape_eval_vjp serves, refused with its reasons first.  Two refusals of this call
        alone follow them" -- "bounds", then "trajectory_derivative" (hvp_check's order); grape_eval_gnvp: "One refusal of this
        call alone follows them" -- "trajectory_derivative"; the mean forms: "Served and refused exactly where the underlying
        call is"; the multi forms: "Every other argument check, refusal (checked first) ... is grape_eval_vjp's"."""
        b = base(op)
        if b in ("observe", "observe_mean"):
            return self.traj_refusal("observe")
        why = self.traj_refusal()
        if why:
            return why
        if b == "hvp" and self.bounds is not None:
            return (UNSUPPORTED, "bounds")
        if b in ("hvp", "gnvp") and self.traj_mode == "exact":
            return (UNSUPPORTED, "trajectory_derivative")
        return None

    def reuse_refusal_of(self, op):
        """what a d_x = NULL call of the form answers now: the call's own refusals, then the rule of the flag"""
        why = self.family_refusal(op)
        if why:
            return why
        if self.ctx["chunked"]:
            return (NOT_READY, "member_chunk")
        if self.valid is None:
            return (NOT_READY, "reuse")
        return None

    def parts(self, step):
        """the calls of a step in their order, as (form, reuse): the loops are sequences of reuse calls"""
        op = step["op"]
        if op == "newton_cg":
            return [("jvp", True), ("hvp", True)]
        if op == "gn_cg":
            return [("gnvp", True), ("gnvp", True), ("jvp", True), ("vjp", True)]
        if op == "gn_pair":
            return [("jvp", True), ("vjp", True)]
        return [(base(op), op.endswith("_reuse"))]

    def step_refusal(self, step):
        """the refusal of the step's first refused call, or None when all of them run"""
        op = step["op"]
        if op in ALL_REUSE:
            for form, _ in self.parts(step):
                why = self.reuse_refusal_of(form)
                if why:
                    return why
            return None
        if op == "device_refused":
            return self.family_refusal(step["form"])
        if op in ("jvp_linear", "linear"):
            return self.traj_refusal()
        if op in ts.OLD_CHECK_OPS + ("risk_weights",):
            return None
        return self.family_refusal(op)

    def apply(self, step):
        op = step["op"]
        if op not in FAMILY_CHECK_OPS:
            super().apply(step)
            return
        self.refusal, self.refused = None, False
        if op in HOST_NEW or op == "linear":
            self.clear("family host form")
        elif op in DEVICE_NEW:
            if self.family_refusal(op):
                self.clear("refused device call")
            elif self.ctx["chunked"]:
                self.clear("chunked context")
            else:
                self.valid = (op, step["i"])
        elif self.step_refusal(step):                         # the reuse forms and the loops: a failed call clears the flag
            self.clear("refused device call")

    def traj_key(self, kind, i, *rest):
        """trajectory_sequences' key; the read-outs, averaged or not, do not depend on the derivative mode"""
        if kind == "observe_mean":
            return (kind, self.gen, self.basis_gen, self.bounds_gen, i) + rest
        return super().traj_key(kind, i, *rest)

    def settings_key(self):
        """everything a call's scratch may be sized by, besides the call itself"""
        rc = (self.rc_gen, self.rc_mode) if self.rc is not None else None
        return (self.gen, self.basis_gen, self.bounds_gen, self.pen_gen if self.pen is not None else None, rc, self.risk,
                self.traj_mode, self.rc_mode)

    def images(self, step):
        """the E_t images a jvp_multi call keeps side by side in the exact mode (jvp_exact_images, grape_api.cpp)"""
        n, m = self.ctx["n"], self.ctx["m"]
        block = 8 if n == 2 else 4 if n == 3 else 3 if m <= 2 else 2
        return 1 if step["jm"] == "0" or self.ctx["long"] else min(len(step["ds"]), block)


# ---- steps ----------------------------------------------------------------------------------------------------------------
def same_form(probe, c):
    """the entries of the probe set's cotangent pool in the form of entry c: what one multi call can take"""
    return list(range(c % 3, 3 * POOL, 3)) if probe["n_obs"] else list(range(POOL))


def has_ybar(probe, c):
    return probe["cots"][c][0] is not None


def _draw_setting(rng, ctx, st, forced=None):
    step = ts._draw_setting(rng, ctx, st, forced)
    if step["op"] in ("basis_on", "basis_per_control"):
        step["tdots"] = rng.standard_normal((POOL, ctx["K"], step["M"]))
    return step


def _draw_check(rng, ctx, op, again):
    """every field any check op reads, drawn for all of them alike"""
    step = dict(op=op, i=int(rng.integers(0, 3)), p=int(rng.integers(0, 3)))
    full = [q for q in range(3) if ctx["probes"][q]["n_obs"] == 16]
    probe = ctx["probes"][step["p"]]
    step.update(c=int(rng.integers(0, len(probe["cots"]))), d=int(rng.integers(0, POOL)), t=int(rng.integers(0, 2)),
                w=int(rng.integers(0, len(probe["weights"]))), v=int(rng.integers(0, 2)))
    if again is not None and rng.random() < 0.5:              # the probes and vectors of the last check again: the memo compares bits
        step.update({k: again[k] for k in ("p", "c", "d", "t", "w", "v")})
        probe = ctx["probes"][step["p"]]
        if rng.random() < 0.5:
            step["i"] = again["i"]
    elif op == "observe_mean" and full and rng.random() < 0.8:    # (d_mean_io only grows: 16 probes, then 1, then 16 again)
        step["p"] = full[0]
        probe = ctx["probes"][step["p"]]
        step.update(c=int(rng.integers(0, len(probe["cots"]))), w=int(rng.integers(0, len(probe["weights"]))))
    step["wm"] = int(rng.integers(0, 2))                      # shared weights handed over in the per-member shape
    step["jm"], step["vm"] = ENV[int(rng.integers(0, 3))], ENV[int(rng.integers(0, 3))]
    # subsets with repetition and out of order, so that block position and pool index are decoupled; the step's own c and d
    # are among them
    pool = same_form(probe, step["c"])
    cs = [pool[int(j)] for j in rng.integers(0, len(pool), int(rng.choice(MULTI_COUNTS)))]
    ds = [int(j) for j in rng.integers(0, POOL, int(rng.choice(MULTI_COUNTS)))]
    cs[int(rng.integers(0, len(cs)))] = step["c"]
    ds[int(rng.integers(0, len(ds)))] = step["d"]
    step.update(cs=cs, ds=ds, col=None)
    if op == "observe_mean" and probe["n_obs"] == 16 and rng.random() < 0.3:
        step["col"] = int(rng.integers(0, 16))                # the 1-probe call with probe col: column col of the 16-probe call
    if op == "device_refused":
        step["form"] = DEVICE_FORMS[int(rng.integers(0, len(DEVICE_FORMS)))]
        step["arg"] = int(rng.integers(0, 2))
    return step


def _follow(rng, ctx, st, step):
    """The adjacent pairs the shared fields make dangerous (the table of the walk's description): the steps to run right
    behind `step`, on its pulse and probe set, so that the memo key of the second exists already or will recur.  Entries are
    check steps, or ("flip",): an operator re-upload that flips the data flow."""
    op, b = step["op"], base(step["op"])
    hold = ctx["served"] and not ctx["chunked"]
    probe = ctx["probes"][step["p"]]

    def then(new_op, **over):
        nxt = dict(step, op=new_op, jm=ENV[int(rng.integers(0, 3))], vm=ENV[int(rng.integers(0, 3))], col=None)
        nxt.update(over)
        return nxt

    def kind(stem):                                           # host form, device form, or the reuse behind a device form
        forms = [stem, stem + "_device"] + ([stem + "_reuse"] * 2 if hold and op != b else [])
        return forms[int(rng.integers(0, len(forms)))]

    r = rng.random()
    if b == "vjp_multi":
        if len(step["cs"]) >= 2 and st.rc is not None and r < 0.5:
            return [then(["eval", "device", "batch"][int(rng.integers(0, 3))])]
        return [then(kind("vjp"), c=step["cs"][int(rng.integers(0, len(step["cs"])))])]
    if b == "jvp_multi":
        if st.traj_mode == "exact" and st.images(step) > 1 and r < 0.6:
            return [then("eval")] if st.rc is not None and st.rc_mode == "exact" and r < 0.3 else [then(kind("vjp"))]
        return [then(kind("jvp"), d=step["ds"][int(rng.integers(0, len(step["ds"])))])]
    if b == "hvp":
        return [("flip",), then(op)] if r < 0.25 else [then(kind("vjp"))]
    if b == "gnvp":
        if r < 0.25:
            return [("flip",), then(op)]
        if r < 0.6:
            return [then(kind("hvp")), then(op)]
        pool = [c for c in same_form(probe, step["c"]) if has_ybar(probe, c)] or [c for c in range(len(probe["cots"])) if has_ybar(probe, c)]
        return [then(kind("vjp"), c=pool[int(rng.integers(0, len(pool)))] if pool else step["c"])]
    if b == "observe_mean" and probe["n_obs"] == 16 and step["col"] is None and r < 0.8:
        return [then(op, col=int(rng.integers(0, 16))), then(op)]
    if b in ("observe_mean", "vjp_mean", "jvp_mean"):
        return [then(["observe", "vjp", "jvp"][int(rng.integers(0, 3))])]
    return []


def draw_steps(rng, ctx):
    """24 to 40 steps where the flag can be set, 14 to 22 on the member-chunked contexts, 9 to 15 where the family is refused,
    8 to 12 on the long contexts (whose references are the slowest).  trajectory_sequences' policy -- settings first; while the flag is set mostly a reuse of any kind or a call
    that must clear it, and a reuse again behind that call; half of the checks repeat the previous check's probes and vectors
    -- and behind six in ten of the family's calls (a third of the device forms, behind which the reuse kinds are drawn freely)
    the adjacent pair of _follow.  On a context that serves the push-forward the
    walk ends with the linearity checks."""
    steps, st = [], FState(ctx)
    hold = ctx["served"] and not ctx["chunked"]
    n_steps = int(rng.integers(8, 13)) if ctx["long"] else int(rng.integers(24, 41)) if hold else int(rng.integers(14, 23)) if ctx["served"] else int(rng.integers(9, 16))
    checks = (list(ts.OLD_CHECK_OPS) + ["observe", "observe_device", "vjp", "vjp_device", "jvp", "jvp_device", "vjp_reuse", "jvp_reuse",
                                        "gn_pair", "device_refused", "device_refused"]
              + list(HOST_NEW) * 2 + ["hvp", "gnvp"] * 2 + list(DEVICE_NEW) * 3 + list(REUSE_NEW) + list(LOOPS))
    reuses = list(ALL_REUSE) + ["hvp_reuse", "gnvp_reuse"] + list(LOOPS)
    devices = list(DEVICE_FORMS) * 2 + ["hvp_device", "gnvp_device"]
    # (hvp_device / gnvp_device: refused by a setting they clear the flag, served they set it anew)
    invalidators = ["eval", "device", "batch", "fom", "controls", "observe", "vjp", "jvp", "upload", "refused setting", None, None] \
        + ["device_refused"] * 5 + ["hvp_device", "gnvp_device"] + list(HOST_NEW)
    cleared, again, queue = False, None, []

    def pick(ops):
        """one of ops; three times in four one that the settings in force do not refuse, where there is one"""
        ops = list(ops)
        serve = [o_ for o_ in ops if st.step_refusal(dict(op=o_, form="vjp_device")) is None]
        if serve and ctx["served"] and rng.random() < 0.75:   # (elsewhere the refusals are what there is to walk)
            ops = serve
        return ops[int(rng.integers(0, len(ops)))]

    first = ["rc_exact", "rc_on", "traj_exact"] if hold and rng.random() < 0.35 else []
    while len(steps) < n_steps or queue:
        last = len(steps) >= n_steps - 1 and not queue
        was_valid, r = st.valid is not None, rng.random()
        step = None
        if queue:
            step = queue.pop(0)
            if step == ("flip",):
                ops = ss._full_operators(rng, ctx, not st.ops["herm"], bool(rng.integers(0, 2)))
                step = dict(op="upload", ops=ops, herm=ops["herm"], sparse=ops["sparse"])
            op = step["op"]
        elif first:
            op = first.pop(0)
        elif was_valid and r < 0.65:
            op = pick(reuses)
        elif cleared and r < 0.6:                             # behind the call that cleared the flag: a reuse, to be refused
            op = str(rng.choice(ALL_REUSE))
        elif was_valid and r < 0.85 and not last:             # the flag is set: something that must clear it
            op = invalidators[int(rng.integers(0, len(invalidators)))]
        elif hold and not was_valid and rng.random() < 0.4:
            op = pick(devices)
        elif not last and rng.random() < (0.8 if len(steps) < 3 else 0.3):
            op = None
            if st.traj_mode == "exact" and rng.random() < 0.5:      # (trajectory_sequences' menu leaves the exact mode and the
                op = "traj_first"                             # bounds rarely: HVP and GNVP are refused under them)
            elif st.bounds is not None and rng.random() < 0.35:
                op = "bounds_off"
        else:
            op = pick(checks + (["risk_weights"] * 6 if st.risk is not None else []))
        if op == "refused setting":                           # (a risk under a running cost or the reverse, if either stands)
            op = "rc_on" if st.risk is not None else "risk_on" if st.rc is not None else None
        if step is None:
            if op is None or op in SETTING_OPS:
                step = _draw_setting(rng, ctx, st, op)
            else:
                step = _draw_check(rng, ctx, op, again)
                if ctx["served"] and base(op) in ("vjp_multi", "jvp_multi", "hvp", "gnvp", "observe_mean", "vjp_mean", "jvp_mean") \
                        and st.step_refusal(step) is None and (rng.random() < (0.35 if op in DEVICE_NEW else 0.6) or op == "observe_mean"):
                    queue = _follow(rng, ctx, st, step)
        if step["op"] in CHECK_OPS:
            again = step
        st.apply(step)
        cleared = was_valid and st.valid is None
        steps.append(step)
    if ctx["served"]:
        for op in ("jvp_linear", "linear"):
            step = _draw_check(rng, ctx, op, None)
            st.apply(step)
            steps.append(step)
    return steps


def walk_seed(seed, contexts=CONTEXTS_PER_SEED):
    """exactly the (context, steps) pairs run_seed runs"""
    rng = np.random.default_rng(BASE_SEED + seed)
    out = []
    for _ in range(contexts):
        ctx = draw_context(rng)
        out.append((ctx, draw_steps(rng, ctx)))
    return out


def drawn_checks(steps):
    return sum(s["op"] in CHECK_OPS for s in steps)


# ---- the references -------------------------------------------------------------------------------------------------------
def weight_arrays(probe, wi, E, per_member_shape=False):
    """(w, wf, blocks) of a weight draw as GrapeEngine.observe_gnvp and gnvp_reference take them; per_member_shape: a block
    shared by the members repeated per member (the header: "shared weights return the bits of the same block repeated")"""
    wd = probe["weights"][wi]
    w = wd["w"]
    if w is not None and per_member_shape and not wd["member"]:
        w = np.broadcast_to(w[:, None], (3, E) + w.shape[1:]).copy() if wd["blocks"] else np.broadcast_to(w, (E,) + w.shape).copy()
    return w, wd["wf"], wd["blocks"]


def mean_cotangent(probe, c):
    """the cotangent of the AVERAGED values of pool entry c: its first member's block"""
    yb, xb = probe["cots"][c]
    return (None if yb is None else yb[0]), (None if xb is None else xb[0])


class FRefs(ts.Refs):
    """trajectory_sequences.Refs and the references of the new calls, each in physical slice space of explicit operators,
    pulse and physical direction"""

    def props(self, gen, ops, x):
        ctx = self.ctx
        x = np.ascontiguousarray(x, dtype=np.float64)
        return self.cached(("props", gen, x.tobytes()),
                           lambda: propagators(np.asarray(ops["A"], complex), np.asarray(ops["B"], complex), x, ctx["T"], ctx["variant"]))

    def hvp(self, gen, ops, x, xdot, p, c, t, swap=False, weights=None):
        """(term of Lamd, term of Xdot) of hvp_reference.hvp_ref; swap: the cotangent and its tangent exchanged, weights:
        per-member factors on both (mix-ups of the host test)"""
        ctx, probe = self.ctx, self.ctx["probes"][p]
        x, xdot = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(xdot, dtype=np.float64)
        (yb, xb), (ybd, xbd) = probe["cots"][c], probe["tans"][t]
        if swap:
            (yb, xb), (ybd, xbd) = (ybd, xbd), (yb, xb)
        if weights is not None:
            yb, xb, ybd, xbd = (None if a is None else a * np.asarray(weights)[:, None, None] for a in (yb, xb, ybd, xbd))
        return self.cached(("hvp", gen, p, c, t, swap, None if weights is None else np.asarray(weights).tobytes(), x.tobytes(), xdot.tobytes()),
                           lambda: hr.hvp_ref(ops["A"], ops["B"], ops["Xi"], x, xdot, ctx["T"], probe["O"], yb, xb, ybd, xbd,
                                              probe["per_member"], ctx["variant"], self.props(gen, ops, x)))

    def vjp_of_tangent(self, gen, ops, x, p, t):
        """vjp(ybar_dot, Xbar_dot): what grape_eval_hvp returns for xdot = 0"""
        ctx, probe = self.ctx, self.ctx["probes"][p]
        ybd, xbd = probe["tans"][t]
        return vr.vjp_ref(ops["A"], ops["B"], ops["Xi"], x, ctx["T"], probe["O"], ybd, xbd, probe["per_member"], ctx["variant"])

    def gnvp(self, gen, ops, x, xdot, p, wi, w=None, wf=None, blocks=None, tag=None):
        """Gn of gnvp_reference.gnvp_ref for weight draw wi; (w, wf, blocks, tag): other weights under a name (the mix-ups)"""
        ctx, probe = self.ctx, self.ctx["probes"][p]
        x, xdot = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(xdot, dtype=np.float64)
        if tag is None:
            w, wf, blocks = weight_arrays(probe, wi, ctx["E"])
        return self.cached(("gnvp", gen, p, wi, tag, x.tobytes(), xdot.tobytes()),
                           lambda: gr.gnvp_ref(ops["A"], ops["B"], ops["Xi"], x, xdot, ctx["T"], probe["O"] if w is not None else None,
                                               w, wf, probe["per_member"], ctx["variant"], self.props(gen, ops, x), blocks))

    def vjp_mean(self, gen, ops, x, p, c, v, mode):
        """G of the explicit cotangents v_k ybar_mean, v_k Xbar_mean (traj_mean_reference.vjp_mean_ref; in the exact mode
        through traj_exact_reference)"""
        ctx, probe = self.ctx, self.ctx["probes"][p]
        x = np.ascontiguousarray(x, dtype=np.float64)
        ybm, xbm = mean_cotangent(probe, c)

        def make():
            if mode == "exact":
                return xr.exact_vjp_ref(ops["A"], ops["B"], ops["Xi"], x, ctx["T"], probe["O"], tm.broadcast_cotangent(v, ybm),
                                        tm.broadcast_cotangent(v, xbm), probe["per_member"], ctx["variant"], self.slices(gen, ops, x))
            return tm.vjp_mean_ref(ops["A"], ops["B"], ops["Xi"], x, ctx["T"], probe["O"], v, ybm, xbm, probe["per_member"], ctx["variant"])
        return self.cached(("vjp mean", gen, p, c, mode, np.asarray(v).tobytes(), x.tobytes()), make)

    # -- of a state of the walk, in the coordinates the calls work in --
    def v_of(self, st, vi):
        v = st.ctx["vs"][vi]
        return np.asarray(st.ops["wts"], dtype=np.float64) if v is None else v

    def hvp_of(self, st, i, p, c, d, t, scale=1.0):
        """Gdot: no bounds stand where the call runs, so the pulse map is the basis alone -- projection only"""
        x, _ = st.physical(st.pulses()[i])
        tl, tx = self.hvp(st.gen, st.ops, x, st.expand_dir(scale * st.dirs()[d]), p, c, t)
        return st.project(tl + tx)

    def gnvp_of(self, st, i, p, d, wi):
        """Phi' s J' W J s Phi tdot: the slope on both sides"""
        x, s = st.physical(st.pulses()[i])
        return st.project(s * self.gnvp(st.gen, st.ops, x, s * st.expand_dir(st.dirs()[d]), p, wi))

    def observe_mean_of(self, st, i, p, vi):
        y, Xf = self.observe_of(st, i, p)
        v = self.v_of(st, vi)
        return (None if y is None else tm.member_sum(v, y)), tm.member_sum(v, Xf)

    def jvp_mean_of(self, st, i, p, d, vi):
        yd, Xd = self.jvp_of(st, i, p, d)
        v = self.v_of(st, vi)
        return (None if yd is None else tm.member_sum(v, yd)), tm.member_sum(v, Xd)

    def vjp_mean_of(self, st, i, p, c, vi):
        x, s = st.physical(st.pulses()[i])
        return st.project(self.vjp_mean(st.gen, st.ops, x, p, c, self.v_of(st, vi), st.traj_mode) * s)


def check_fsum(got, v, members, what):
    """the device's sum against math.fsum of v_k members[k], every component within traj_mean_reference.fsum_tolerance:
    E 2^-52 sum_k |v_k| |component_k| (twice the a-priori first-order bound of any summation order) -- test_gpu_traj_mean.py's
    check; `members` is the per-member result of the same step, itself held to the NumPy reference"""
    ref, mag = tm.fsum_mean(v, members)
    assert got.shape == ref.shape and tm.within(got, ref, tm.fsum_tolerance(len(v), mag)), f"{what}: outside the tolerance of the sum"


# ---- on the device --------------------------------------------------------------------------------------------------------
def run_context(qoc, oracle, ctx, steps, setenv, cid, log):
    """Creates the context and walks the steps; every check against the references, the memo and the identities.  setenv(name,
    value or None) sets the environment the way the caller wants it undone.  log(line) receives each step before it runs.
    Returns the number of checked operations (refused settings, which end in an evaluation, not counted)."""
    import torch
    setenv("GRAPE_SMALL_KERNEL", ctx["kernel"])
    setenv("GRAPE_MAX_WORKSPACE_BYTES", None if ctx["budget"] is None else str(ctx["budget"]))
    setenv("GRAPE_TRAJ_STAGED", ctx["staged"])
    n, m, K, N, E, T, mb = ctx["n"], ctx["m"], ctx["K"], ctx["N"], ctx["E"], ctx["T"], ctx["max_batch"]
    st, refs, memo, o, checks = FState(ctx), FRefs(oracle, ctx), {}, ctx["ops"], 0
    kw = dict(gradient="exact", objective=ctx["gexact"]) if ctx["gexact"] else {}
    held = {}                                                 # the last multi results, for the transpose identity
    sized = set()                                             # (call, settings) whose scratch has been sized already
    log("context: " + context_line(ctx))

    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def ptr(t):
        return 0 if t is None else t.data_ptr()

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def nan(*shape, dtype=torch.complex128):
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda")

    def host(t):
        return None if t is None else t.cpu().numpy()

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
            if ctx["long"]:                                   # one lane per time chunk, 64 chunks per wave of the lane kernel
                assert info["slices_per_lane"] == 1 and 64 * info["waves_per_member"] > MULTI_MAX_THREADS, info

        # ---- the device forms: every array stays referenced until the synchronise behind the call
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
            yb, xb = cot
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

        def vjp_multi_arrays(probe, cs):
            yb = None if probe["cots"][cs[0]][0] is None else np.array([probe["cots"][c][0] for c in cs])
            xb = None if probe["cots"][cs[0]][1] is None else np.array([probe["cots"][c][1] for c in cs])
            return yb, xb

        def vjp_multi_device(th, probe, cs):
            yb, xb = vjp_multi_arrays(probe, cs)
            try:
                G = eng.observe_vjp_multi_device(dev(th), dev(probe["O"]) if yb is not None else None, dev(yb), dev(xb),
                                                 per_member=probe["per_member"], stream=stream())
            finally:
                torch.cuda.synchronize()
            return G.cpu().numpy()

        def jvp_multi_device(th, tdots, probe):
            try:
                yd, Xd = eng.observe_jvp_multi_device(dev(th), dev(np.array(tdots)), dev(probe["O"]) if probe["n_obs"] else None,
                                                      per_member=probe["per_member"], final=True, stream=stream())
            finally:
                torch.cuda.synchronize()
            return host(yd), host(Xd)

        def hvp_device(th, tdot, probe, cot, tan, bad=False):
            (yb, xb), (ybd, xbd) = cot, tan
            n_obs = probe["n_obs"] if (yb is not None or ybd is not None) and not bad else 0
            t = [None if th is None else dev(th.T), dev(tdot.T), dev(_probes_cm(probe)) if n_obs else None, dev(yb),
                 None if xb is None else dev(_cm(xb)), dev(ybd), None if xbd is None else dev(_cm(xbd))]
            G = nan(eng._cols, K, dtype=torch.float64)
            try:
                eng.observe_hvp_device(ptr(t[0]), ptr(t[1]), n_obs, probe["per_member"], ptr(t[2]), ptr(t[3]), ptr(t[4]), ptr(t[5]),
                                       ptr(t[6]), ptr(G), stream())
            finally:
                torch.cuda.synchronize()
            return np.ascontiguousarray(G.cpu().numpy().T)

        def gnvp_device(th, tdot, probe, w, wf, blocks, wpm_bad=None):
            wpm, planes = eng._gnvp_weights("gnvp_device", w, probe["n_obs"], blocks) if w is not None else (0, None)
            n_obs = probe["n_obs"] if w is not None else 0
            t = [None if th is None else dev(th.T), dev(tdot.T), dev(_probes_cm(probe)) if n_obs else None, dev(planes), dev(wf)]
            G = nan(eng._cols, K, dtype=torch.float64)
            try:
                eng.observe_gnvp_device(ptr(t[0]), ptr(t[1]), n_obs, probe["per_member"], ptr(t[2]), wpm if wpm_bad is None else wpm_bad,
                                        ptr(t[3]), ptr(t[4]), ptr(G), stream())
            finally:
                torch.cuda.synchronize()
            return np.ascontiguousarray(G.cpu().numpy().T)

        def raw(name, *args):
            """an entry point with arguments the binding refuses itself; pointers as integers, None for NULL"""
            try:
                eng._check(getattr(eng._lib, name)(eng._h, *args))
            finally:
                torch.cuda.synchronize()

        def refused_family_form(form, arg, th, tdot, probe):
            """a call of one of the four new device forms with an argument the header lists as invalid; every array is sized for
            the count handed over, so that a library that wrongly accepted it would stay inside them"""
            what_arg, value, _ = BAD_ARGS[form][arg % len(BAD_ARGS[form])]
            xd, xb1 = dev(th.T), probe["cots"][-1][1]
            if form == "vjp_multi_device":
                xbs, G = dev(_cm(np.array([xb1] * (MAX_MULTI + 1)))), nan(MAX_MULTI + 1, eng._cols, K, dtype=torch.float64)
                raw("grape_eval_vjp_multi_device", ptr(xd), value, 0, 0, None, None, ptr(xbs), ptr(G), stream())
            elif form == "jvp_multi_device":
                xds, Xd = dev(np.array([tdot.T] * (MAX_MULTI + 1))), nan(MAX_MULTI + 1, E, m, n)
                raw("grape_eval_jvp_multi_device", ptr(xd), value, ptr(xds), 0, 0, None, None, ptr(Xd), stream())
            elif form == "hvp_device":                        # n_obs = 0 with a non-NULL ybar_dot (Xbar_final given)
                ybd = torch.zeros((E, 1, N + 1), dtype=torch.complex128, device="cuda")
                t, G = [dev(tdot.T), dev(_cm(xb1))], nan(eng._cols, K, dtype=torch.float64)
                try:
                    eng.observe_hvp_device(ptr(xd), ptr(t[0]), 0, probe["per_member"], 0, 0, ptr(t[1]), ptr(ybd), 0, ptr(G), stream())
                finally:
                    torch.cuda.synchronize()
            elif what_arg == "no weights":
                t, G = dev(tdot.T), nan(eng._cols, K, dtype=torch.float64)
                raw("grape_eval_gnvp_device", ptr(xd), ptr(t), 0, 0, None, 0, None, None, ptr(G), stream())
            else:
                gnvp_device(th, tdot, probe, None, probe["weights"][0]["wf"], None, wpm_bad=value)

        # ---- the checks
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

        def check_hvp(i, p, c, d, t, G, what):
            close(G, refs.hvp_of(st, i, p, c, d, t), what + " Gdot")
            _same(memo, st.traj_key("hvp", i, p, c, d, t), (G,), what)

        def check_gnvp(i, p, d, wi, G, what):                 # (the shared and the per-member shape of one block: one key)
            close(G, refs.gnvp_of(st, i, p, d, wi), what + " Gn")
            _same(memo, st.traj_key("gnvp", i, p, d, wi), (G,), what)

        def pairings(i, p, what):
            """the transpose identity between the multi results held for this pulse, probe set and state: for every (r, d)
            <cot_r, J xdot_d> = <J' cot_r, xdot_d> to 1e-12 of the sum of the absolute terms, the bar of the Gauss-Newton pair"""
            key = st.traj_key("pair", i, p)
            if ("jvp", key) not in held or ("vjp", key) not in held:
                return
            (ds, yd, Xd), (cs, G) = held[("jvp", key)], held[("vjp", key)]
            for r, c in enumerate(cs):
                yb, xb = ctx["probes"][p]["cots"][c]
                for k, d in enumerate(ds):
                    lhs, mag = jr.pairing(yb, None if yd is None else yd[k], xb, Xd[k])
                    rhs = float(np.sum(G[r] * st.dirs()[d]))
                    assert abs(lhs - rhs) <= 1e-12 * mag, f"{what}: set {c} x direction {d}: {lhs!r} against {rhs!r}, sum of |terms| {mag!r}"

        def names_after(op, step, names, what):
            """the kernels the header names for a host form"""
            exact, forced_long = st.traj_mode == "exact", ctx["long"]
            if op == "hvp":
                assert "trajectory_hvp_kernel" in names, (what, names)
            elif op == "gnvp":
                assert "trajectory_gnvp_kernel" in names, (what, names)
            elif op in ("observe_mean", "jvp_mean"):
                assert "traj_mean_reduce_kernel" in names and ("traj_mean_combine_kernel" in names) == (E > 16), (what, names)
            elif op == "vjp_mean":
                assert "traj_mean_broadcast_kernel" in names, (what, names)
            elif op == "jvp_multi":
                multi, single = ("trajectory_jvp_multi_exact_kernel", "trajectory_jvp_exact_kernel") if exact else \
                    ("trajectory_jvp_multi_kernel", "trajectory_jvp_kernel")
                if step["jm"] == "0" or forced_long:          # (more than 256 chunks: the single kernel per direction, whatever is forced)
                    assert single in names and multi not in names, (what, names)
                elif step["jm"] == "1":
                    assert multi in names and single not in names, (what, names)
                else:
                    assert multi in names or single in names, (what, names)
            elif op == "vjp_multi":
                single = ("trajectory_vjp_exact_kernel",) if exact else ("trajectory_vjp_kernel", "trajectory_vjp_staged_kernel")
                if step["vm"] == "1" and not exact and not forced_long:
                    assert "trajectory_vjp_multi_kernel" in names, (what, names)
                else:                                         # (no shape dispatches to the multi kernel by default)
                    assert any(k in names for k in single) and "trajectory_vjp_multi_kernel" not in names, (what, names)

        plan()
        ws = eng.info["workspace_bytes"]
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
                if refusal:                                   # the refused call has cleared the flag as every grape_set_* does: a
                    why = st.reuse_refusal()                  # reuse right behind it, before anything evaluates
                    pr = ctx["probes"][si % 3]
                    _expect(qoc, lambda: vjp_device(None, pr, pr["cots"][0]), why[0], why[1], what + " refused, then a reuse")
                    i = si % 3                                # ... and it left the evaluation what it was
                    F, G = eng.eval(st.pulses()[i])
                    check_fg(i, F, G, what + " refused, then eval")
                    st.clear("eval")
                now = eng.info["workspace_bytes"]
                # (the one release the library documents and test_gpu_workspace_accounting.py pins: on a gradient = exact
                # context with square states an upload of Hermitian generators hands the costate array back)
                released = op == "upload" and ctx["gexact"] and m == n and step["herm"]
                assert now >= ws or released, f"{what}: workspace_bytes fell from {ws} to {now}"
                ws = now
                continue
            checks += 1
            i, p, c, d, t, wi, vi = (step[k] for k in ("i", "p", "c", "d", "t", "w", "v"))
            cs, ds = step["cs"], step["ds"]
            probe = ctx["probes"][p]
            th = st.pulses()[i]
            cot, tan = probe["cots"][c], probe["tans"][t]
            yb, xb = cot
            O = probe["O"]
            b = base(op)
            setenv("GRAPE_JVP_MULTI", step["jm"])
            setenv("GRAPE_VJP_MULTI", step["vm"])
            refusal = st.step_refusal(step)
            if op in ALL_REUSE and refusal is None:
                i = st.valid[1]                               # the trajectory in the workspace is that pulse's
                what += f" along pulse {i} of {st.valid[0]}"
            reuse = op in ALL_REUSE
            x_in = None if reuse else th
            tdot = st.dirs()[d]
            call = None                                       # ops that are one call: refused as a whole, or checked by `done`
            if op == "eval":
                F, G = eng.eval(th)
                check_fg(i, F, G, what)
                names = eng.kernel_names()
                assert not [k for k in names if k in FAMILY_KERNELS], f"{what}: kernels of the trajectory family in a plain evaluation: {names}"
            elif op == "device":
                xd = dev(th.T)
                fg = torch.zeros(xd.numel() + 1, dtype=torch.float64, device="cuda")
                eng.eval_device(xd.data_ptr(), fg.data_ptr(), stream())
                torch.cuda.synchronize()
                h = fg.cpu().numpy()
                check_fg(i, h[-1], h[:-1].reshape(th.shape[1], K).T, what)
            elif op == "batch":
                idx = [(i + k) % 3 for k in range(mb)]
                Fs, Gs = eng.eval_batch(np.array([st.pulses()[j] for j in idx]))
                for k, j in enumerate(idx):
                    check_fg(j, Fs[k], Gs[k], f"{what} entry {k}")
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

                def done(res):
                    y, Xf, F = res
                    check_observe(i, p, y, Xf, what)
                    F_ref, G_ref, _ = refs.fg(st, i)
                    assert_parity(F, G_ref, F_ref, G_ref, n, what=what + " F")
                    key = st.fg_key(i)
                    assert key not in memo or memo[key][0][0] == F, f"{what}: F is not grape_eval's bit for bit"
            elif op == "observe_device":
                def call():
                    return observe_device(th, probe)

                def done(res):
                    y, Xf, fg = res
                    check_observe(i, p, y, Xf, what)
                    check_fg(i, fg[-1], fg[:-1].reshape(th.shape[1], K).T, what + " fg")
            elif op == "vjp":
                def call():
                    return eng.observe_vjp(th, O if yb is not None else None, ybar=yb, xbar_final=xb, per_member=probe["per_member"])

                def done(G):
                    check_vjp(i, p, c, G, what)
            elif op in ("vjp_device", "vjp_reuse"):
                def call():
                    return vjp_device(x_in, probe, cot)

                def done(G):
                    check_vjp(i, p, c, G, what)
            elif op in ("jvp", "jvp_linear"):
                def call(sign=1.0):
                    return eng.observe_jvp(th, sign * tdot, O, per_member=probe["per_member"], final=True)

                def done(res):
                    yd, Xd = res
                    check_jvp(i, p, d, yd, Xd, what)
                    if op == "jvp_linear":                    # every operation is linear in xdot: -xdot returns the negated bits
                        ym, Xm = call(-1.0)
                        assert (yd is None or np.array_equal(ym, -yd)) and np.array_equal(Xm, -Xd), f"{what}: -xdot"
            elif op in ("jvp_device", "jvp_reuse"):
                def call():
                    return jvp_device(x_in, tdot, probe)

                def done(res):
                    check_jvp(i, p, d, res[0], res[1], what)
            elif op == "gn_pair":                             # J v, then J' w, along one stored trajectory
                if refusal:
                    _expect(qoc, lambda: jvp_device(None, tdot, probe), refusal[0], refusal[1], what + " J v")
                    _expect(qoc, lambda: vjp_device(None, probe, cot), refusal[0], refusal[1], what + " J' w")
                else:
                    yd, Xd = jvp_device(None, tdot, probe)
                    check_jvp(i, p, d, yd, Xd, what + " J v")
                    G = vjp_device(None, probe, cot)
                    check_vjp(i, p, c, G, what + " J' w")
                    lhs, mag = jr.pairing(yb, yd, xb, Xd)
                    rhs = float(np.sum(G * tdot))
                    assert abs(lhs - rhs) <= 1e-12 * mag, f"{what}: <cot, J v> = {lhs!r}, <J' cot, v> = {rhs!r}, sum of |terms| {mag!r}"
            elif op == "device_refused":                      # invalid arguments: INVALID_ARG behind the context's own refusals
                form = step["form"]                           # (and the call's own); a failed device form clears the flag
                if form in ts.DEVICE_FORMS:                   # n_obs = 0 with a non-null y / ybar / ydot
                    status, word = st.traj_refusal(form) or (INVALID_ARG, "n_obs = 0")
                    bad = {"observe_device": lambda: observe_device(th, probe, bad=True),
                           "vjp_device": lambda: vjp_device(th, probe, (None, probe["cots"][-1][1]), bad=True),
                           "jvp_device": lambda: jvp_device(th, tdot, probe, bad=True)}[form]
                else:
                    status, word = st.family_refusal(form) or (INVALID_ARG, BAD_ARGS[form][step["arg"] % len(BAD_ARGS[form])][2])

                    def bad():
                        return refused_family_form(form, step["arg"], th, tdot, probe)
                _expect(qoc, bad, status, word, f"{what} {form}")
            # ---- the family
            elif b == "vjp_multi":
                ybs, xbs = vjp_multi_arrays(probe, cs)
                if op == "vjp_multi":
                    def call():
                        return eng.observe_vjp_multi(th, O if ybs is not None else None, ybars=ybs, xbars_final=xbs, per_member=probe["per_member"])
                else:
                    def call():
                        return vjp_multi_device(x_in, probe, cs)

                def done(G):
                    assert G.shape == (len(cs), K, th.shape[1]), (what, G.shape)
                    for r, cr in enumerate(cs):               # block r is the single call of set r: parity, and the single call's key
                        check_vjp(i, p, cr, np.ascontiguousarray(G[r]), f"{what} block {r} (set {cr})")
                    held[("vjp", st.traj_key("pair", i, p))] = (cs, G)
                    pairings(i, p, what)
            elif b == "jvp_multi":
                tdots = [st.dirs()[k] for k in ds]
                if op == "jvp_multi":
                    def call():
                        return eng.observe_jvp_multi(th, np.array(tdots), O, per_member=probe["per_member"], final=True)
                else:
                    def call():
                        return jvp_multi_device(x_in, tdots, probe)

                def done(res):
                    yd, Xd = res
                    assert Xd.shape == (len(ds), E, n, m), (what, Xd.shape)
                    for k, dk in enumerate(ds):
                        check_jvp(i, p, dk, None if yd is None else np.ascontiguousarray(yd[k]), np.ascontiguousarray(Xd[k]),
                                  f"{what} block {k} (direction {dk})")
                    held[("jvp", st.traj_key("pair", i, p))] = (ds, yd, Xd)
                    pairings(i, p, what)
            elif b == "hvp":
                if op == "hvp":
                    def call():
                        return eng.observe_hvp(th, tdot, O if (yb is not None or tan[0] is not None) else None, ybar=yb, xbar_final=xb,
                                               ybar_dot=tan[0], xbar_final_dot=tan[1], per_member=probe["per_member"])
                else:
                    def call():
                        return hvp_device(x_in, tdot, probe, cot, tan)

                def done(G):
                    check_hvp(i, p, c, d, t, G, what)
            elif b == "gnvp":
                w, wf, blocks = weight_arrays(probe, wi, E, bool(step["wm"]))
                if op == "gnvp":
                    def call():
                        return eng.observe_gnvp(th, tdot, O if w is not None else None, w=w, wf=wf, per_member=probe["per_member"], blocks=blocks)
                else:
                    def call():
                        return gnvp_device(x_in, tdot, probe, w, wf, blocks)

                def done(G):
                    check_gnvp(i, p, d, wi, G, what)
            elif op == "observe_mean":
                v, col = ctx["vs"][vi], step["col"]
                Oc = O if col is None else (O[:, col:col + 1] if probe["per_member"] else O[col:col + 1])

                def call():
                    return eng.observe_mean(th, Oc, v=v, per_member=probe["per_member"], final=True, want_F=True)

                def done(res):
                    ym, Xm, F = res
                    ym_ref, Xm_ref = refs.observe_mean_of(st, i, p, vi)
                    key = st.traj_key("observe_mean", i, p, vi)
                    if col is not None:                       # column col of the 16-probe call, bit for bit
                        assert ym.shape == (1, N + 1), (what, ym.shape)
                        close(ym, ym_ref[col:col + 1], what + " y_mean")
                        if key in memo and memo[key][0][0] is not None:
                            assert np.array_equal(ym[0], memo[key][0][0][col]), f"{what}: not column {col} of {memo[key][1]}"
                        _same(memo, key, (None, Xm), what)
                    else:
                        if ym_ref is not None:
                            close(ym, ym_ref, what + " y_mean")
                        _same(memo, key, (ym, Xm), what)
                    close(Xm, Xm_ref, what + " X_mean")
                    F_ref, G_ref, _ = refs.fg(st, i)
                    assert_parity(F, G_ref, F_ref, G_ref, n, what=what + " F")
                    fkey = st.fg_key(i)                        # the F of the read-out is grape_eval's: the [F, G] key's F
                    assert fkey not in memo or memo[fkey][0][0] == F, f"{what}: F is not grape_eval's bit for bit"
                    # the same step's per-member read-out: the sums against its fsum
                    y, Xf, _ = eng.observe(th, O, per_member=probe["per_member"], final=True, want_F=True)
                    check_observe(i, p, y, Xf, what + ", then observe")
                    vv = refs.v_of(st, vi)
                    if y is not None:
                        check_fsum(ym, vv, y if col is None else y[:, col:col + 1], what + " y_mean")
                    check_fsum(Xm, vv, Xf, what + " X_mean")
            elif op == "jvp_mean":
                v = ctx["vs"][vi]

                def call():
                    return eng.observe_jvp_mean(th, tdot, O, v=v, per_member=probe["per_member"], final=True)

                def done(res):
                    ym, Xm = res
                    ym_ref, Xm_ref = refs.jvp_mean_of(st, i, p, d, vi)
                    if ym_ref is not None:
                        close(ym, ym_ref, what + " ydot_mean")
                    close(Xm, Xm_ref, what + " Xdot_mean")
                    _same(memo, st.traj_key("jvp_mean", i, p, vi, d), (ym, Xm), what)
                    yd, Xd = eng.observe_jvp(th, tdot, O, per_member=probe["per_member"], final=True)
                    check_jvp(i, p, d, yd, Xd, what + ", then jvp")
                    vv = refs.v_of(st, vi)
                    if yd is not None:
                        check_fsum(ym, vv, yd, what + " ydot_mean")
                    check_fsum(Xm, vv, Xd, what + " Xdot_mean")
            elif op == "vjp_mean":
                v = ctx["vs"][vi]
                ybm, xbm = mean_cotangent(probe, c)

                def call():
                    return eng.observe_vjp_mean(th, O if ybm is not None else None, ybar_mean=ybm, xbar_mean=xbm, v=v, per_member=probe["per_member"])

                def done(G):
                    close(G, refs.vjp_mean_of(st, i, p, c, vi), what + " G")
                    _same(memo, st.traj_key("vjp_mean", i, p, vi, c), (G,), what)
                    vv = refs.v_of(st, vi)                    # bit for bit the plain pull-back of the explicit cotangents
                    Ge = eng.observe_vjp(th, O if ybm is not None else None, ybar=tm.broadcast_cotangent(vv, ybm),
                                         xbar_final=tm.broadcast_cotangent(vv, xbm), per_member=probe["per_member"])
                    assert np.array_equal(G, Ge), f"{what}: not grape_eval_vjp of v_k ybar_mean, v_k Xbar_mean bit for bit"
            elif op == "newton_cg":                           # jvp_reuse, then hvp_reuse, along one stored trajectory
                for part, sub in (("jvp", dict(step, op="jvp_reuse")), ("hvp", dict(step, op="hvp_reuse"))):
                    why = st.reuse_refusal_of(part)
                    one = (lambda: jvp_device(None, tdot, probe)) if part == "jvp" else (lambda: hvp_device(None, tdot, probe, cot, tan))
                    if why:
                        _expect(qoc, one, why[0], why[1], f"{what} {part}")
                    elif part == "jvp":
                        yd, Xd = one()
                        check_jvp(st.valid[1], p, d, yd, Xd, what + " J v")
                    else:
                        check_hvp(st.valid[1], p, c, d, t, one(), what + " H v")
                    st.apply(sub)
            elif op == "gn_cg":                               # gnvp_reuse for two directions; then J v -> W in NumPy -> J' w
                w, wf, blocks = weight_arrays(probe, wi, E, bool(step["wm"]))
                if refusal:
                    _expect(qoc, lambda: gnvp_device(None, tdot, probe, w, wf, blocks), refusal[0], refusal[1], what)
                else:
                    d2 = (d + 1 + t) % POOL
                    u = st.dirs()[d2]
                    Gv = gnvp_device(None, tdot, probe, w, wf, blocks)
                    check_gnvp(i, p, d, wi, Gv, what + " GN v")
                    Gu = gnvp_device(None, u, probe, w, wf, blocks)
                    check_gnvp(i, p, d2, wi, Gu, what + " GN u")
                    # <u, GN v> = <v, GN u> at PARITY_RTOL of the magnitude, as test_gpu_gnvp.py::test_symmetric_and_positive
                    uv, vu, mag = float(np.sum(u * Gv)), float(np.sum(tdot * Gu)), float(np.sum(np.abs(u) * np.abs(Gv)))
                    assert abs(uv - vu) <= PARITY_RTOL * mag, f"{what}: <u, GN v> = {uv!r}, <v, GN u> = {vu!r}, magnitude {mag!r}"
                    yd, Xd = jvp_device(None, tdot, probe)
                    check_jvp(i, p, d, yd, Xd, what + " J v")
                    ybw = gr.apply_weights(w, yd, blocks) if w is not None else None
                    xbw = None if wf is None else wf[:, None, None] * Xd
                    Gc = vjp_device(None, probe, (ybw, xbw))  # the fused result against the composed one, at the parity bar
                    close(Gv, Gc, what + ": fused against J' W J v composed")
            elif op == "linear":                              # the exact scaling identities of the header, as bits
                why_h, why_g = st.family_refusal("hvp"), st.family_refusal("gnvp")
                w, wf, blocks = weight_arrays(probe, wi, E)

                def hvp(s):
                    return eng.observe_hvp(th, s * tdot, O if (yb is not None or tan[0] is not None) else None, ybar=yb, xbar_final=xb,
                                           ybar_dot=None if tan[0] is None else s * tan[0],
                                           xbar_final_dot=None if tan[1] is None else s * tan[1], per_member=probe["per_member"])

                def gnvp(s):
                    return eng.observe_gnvp(th, s * tdot, O if w is not None else None, w=w, wf=wf, per_member=probe["per_member"], blocks=blocks)
                if why_h:
                    _expect(qoc, lambda: hvp(1.0), why_h[0], why_h[1], what + " hvp")
                else:
                    G1 = hvp(1.0)
                    check_hvp(i, p, c, d, t, G1, what + " hvp")
                    assert np.array_equal(hvp(2.0), 2.0 * G1) and np.array_equal(hvp(-1.0), -G1), f"{what}: hvp of the scaled triple"
                    # xdot = 0: grape_eval_vjp(ybar_dot, Xbar_final_dot), at the parity bar
                    G0 = eng.observe_hvp(th, 0.0 * tdot, O if (yb is not None or tan[0] is not None) else None, ybar=yb, xbar_final=xb,
                                         ybar_dot=tan[0], xbar_final_dot=tan[1], per_member=probe["per_member"])
                    Gt = eng.observe_vjp(th, O if tan[0] is not None else None, ybar=tan[0], xbar_final=tan[1], per_member=probe["per_member"])
                    close(G0, Gt, what + ": hvp with xdot = 0 against vjp of the tangent")
                if why_g:
                    _expect(qoc, lambda: gnvp(1.0), why_g[0], why_g[1], what + " gnvp")
                else:
                    G1 = gnvp(1.0)
                    check_gnvp(i, p, d, wi, G1, what + " gnvp")
                    assert np.array_equal(gnvp(2.0), 2.0 * G1) and np.array_equal(gnvp(-1.0), -G1), f"{what}: gnvp of the scaled direction"
                    assert not gnvp(0.0).any(), f"{what}: gnvp of xdot = 0"
            else:
                raise AssertionError(f"unknown step {op}")
            if call is not None:
                if refusal:
                    _expect(qoc, call, refusal[0], refusal[1], what)
                else:
                    res = call()
                    if op in HOST_NEW:
                        names_after(op, step, eng.kernel_names(), what)
                    elif ctx["long"] and b in ("vjp_multi", "jvp_multi"):
                        names = eng.kernel_names()                # the fallback to the single kernels per set / direction
                        assert "trajectory_vjp_multi_kernel" not in names and "trajectory_jvp_multi_kernel" not in names, (what, names)
                    done(res)
            if op != "newton_cg":
                st.apply(step)
            # workspace_bytes never falls, and a call whose kind, shapes and settings have occurred before sizes nothing anew
            now = eng.info["workspace_bytes"]
            assert now >= ws, f"{what}: workspace_bytes fell from {ws} to {now}"
            sig = (op, p, c % 3 if probe["n_obs"] else 0, t, wi, step["wm"], len(cs), len(ds), step["jm"], step["vm"], step["col"],
                   step.get("form"), step.get("arg"), refusal, st.settings_key())
            if sig in sized:
                assert now == ws, f"{what}: workspace_bytes grew from {ws} to {now} on a call that has run before under these settings"
            sized.add(sig)
            ws = now
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
    """the model's word on a check step: True when every call of it runs (for device_refused: when the argument check is what
    refuses it), False when the context, a setting, the flag or the member chunk refuses it"""
    return st.step_refusal(step) is None


def _pairs(st, prev, mid, step, ctx):
    """the rows of the adjacent-pair table that (prev, [mid,] step) is an instance of; st: the state in front of `step`"""
    out = []
    if prev is None or step["op"] not in CHECK_OPS:
        return out
    a, b_ = base(prev["op"]), base(step["op"])
    same = prev["p"] == step["p"]
    probe = ctx["probes"][step["p"]]
    if mid is not None:                                       # X, an upload that flips the flow, the same op again
        if mid["op"] == "upload" and a in ("hvp", "gnvp") and prev["op"] == step["op"] and mid.get("flipped"):
            out.append(f"{a}* > flip > {a}*")
        return out
    if a == "vjp_multi" and b_ == "vjp" and same:
        out.append("vjp_multi* > vjp*")
    if a == "jvp_multi" and b_ == "jvp" and same:
        out.append("jvp_multi* > jvp*")
    if a == "hvp" and b_ == "vjp" and same:
        out.append("hvp* > vjp*")
        if ctx["staged"] == "1" and probe["n_obs"] in (9, 16) and has_ybar(probe, step["c"]) and step["op"] != "vjp":
            out.append(f"hvp* > staged vjp* with {probe['n_obs']} probes")
    if a == "gnvp" and b_ == "vjp" and same and has_ybar(probe, step["c"]):
        out.append("gnvp* > vjp* with a ybar")
    if a == "gnvp" and b_ == "hvp":
        out.append("gnvp* > hvp*")
    if a == "hvp" and b_ == "gnvp":
        out.append("hvp* > gnvp*")
    if a in ("observe_mean", "vjp_mean", "jvp_mean") and step["op"] in ("observe", "vjp", "jvp"):
        out.append("*_mean > observe / vjp / jvp")
    if a == b_ == "observe_mean" and same and probe["n_obs"] == 16:
        if prev["col"] is None and step["col"] is not None:
            out.append("observe_mean 16 > 1")
        if prev["col"] is not None and step["col"] is None:
            out.append("observe_mean 1 > 16")
    if a == "vjp_multi" and len(prev["cs"]) >= 2 and step["op"] in ("eval", "device", "batch") and st.rc is not None:
        out.append(f"vjp_multi* (n_set >= 2) > eval / device / batch under a running cost ({st.rc_mode})")
    if a == "jvp_multi" and st.traj_mode == "exact" and st.images(prev) > 1:
        if b_ == "vjp":
            out.append("jvp_multi* (several images, exact) > exact vjp*")
        if step["op"] == "eval" and st.rc is not None and st.rc_mode == "exact":
            out.append("jvp_multi* (several images, exact) > eval under an exact running cost")
    return out


def coverage(seeds=SEEDS, contexts=CONTEXTS_PER_SEED):
    """Counter over the walks of `seeds`: ("op", op, condition) for the checks that RUN and ("refused", op, condition) for
    those that are refused (the refusal is then the assertion), ("accepted", reuse op, device form behind it), ("refused reuse",
    class of the invalidator), ("refusal", op, word), ("pair", row of the table), ("multi", "vjp" | "jvp", count, forced value),
    ("E=33", "mean" | "multi"), ("flag set", refused device form), "contexts", "long contexts", "checks", "checks that run",
    "refused settings"."""
    cnt = Counter()
    for seed in seeds:
        for ctx, steps in walk_seed(seed, contexts):
            st = FState(ctx)
            cnt["contexts"] += 1
            cnt["long contexts"] += ctx["long"]
            prev = mid = None                                 # the last check that ran, and a setting behind it
            for step in steps:
                op = step["op"]
                if op in SETTING_OPS:
                    why = st.setting_refusal(op)
                    if why:
                        cnt["refused settings"] += 1
                    if op == "upload":
                        step = dict(step, flipped=ctx["full"] and step["herm"] != st.ops["herm"])
                    mid = step if mid is None and not why else False
                    st.apply(step)
                    if why:
                        st.clear("eval")
                    continue
                ok = runs(st, step)
                cnt["checks"] += 1
                cnt["checks that run"] += ok
                for cond in ["any"] + st.conditions():
                    cnt[("op" if ok else "refused", op, cond)] += 1
                why = st.step_refusal(step)
                if ok and mid is not False:
                    for row in _pairs(st, prev, mid, step, ctx):
                        cnt[("pair", row)] += 1
                if op in ALL_REUSE:
                    if why is None:
                        cnt[("accepted", op, st.valid[0])] += 1
                    elif why[0] == NOT_READY:
                        cnt[("refused reuse", "chunked context" if ctx["chunked"] else st.cleared_by)] += 1
                    else:
                        cnt[("refusal", op, why[1])] += 1
                elif why is not None:
                    cnt[("refusal", step["form"] if op == "device_refused" else op, why[1])] += 1
                    if op in DEVICE_NEW and st.valid is not None:
                        cnt[("flag set", op, why[1])] += 1
                elif op == "device_refused" and step["form"] in DEVICE_NEW:
                    cnt[("refusal", step["form"], BAD_ARGS[step["form"]][step["arg"] % len(BAD_ARGS[step["form"]])][2])] += 1
                    if st.valid is not None:
                        cnt[("flag set", step["form"], "arguments")] += 1
                if ok and base(op) == "vjp_multi":
                    cnt[("multi", "vjp", len(step["cs"]), step["vm"])] += 1
                if ok and base(op) == "jvp_multi":
                    cnt[("multi", "jvp", len(step["ds"]), step["jm"])] += 1
                if ok and ctx["E"] == 33 and base(op) in ("observe_mean", "vjp_mean", "jvp_mean"):
                    cnt[("E=33", "mean")] += 1
                if ok and ctx["E"] == 33 and base(op) in ("vjp_multi", "jvp_multi"):
                    cnt[("E=33", "multi")] += 1
                prev, mid = (step, None) if ok else (None, None)
                st.apply(step)
    return cnt
