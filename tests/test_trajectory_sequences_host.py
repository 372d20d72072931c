"""The trajectory soak's generator and references (tests/trajectory_sequences.py) on the CPU: the committed seeds of
test_gpu_trajectory_soak.py walk what the module claims (the coverage floors below are conditions, met by the seed count), the
flag model agrees with the header's sentence case by case, no likely mix-up can hide under the parity bar, and the references
form a transpose pair on the walk's own inputs.  Needs neither a GPU nor the library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jvp_reference as jr  # noqa: E402
import settings_sequences as ss  # noqa: E402
import trajectory_sequences as ts  # noqa: E402

CONDITIONS = ("basis", "bounds", "penalties", "running cost", "exact running cost", "risk", "exact trajectory mode", "chunked")
WALKED = [op for op in ts.NEW_CHECK_OPS if op != "jvp_linear"]       # (jvp_linear: once per context, behind the walk)
# refused by design, so they never run: a running cost and a risk exclude each other (the header refuses either under the
# other), and a member-chunked context answers every reuse with GRAPE_ERR_NOT_READY ("member_chunk")
IMPOSSIBLE = {("risk_weights", "running cost"), ("risk_weights", "exact running cost"), ("vjp_reuse", "chunked"),
              ("jvp_reuse", "chunked"), ("gn_pair", "chunked")}
INVALIDATORS = ("setting change", "eval", "batch", "fom", "host form", "controls", "upload", "refused device call", "chunked context")
REFUSALS = [("rc_on", "risk"), ("risk_on", "running cost"), ("traj_exact", "StateTransfer"), ("rc_exact", "StateTransfer"),
            ("rc_on", "StateTransfer"), ("rc_on", "exact"), ("rc_first", "exact"), ("traj_exact", "exact")]
HIDE_MARGIN = 1e-6


def table(cnt, kind="op"):
    """kind "op": the checks that run (held to references, memo and identities); "refused": those whose refusal is the assertion"""
    conds = ("any",) + CONDITIONS
    lines = [f"{'op':16s}" + "".join(f"{c[:10]:>11s}" for c in conds)]
    for op in ts.CHECK_OPS:
        lines.append(f"{op:16s}" + "".join(f"{cnt[(kind, op, c)]:11d}" for c in conds))
    return "\n".join(lines)


def test_the_committed_seeds_meet_the_coverage_floors():
    cnt = ts.coverage()
    print(f"{len(ts.SEEDS)} seeds, {cnt['contexts']} contexts, {cnt['checks']} checks: {cnt['checks that run']} run, "
          f"{cnt['checks'] - cnt['checks that run']} assert a refusal; {cnt['refused settings']} refused settings (each followed by "
          "a refused reuse and an evaluation)")
    print("checks that run (device_refused: refused for its arguments, on a context that serves the form):")
    print(table(cnt))
    print("checks refused by the context, the flag or the member chunk:")
    print(table(cnt, "refused"))
    for k in sorted((k for k in cnt if isinstance(k, tuple) and k[0] not in ("op", "refused")), key=str):
        print(k, cnt[k])
    short = {}
    for op in WALKED:                                         # every new check op RUNS at least twice under every setting
        for cond in CONDITIONS:
            if (op, cond) not in IMPOSSIBLE and cnt[("op", op, cond)] < 2:
                short[(op, cond)] = cnt[("op", op, cond)]
    for op in ts.REUSE_OPS:                                   # each reuse kind accepted three times behind each device form
        for form in ts.DEVICE_FORMS:
            if cnt[("accepted", op, form)] < 3:
                short[("accepted", op, form)] = cnt[("accepted", op, form)]
        if cnt[("exact pair under an exact running cost", op)] < 2:       # the buffer both exact modes share
            short[("exact pair under an exact running cost", op)] = cnt[("exact pair under an exact running cost", op)]
    for by in INVALIDATORS:                                   # a refused reuse behind every class of invalidator
        if cnt[("refused reuse", by)] < 1:
            short[("refused reuse", by)] = 0
    for op, word in REFUSALS:                                 # every documented refusal
        if cnt[("refusal", op, word)] < 1:
            short[("refusal", op, word)] = 0
    for n_obs in (8, 9, 16):                                  # the staged / direct switch under both forced choices
        for staged in ("0", "1"):
            if cnt[("staged", n_obs, staged)] < 1:
                short[("staged", n_obs, staged)] = 0
    if cnt[("E=33 vjp",)] < 1:
        short["E=33 vjp"] = 0
    if cnt[("refused setting, flag set",)] < 1:               # (the reuse behind it pins that a refused grape_set_* clears the flag)
        short["refused setting, flag set"] = 0
    assert not short, short


def test_the_generator_is_a_pure_function_of_the_seed():
    a, b = ts.walk_seed(3), ts.walk_seed(3)
    assert [ts.context_line(c) for c, _ in a] == [ts.context_line(c) for c, _ in b]
    assert [[ts.step_line(s) for s in st] for _, st in a] == [[ts.step_line(s) for s in st] for _, st in b]
    assert np.array_equal(a[0][0]["pool"], b[0][0]["pool"]) and np.array_equal(a[-1][0]["ops"]["A"], b[-1][0]["ops"]["A"])
    assert np.array_equal(a[1][0]["xdots"], b[1][0]["xdots"])
    for (ca, _), (cb, _) in zip(a, b):
        for pa, pb in zip(ca["probes"], cb["probes"]):
            assert pa["n_obs"] == pb["n_obs"] and all(np.array_equal(u[1], v[1]) for u, v in zip(pa["cots"], pb["cots"]))


def test_no_step_is_dropped_and_the_contexts_are_the_issues():
    for seed in ts.SEEDS:
        for ctx, steps in ts.walk_seed(seed):
            assert all(s["op"] in ts.SETTING_OPS + ts.CHECK_OPS for s in steps)
            assert ts.drawn_checks(steps) == sum(s["op"] not in ts.SETTING_OPS for s in steps) >= 1
            assert steps[-1]["op"] in ts.CHECK_OPS and (steps[-1]["op"] == "jvp_linear") == ctx["served"]
            assert ctx["n"] in (2, 3, 4) and ctx["K"] in (1, 2, 3, 5) and ctx["N"] in (1, 3, 8, 20, 65, 130)
            assert ctx["E"] in (1, 2, 3, 7, 33) and (ctx["E"] != 33 or ctx["N"] <= 20)
            assert all(p["n_obs"] in ts.PROBE_COUNTS for p in ctx["probes"])
            assert not ctx["chunked"] or (ctx["E"] == 7 and ctx["budget"] and ctx["served"])


# ---- the flag model against the header's sentence --------------------------------------------------------------------------
# "set at the end of a successful call of either device form with a non-NULL d_x on a context that is not member-chunked [the
# push-forward's device form likewise]; cleared by every other entry point that evaluates or changes a setting (grape_eval*,
# grape_eval_fom, the host forms, grape_get_controls, every grape_set_*) and by any failed call of the device forms"; "a reuse
# call keeps the flag set".  (context kind, steps, flag set afterwards, what a reuse answers: None = it runs)
FLAG_TABLE = [
    ("served", [], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device"], True, None),
    ("served", ["vjp_device"], True, None),
    ("served", ["jvp_device"], True, None),
    ("served", ["observe_device", "vjp_reuse", "jvp_reuse", "gn_pair"], True, None),
    ("served", ["vjp_device", "eval"], False, (ts.NOT_READY, "reuse")),
    ("served", ["vjp_device", "device"], False, (ts.NOT_READY, "reuse")),
    ("served", ["vjp_device", "batch"], False, (ts.NOT_READY, "reuse")),
    ("served", ["jvp_device", "fom"], False, (ts.NOT_READY, "reuse")),
    ("served", ["jvp_device", "controls"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "observe"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "vjp"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "jvp"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "device_refused"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "risk_weights"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "pen_on"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "traj_exact"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "rc_exact"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "risk_on"], False, (ts.NOT_READY, "reuse")),
    ("served", ["observe_device", "upload"], False, (ts.NOT_READY, "reuse")),
    ("served", ["risk_on", "observe_device", "rc_on"], False, (ts.NOT_READY, "reuse")),      # a refused setting clears it too
    ("served", ["vjp_device", "eval", "vjp_reuse", "jvp_device"], True, None),
    ("chunked", ["observe_device"], False, (ts.NOT_READY, "member_chunk")),
    ("chunked", ["vjp_device", "jvp_device"], False, (ts.NOT_READY, "member_chunk")),
    ("sandwich", ["observe_device"], True, (ts.UNSUPPORTED, "StateTransfer")),
    ("sandwich", ["vjp_device"], False, (ts.UNSUPPORTED, "StateTransfer")),
    ("exact", ["observe_device"], False, (ts.UNSUPPORTED, "exact")),
]


def _context_of_kind(kind):
    for seed in ts.SEEDS:
        for ctx, _ in ts.walk_seed(seed):
            this = ("chunked" if ctx["chunked"] else "served") if ctx["served"] else ("exact" if ctx["gexact"] else "sandwich")
            if this == kind:
                return ctx
    raise AssertionError(kind)


@pytest.mark.parametrize("row", range(len(FLAG_TABLE)))
def test_the_flag_model_follows_the_headers_sentence(row):
    kind, ops, valid, answer = FLAG_TABLE[row]
    ctx = _context_of_kind(kind)
    st, rng = ts.TState(ctx), np.random.default_rng(row)
    for op in ops:
        if op in ts.SETTING_OPS:
            step = dict(op=op, beta=4.0, ops=ctx["ops"], amp=np.ones(ctx["K"]), var=None)
            if op == "rc_on":
                step.update(ss._draw_rc(rng, ctx, ctx["ops"]["Xt"], 1))
        else:
            step = dict(op=op, i=1, p=0, c=0, d=0, form="vjp_device")
        st.apply(step)
    assert (st.valid is not None) == valid and st.reuse_refusal() == answer
    if valid and ops[0] in ts.DEVICE_FORMS and kind == "served":
        assert st.valid[1] == 1                               # the trajectory is that of the pulse the device form took


# ---- no mix-up can hide ------------------------------------------------------------------------------------------------------
def _differs(wrong, right):
    """some output array of the mixed-up answer is further than the margin from the right one"""
    for a, b in zip(wrong, right):
        if a is not None and b is not None and np.abs(a - b).max() > HIDE_MARGIN * np.abs(b).max():
            return True
    return False


def _raw(st, th):
    """the pulse a library that forgot the map (the bounds; without them the offset of the basis) would evaluate, or None"""
    a, _ = st.expand(th)
    if st.bounds is not None:
        return a
    if st.basis is not None and st.basis["x0"] is not None:
        return a - st.basis["x0"]
    return None


def mixups(refs, st, step):
    """[(name, differs, excusable)] of one accepted trajectory check, or of an evaluation under a running cost"""
    op, ctx = step["op"], st.ctx
    i, p, c, d = step["i"], step["p"], step["c"], step["d"]
    if op in ts.REUSE_OPS:
        i = st.valid[1]
    th, stale = st.pulses()[i], st.pulses()[(i + 2) % 3]
    x, s = st.physical(th)
    raw, prev = _raw(st, th), st.prev_ops
    other = "exact" if st.traj_mode == "first_order" else "first_order"
    zero_rows = p == 2 and c == 0 and ctx["probes"][p]["n_obs"] > 0
    out = []
    if op in ("observe", "observe_device"):
        right = refs.observe(st.gen, st.ops, x, p)
        if raw is not None:
            out.append(("raw coordinates", _differs(refs.observe(st.gen, st.ops, raw, p), right), False))
        out.append(("stale pulse", _differs(refs.observe(st.gen, st.ops, st.physical(stale)[0], p), right), False))
        if prev is not None:
            out.append(("previous operators", _differs(refs.observe(st.gen - 1, prev, x, p), right), False))
    if op in ("vjp", "vjp_device", "vjp_reuse", "gn_pair"):
        def back(G):
            return (st.project(G * s),)
        Gp = refs.vjp(st.gen, st.ops, x, p, st.traj_mode)[c]
        right = back(Gp)
        assert np.abs(right[0]).max() > 0
        out.append(("other mode", _differs(back(refs.vjp(st.gen, st.ops, x, p, other)[c]), right), ctx["N"] == 1))
        if raw is not None:
            out.append(("raw coordinates", _differs(back(refs.vjp(st.gen, st.ops, raw, p, st.traj_mode)[c]), right), zero_rows))
        xs, ss_ = st.physical(stale)
        out.append(("stale pulse", _differs((st.project(refs.vjp(st.gen, st.ops, xs, p, st.traj_mode)[c] * ss_),), right), zero_rows))
        if prev is not None:
            out.append(("previous operators", _differs(back(refs.vjp(st.gen - 1, prev, x, p, st.traj_mode)[c]), right), zero_rows))
        if ctx["E"] > 1:
            out.append(("weights folded in", _differs(back(refs.vjp(st.gen, st.ops, x, p, st.traj_mode, st.ops["wts"])[c]), right), zero_rows))
        pen = ss.penalty_ref(x, st.pen["amp"], st.pen["var"])[1] if st.pen is not None else None
        if pen is not None:                                   # (N = 1 under a variation penalty alone: its gradient is 0)
            out.append(("penalties folded in", _differs(back(Gp + pen), right), ctx["N"] == 1 and not np.abs(pen).any()))
        if st.rc is not None:
            GJ = (refs.composed(st.gen, st.ops, x, st.rc, st.rc_gen)[5] if st.rc_mode == "first_order" else
                  refs.rc_exact(st.gen, st.ops, x, st.rc, st.rc_gen)[1])
            out.append(("running cost folded in", _differs(back(Gp + GJ), right), False))
        if st.risk is not None and ctx["E"] > 1:
            pk = refs.fg(st, i)[2]
            out.append(("risk folded in", _differs(back(refs.vjp(st.gen, st.ops, x, p, st.traj_mode, pk)[c]), right), zero_rows))
        if st.bounds is not None:
            out.append(("slope left out", _differs((st.project(Gp),), right), False))
    if op in ("jvp", "jvp_device", "jvp_reuse", "gn_pair", "jvp_linear"):
        xd = st.expand_dir(st.dirs()[d])
        right = refs.jvp(st.gen, st.ops, x, s * xd, p, st.traj_mode)
        out.append(("other mode (push-forward)", _differs(refs.jvp(st.gen, st.ops, x, s * xd, p, other), right), ctx["N"] == 1))
        if raw is not None:
            out.append(("raw coordinates (push-forward)", _differs(refs.jvp(st.gen, st.ops, raw, s * xd, p, st.traj_mode), right), False))
        xs, ss_ = st.physical(stale)
        out.append(("stale pulse (push-forward)", _differs(refs.jvp(st.gen, st.ops, xs, ss_ * xd, p, st.traj_mode), right), False))
        if prev is not None:
            out.append(("previous operators (push-forward)", _differs(refs.jvp(st.gen - 1, prev, x, s * xd, p, st.traj_mode), right), False))
        if st.bounds is not None:
            out.append(("slope left out (push-forward)", _differs(refs.jvp(st.gen, st.ops, x, xd, p, st.traj_mode), right), False))
    if op in ("eval", "device") and st.rc is not None:
        G = refs.fg(st, i)[1]
        mode, st.rc_mode = st.rc_mode, "exact" if st.rc_mode == "first_order" else "first_order"
        out.append(("other running-cost mode", _differs((refs.fg(st, i)[1],), (G,)), ctx["N"] == 1))
        st.rc_mode = mode
    return out


@pytest.mark.parametrize("seed", ts.SEEDS)
def test_no_mix_up_can_hide_under_the_parity_bar(oracle, seed):
    """every accepted trajectory check of the seed: the answer under each likely mix-up -- the other derivative mode, raw
    instead of physical coordinates, the previous pulse of the pool, the previous operators, weights / penalties / running
    cost / risk folded into a pull-back, the slope left out -- is further than 1e-6 of the reference's scale from the
    reference.  Excepted by name, listed, and at most 10 % of the checks: N = 1 (one slice: the two rules may coincide
    closely, and a variation penalty alone has a zero gradient, so that "penalties folded in" changes nothing) and the
    cotangent draw with whole zero rows."""
    hidden, excepted, looked = [], [], 0
    for ci, (ctx, steps) in enumerate(ts.walk_seed(seed)):
        st, refs = ts.TState(ctx), ts.Refs(oracle, ctx)
        for si, step in enumerate(steps):
            op = step["op"]
            if op in ts.CHECK_OPS and ts.runs(st, step) and op not in ("device_refused", "risk_weights"):
                found = mixups(refs, st, step)
                looked += bool(found)
                for name, differs, excusable in found:
                    if not differs:
                        where = f"seed {seed} context {ci} ({ts.context_line(ctx)}) step {si} {ts.step_line(step)}: {name}"
                        (excepted if excusable else hidden).append(where)
            st.apply(step)
            if st.refusal:
                st.clear("eval")
    print(f"seed {seed}: {looked} checks looked at, {len(excepted)} excepted")
    print("\n".join(excepted))
    assert not hidden, hidden
    assert len(excepted) <= 0.1 * looked, (len(excepted), looked)


# ---- the references are a transpose pair on the walk's inputs ----------------------------------------------------------------
def test_the_references_form_a_transpose_pair_on_the_walks_inputs(oracle):
    """exact_vjp_ref / exact_jvp_ref (and the first-order pair) on the pulses, probes, cotangents and directions of the first
    six seeds: <(ybar, Xbar), J xdot> = <J' (ybar, Xbar), xdot> to 1e-12 of the sum of the absolute terms"""
    done = 0
    for seed in list(ts.SEEDS)[:6]:
        for ctx, _ in ts.walk_seed(seed):
            if not ctx["served"] or ctx["N"] > 65:
                continue
            refs, o = ts.Refs(oracle, ctx), ctx["ops"]
            for mode in ("exact", "first_order"):
                for p, probe in enumerate(ctx["probes"]):
                    G = refs.vjp(0, o, ctx["pool"][0], p, mode)
                    ydot, Xdot = refs.jvp(0, o, ctx["pool"][0], ctx["xdots"][1], p, mode)
                    for c, (yb, xb) in enumerate(probe["cots"]):
                        lhs, mag = jr.pairing(yb, ydot, xb, Xdot)
                        rhs = float(np.sum(G[c] * ctx["xdots"][1]))
                        assert abs(lhs - rhs) <= 1e-12 * mag, (ts.context_line(ctx), mode, p, c, lhs, rhs, mag)
                        done += 1
    print(f"{done} pairings")
    assert done >= 60
