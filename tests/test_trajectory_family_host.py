"""The family walk's generator and references (tests/trajectory_family_sequences.py) on the CPU: the older walk draws what it
drew before this module existed (a digest of its 40 seeds), the committed seeds of test_gpu_trajectory_family_soak.py walk what
the module claims (the coverage floors below are conditions, met by the seed count), the flag model agrees with the header's
sentences on the new forms case by case, no likely mix-up can hide under the parity bar, and the references are consistent with
each other on the walk's own inputs.  Needs neither a GPU nor the library."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gnvp_reference as gr  # noqa: E402
import hvp_reference as hr  # noqa: E402
import settings_sequences as ss  # noqa: E402
import traj_mean_reference as tm  # noqa: E402
import trajectory_family_sequences as tf  # noqa: E402
import trajectory_sequences as ts  # noqa: E402
import vjp_reference as vr  # noqa: E402
from test_trajectory_sequences_host import HIDE_MARGIN, _differs, _raw  # noqa: E402

# SHA-256 over context_line and every step_line of trajectory_sequences.walk_seed(s), s in trajectory_sequences.SEEDS, computed
# at the commit in front of the family walk: the older walk stays byte-identical
PARENT_DIGEST = "274c4ba1bda8c6a8188469930e6c108cac333efb407c29051af5287a1fe3a6e1"
CONDITIONS = ("basis", "bounds", "penalties", "running cost", "exact running cost", "risk", "exact trajectory mode", "chunked")
WALKED = tf.HOST_NEW + tf.DEVICE_NEW + tf.REUSE_NEW + tf.LOOPS + ("device_refused",)     # (linear: once per context, behind the walk)
INVALIDATORS = ("setting change", "eval", "batch", "fom", "host form", "family host form", "controls", "upload", "refused device call",
                "chunked context")
PAIRS = ("vjp_multi* > vjp*", "jvp_multi* > jvp*", "hvp* > vjp*", "gnvp* > vjp* with a ybar", "gnvp* > hvp*", "hvp* > gnvp*",
         "*_mean > observe / vjp / jvp", "observe_mean 16 > 1", "observe_mean 1 > 16",
         "vjp_multi* (n_set >= 2) > eval / device / batch under a running cost (first_order)",
         "vjp_multi* (n_set >= 2) > eval / device / batch under a running cost (exact)",
         "jvp_multi* (several images, exact) > exact vjp*", "jvp_multi* (several images, exact) > eval under an exact running cost",
         "hvp* > flip > hvp*", "gnvp* > flip > gnvp*")
# the refusals the header documents for the new calls: (op, word)
REFUSALS = [(op, word) for op in ("hvp", "hvp_device", "hvp_reuse") for word in ("bounds", "trajectory_derivative", "StateTransfer", "exact")] \
    + [(op, word) for op in ("gnvp", "gnvp_device", "gnvp_reuse") for word in ("trajectory_derivative", "StateTransfer", "exact")] \
    + [(op, word) for op in ("vjp_multi", "vjp_multi_device", "jvp_multi", "jvp_multi_device", "vjp_mean", "jvp_mean")
       for word in ("StateTransfer", "exact")] + [("observe_mean", "exact"), ("observe_mean", "c1")] \
    + [(form, bad[2]) for form in tf.DEVICE_NEW for bad in tf.BAD_ARGS[form]]
# the refused device forms that find the flag set
FLAG_SET = [(form, "arguments") for form in tf.DEVICE_NEW] + [("hvp_device", "bounds"), ("hvp_device", "trajectory_derivative"),
                                                             ("gnvp_device", "trajectory_derivative")]


def impossible(op, cond):
    """refused by design, so they never run: grape_eval_hvp under bounds and in the exact mode, grape_eval_gnvp in the exact
    mode (the loops with them), and every reuse on a member-chunked context (GRAPE_ERR_NOT_READY, "member_chunk")"""
    b = tf.base(op)
    return (b in ("hvp", "newton_cg") and cond in ("bounds", "exact trajectory mode")) or \
        (b in ("gnvp", "gn_cg") and cond == "exact trajectory mode") or (op in tf.ALL_REUSE and cond == "chunked")


def table(cnt, kind="op"):
    conds = ("any",) + CONDITIONS
    lines = [f"{'op':18s}" + "".join(f"{c[:10]:>11s}" for c in conds)]
    for op in tf.CHECK_OPS:
        lines.append(f"{op:18s}" + "".join(f"{cnt[(kind, op, c)]:11d}" for c in conds))
    return "\n".join(lines)


def test_the_older_walk_draws_what_it_drew_before():
    h = hashlib.sha256()
    for seed in ts.SEEDS:
        for ctx, steps in ts.walk_seed(seed):
            h.update((ts.context_line(ctx) + "\n").encode())
            for step in steps:
                h.update((ts.step_line(step) + "\n").encode())
    assert len(ts.SEEDS) == 40 and h.hexdigest() == PARENT_DIGEST


def test_the_committed_seeds_meet_the_coverage_floors():
    cnt = tf.coverage()
    print(f"{len(tf.SEEDS)} seeds, {cnt['contexts']} contexts ({cnt['long contexts']} with more than 256 time chunks), {cnt['checks']} "
          f"checks: {cnt['checks that run']} run, {cnt['checks'] - cnt['checks that run']} assert a refusal; {cnt['refused settings']} "
          "refused settings (each followed by a refused reuse and an evaluation)")
    print("checks that run (device_refused: refused for its arguments, on a context that serves the form):")
    print(table(cnt))
    print("checks refused by the context, a setting, the flag or the member chunk:")
    print(table(cnt, "refused"))
    print("accepted reuse kinds (rows) behind the device forms (columns: " + ", ".join(tf.DEVICE_FORMS) + "):")
    for op in tf.ALL_REUSE:
        print(f"{op:18s}" + "".join(f"{cnt[('accepted', op, form)]:6d}" for form in tf.DEVICE_FORMS))
    for k in sorted((k for k in cnt if isinstance(k, tuple) and k[0] not in ("op", "refused", "accepted")), key=str):
        print(k, cnt[k])
    short = {}
    for op in WALKED:                                         # every new check op RUNS at least twice under every setting
        for cond in CONDITIONS:
            if not impossible(op, cond) and cnt[("op", op, cond)] < 2:
                short[(op, cond)] = cnt[("op", op, cond)]
    for op in tf.REUSE_OPS:                                   # each of the seven reuse kinds three times behind each device form
        for form in tf.DEVICE_FORMS:
            if cnt[("accepted", op, form)] < 3:
                short[("accepted", op, form)] = cnt[("accepted", op, form)]
    for row in PAIRS:                                         # each adjacent pair of the table twice
        if cnt[("pair", row)] < 2:
            short[("pair", row)] = cnt[("pair", row)]
    for n_obs in (9, 16):                                     # ... the staged probe counts under GRAPE_TRAJ_STAGED=1 included
        if cnt[("pair", f"hvp* > staged vjp* with {n_obs} probes")] < 1:
            short[("staged", n_obs)] = 0
    for by in INVALIDATORS:                                   # a refused reuse behind every class of invalidator
        if cnt[("refused reuse", by)] < 1:
            short[("refused reuse", by)] = 0
    for op, word in REFUSALS:                                 # every documented refusal of the new calls
        if cnt[("refusal", op, word)] < 1:
            short[("refusal", op, word)] = 0
    for form, word in FLAG_SET:                               # ... the refused device forms that find the flag set included
        if cnt[("flag set", form, word)] < 1:
            short[("flag set", form, word)] = 0
    for which in ("vjp", "jvp"):                              # the multi counts under each forced GRAPE_*_MULTI value
        for count in tf.MULTI_COUNTS:
            for forced in tf.ENV:
                if cnt[("multi", which, count, forced)] < 1:
                    short[("multi", which, count, forced)] = 0
    for which in ("mean", "multi"):
        if cnt[("E=33", which)] < 1:
            short[("E=33", which)] = 0
    if cnt["long contexts"] < 2:
        short["long contexts"] = cnt["long contexts"]
    assert not short, short


def test_the_generator_is_a_pure_function_of_the_seed():
    a, b = tf.walk_seed(3), tf.walk_seed(3)
    assert [tf.context_line(c) for c, _ in a] == [tf.context_line(c) for c, _ in b]
    assert [[tf.step_line(s) for s in st] for _, st in a] == [[tf.step_line(s) for s in st] for _, st in b]
    assert np.array_equal(a[1][0]["xdots"], b[1][0]["xdots"]) and np.array_equal(a[-1][0]["ops"]["A"], b[-1][0]["ops"]["A"])
    for (ca, _), (cb, _) in zip(a, b):
        assert all(np.array_equal(u, v) if u is not None else v is None for u, v in zip(ca["vs"], cb["vs"]))
        for pa, pb in zip(ca["probes"], cb["probes"]):
            assert pa["n_obs"] == pb["n_obs"] and all(np.array_equal(u[1], v[1]) for u, v in zip(pa["cots"], pb["cots"]) if u[1] is not None)
            assert all(np.array_equal(u["wf"], v["wf"]) for u, v in zip(pa["weights"], pb["weights"]))


def test_no_step_is_dropped_and_the_contexts_are_the_issues():
    longs = 0
    for seed in tf.SEEDS:
        for ctx, steps in tf.walk_seed(seed):
            assert all(s["op"] in tf.SETTING_OPS + tf.CHECK_OPS for s in steps)
            assert tf.drawn_checks(steps) == sum(s["op"] not in tf.SETTING_OPS for s in steps) >= 1
            assert (steps[-1]["op"] == "linear" and steps[-2]["op"] == "jvp_linear") == ctx["served"]
            assert ctx["n"] in (2, 3, 4) and ctx["K"] in (1, 2, 3, 5) and ctx["E"] in (1, 2, 3, 7, 33) and (ctx["E"] != 33 or ctx["N"] <= 20)
            assert ctx["xdots"].shape == (tf.POOL, ctx["K"], ctx["N"]) and len(ctx["vs"]) == 2 and ctx["vs"][0] is None
            assert ctx["E"] == 1 and ctx["vs"][1].tolist() == [1.0] or (ctx["vs"][1] == 0.0).sum() == 1
            if ctx["long"]:                                   # more than 256 time chunks: the smallest shape that reaches them
                longs += 1
                assert ctx["N"] == tf.LONG_N == tf.MULTI_MAX_THREADS + 1 and ctx["S"] == 1 and ctx["kernel"] == "lane" and ctx["n"] in (2, 3)
                assert ctx["E"] <= 2 and ctx["K"] <= 2 and all(p["n_obs"] <= 3 for p in ctx["probes"]) and ctx["served"]
            else:
                assert ctx["N"] in (1, 3, 8, 20, 65, 130) and all(p["n_obs"] in ts.PROBE_COUNTS for p in ctx["probes"])
            for p in ctx["probes"]:
                assert len(p["cots"]) == (3 * tf.POOL if p["n_obs"] else tf.POOL) and len(p["tans"]) == 2
                names = [w["name"] for w in p["weights"]]
                assert names == (["psd", "indefinite", "scalar", "final", "psd per member"] if p["n_obs"] else ["final", "final mixed"])
                if p["n_obs"]:
                    assert np.abs(p["weights"][1]["w"][1]).min() > 0          # the indefinite blocks: a non-zero ri plane
                    assert (p["weights"][1]["wf"] < 0).any() and (ctx["E"] == 1 or (p["weights"][1]["wf"] == 0).any())
            for s in steps:
                if s["op"] in tf.CHECK_OPS:
                    probe = ctx["probes"][s["p"]]
                    assert len(s["cs"]) in tf.MULTI_COUNTS and len(s["ds"]) in tf.MULTI_COUNTS and s["jm"] in tf.ENV and s["vm"] in tf.ENV
                    assert len(set(c % 3 for c in s["cs"])) == 1 or not probe["n_obs"]      # one form per multi call
                    if tf.base(s["op"]) in ("vjp_multi", "jvp_multi"):
                        assert s["c"] in s["cs"] and s["d"] in s["ds"] and set(s["cs"]) <= set(tf.same_form(probe, s["c"]))
    assert longs >= 2


# ---- the flag model against the header's sentences on the new forms ----------------------------------------------------------
# (context kind, steps, flag set afterwards, what each reuse kind answers: None = it runs).  The answers are listed for the
# forms vjp, jvp, vjp_multi, jvp_multi, hvp, gnvp in this order; one entry: the same for all six.
R, M = (ts.NOT_READY, "reuse"), (ts.NOT_READY, "member_chunk")
B, D = (ts.UNSUPPORTED, "bounds"), (ts.UNSUPPORTED, "trajectory_derivative")
S, X = (ts.UNSUPPORTED, "StateTransfer"), (ts.UNSUPPORTED, "exact")
FORMS = ("vjp", "jvp", "vjp_multi", "jvp_multi", "hvp", "gnvp")
FLAG_TABLE = [
    # "the "trajectory valid" flag is set under the same conditions [as grape_eval_vjp_device]" (vjp_multi_device); "The
    # "trajectory valid" flag is set under grape_eval_jvp_device's conditions" (jvp_multi_device); "With a non-NULL d_x on a
    # context that is not member-chunked the call sets the "trajectory valid" flag" (hvp_device, gnvp_device)
    ("served", ["vjp_multi_device"], True, [None]),
    ("served", ["jvp_multi_device"], True, [None]),
    ("served", ["hvp_device"], True, [None]),
    ("served", ["gnvp_device"], True, [None]),
    # "d_x = NULL ... keeps the flag set" (all four); "so the other reuse calls may follow"
    ("served", ["hvp_device", "vjp_multi_reuse", "jvp_multi_reuse", "hvp_reuse", "gnvp_reuse", "newton_cg", "gn_cg", "gn_pair"], True, [None]),
    ("served", ["observe_device", "gnvp_reuse", "hvp_reuse"], True, [None]),
    # "cleared by every other entry point that evaluates ... (..., the host forms, ...)": the seven new host forms
    ("served", ["gnvp_device", "vjp_multi"], False, [R]),
    ("served", ["gnvp_device", "jvp_multi"], False, [R]),
    ("served", ["vjp_multi_device", "hvp"], False, [R]),
    ("served", ["vjp_multi_device", "gnvp"], False, [R]),
    ("served", ["hvp_device", "observe_mean"], False, [R]),
    ("served", ["hvp_device", "vjp_mean"], False, [R]),
    ("served", ["jvp_multi_device", "jvp_mean"], False, [R]),
    ("served", ["jvp_multi_device", "linear"], False, [R]),
    # "and by any failed call of the device forms": invalid arguments, a refusal of the call's own, a refused reuse
    ("served", ["hvp_device", "device_refused"], False, [R]),
    ("served", ["gnvp_device", "eval", "gnvp_reuse", "hvp_reuse"], False, [R]),
    # grape_eval_hvp: "Two refusals of this call alone follow them [the context's], GRAPE_ERR_UNSUPPORTED: grape_set_bounds in
    # force ("bounds" ...) and grape_set_trajectory_derivative(GRAPE_TRAJ_EXACT) in force ("trajectory_derivative" ...)", in
    # front of the argument checks and of the NOT_READY of a reuse; as a failed device-form call it clears the flag
    ("served", ["bounds_on"], False, [R, R, R, R, B, R]),
    ("served", ["bounds_on", "vjp_device"], True, [None, None, None, None, B, None]),
    ("served", ["bounds_on", "vjp_device", "hvp_device"], False, [R, R, R, R, B, R]),
    ("served", ["bounds_on", "gnvp_device", "hvp_reuse"], False, [R, R, R, R, B, R]),
    ("served", ["bounds_on", "traj_exact"], False, [R, R, R, R, B, D]),                      # "bounds" in front of the mode
    ("served", ["traj_exact", "jvp_multi_device"], True, [None, None, None, None, D, D]),
    # grape_eval_gnvp: "One refusal of this call alone follows them ... ("trajectory_derivative" ...)"
    ("served", ["traj_exact", "vjp_multi_device", "gnvp_device"], False, [R, R, R, R, D, D]),
    ("served", ["traj_exact", "vjp_multi_device", "gn_cg"], False, [R, R, R, R, D, D]),
    ("served", ["traj_exact", "vjp_multi_device", "newton_cg"], False, [R, R, R, R, D, D]),  # (J v runs, then H v fails)
    ("served", ["traj_exact", "vjp_multi_device", "traj_first"], False, [R]),
    # "with the flag clear, or on a member-chunked context, GRAPE_ERR_NOT_READY with grape_eval_vjp_device's messages"
    ("chunked", ["hvp_device"], False, [M]),
    ("chunked", ["vjp_multi_device", "gnvp_device"], False, [M]),
    ("chunked", ["bounds_on", "hvp_device"], False, [M, M, M, M, B, M]),
    # "Served: the contexts grape_eval_vjp serves, refused with its reasons first"
    ("sandwich", ["hvp_device"], False, [S]),
    ("sandwich", ["observe_device", "gnvp_device"], False, [S]),
    ("sandwich", ["observe_device", "observe_mean"], False, [S]),         # (served like the read-out, and a host form)
    ("exact", ["vjp_multi_device"], False, [X]),
    ("exact", ["gnvp_device"], False, [X]),
]


def _context_of_kind(kind):
    for seed in tf.SEEDS:
        for ctx, _ in tf.walk_seed(seed):
            this = ("chunked" if ctx["chunked"] else "served") if ctx["served"] else ("exact" if ctx["gexact"] else "sandwich")
            if this == kind and not ctx["long"]:
                return ctx
    raise AssertionError(kind)


@pytest.mark.parametrize("row", range(len(FLAG_TABLE)))
def test_the_flag_model_follows_the_headers_sentences(row):
    kind, ops, valid, answers = FLAG_TABLE[row]
    ctx = _context_of_kind(kind)
    st, rng = tf.FState(ctx), np.random.default_rng(row)
    for op in ops:
        if op in tf.SETTING_OPS:
            step = dict(op=op, beta=4.0, ops=ctx["ops"], amp=np.ones(ctx["K"]), var=None, lo=-np.ones(ctx["K"]), hi=np.ones(ctx["K"]))
            if op == "rc_on":
                step.update(ss._draw_rc(rng, ctx, ctx["ops"]["Xt"], 1))
        else:
            step = dict(op=op, i=1, p=0, c=0, d=0, t=0, w=0, v=0, form="hvp_device", arg=0)
        st.apply(step)
    assert (st.valid is not None) == valid
    assert [st.reuse_refusal_of(form) for form in FORMS] == (answers * 6 if len(answers) == 1 else answers)
    if valid and kind == "served":
        assert st.valid[1] == 1                               # the trajectory is that of the pulse the device form took


# ---- no mix-up can hide ------------------------------------------------------------------------------------------------------
def fastest(blocks):
    """a block array (R, ...) as a reader would see it that takes the block index for the FASTEST one of the library's
    set-slowest (direction-slowest) memory"""
    R_ = blocks.shape[0]
    return np.ascontiguousarray(blocks.reshape(-1).reshape(-1, R_).T).reshape(blocks.shape)


def worlds(st, i):
    """{name: (gen, ops, x, slope going in, slope coming out)} of pulse i: the right one and the mix-ups of where a call may
    take its trajectory from"""
    th = st.pulses()[i]
    x, s = st.physical(th)
    out = {"right": (st.gen, st.ops, x, s, s)}
    xs, ss_ = st.physical(st.pulses()[(i + 2) % 3])
    out["stale pulse"] = (st.gen, st.ops, xs, ss_, ss_)
    if st.prev_ops is not None:
        out["previous operators"] = (st.gen - 1, st.prev_ops, x, s, s)
    raw = _raw(st, th)
    if raw is not None:
        out["raw coordinates"] = (st.gen, st.ops, raw, s, s)
    if st.bounds is not None:
        out["slope left out"] = (st.gen, st.ops, x, np.ones_like(s), np.ones_like(s))
        out["slope applied once"] = (st.gen, st.ops, x, np.ones_like(s), s)
    return out


def mixups(refs, st, step):
    """[(name, differs, excusable)] of one family check that runs, from the references alone"""
    op, ctx = step["op"], st.ctx
    i, p, c, d, t, wi, vi = (step[k] for k in ("i", "p", "c", "d", "t", "w", "v"))
    if op in tf.ALL_REUSE:
        i = st.valid[1]
    b, probe, E = tf.base(op), ctx["probes"][p], ctx["E"]
    mode, wts = st.traj_mode, np.asarray(st.ops["wts"], float)
    W = worlds(st, i)
    out = []

    def zero_rows(cc):                                        # (the cotangent draw with whole zero rows)
        return p == 2 and probe["n_obs"] > 0 and cc in (0, 1)

    def add(name, wrong, right, excusable=False):
        out.append((name, _differs(wrong, right), excusable))

    def pull(world, cc, weights=None):
        gen, ops, x, _, so = world
        return st.project(refs.vjp(gen, ops, x, p, mode, weights)[cc] * so)

    def push(world, dd):
        gen, ops, x, si, _ = world
        return refs.jvp(gen, ops, x, si * st.expand_dir(st.dirs()[dd]), p, mode)

    def other_c(cc):
        pool = tf.same_form(probe, cc)
        return pool[(pool.index(cc) + 1) % len(pool)]

    if b == "vjp_multi":
        cs = step["cs"]
        right = (np.array([pull(W["right"], cc) for cc in cs]),)
        assert np.abs(right[0]).max() > 0
        zr = any(zero_rows(cc) for cc in cs)
        for name, world in W.items():
            if name not in ("right", "slope applied once"):
                add(name, (np.array([pull(world, cc) for cc in cs]),), right, zr)
        add("the other pool cotangent", (np.array([pull(W["right"], other_c(cc)) for cc in cs]),), right)
        if len(set(cs)) > 1:
            add("blocks permuted", (np.roll(right[0], 1, axis=0),), right)
            if right[0][0].size > 1:                          # (K = 1 with one column: a block is one number, the layouts coincide)
                add("set-fastest layout", (fastest(right[0]),), right)
        if E > 1:
            add("ensemble weights folded in", (np.array([pull(W["right"], cc, wts) for cc in cs]),), right, zr)
    elif b == "jvp_multi":
        ds = step["ds"]

        def blocks(world, dds):
            res = [push(world, dd) for dd in dds]
            return (None if res[0][0] is None else np.array([r[0] for r in res])), np.array([r[1] for r in res])
        right = blocks(W["right"], ds)
        for name, world in W.items():
            if name not in ("right", "slope applied once"):
                add(name + " (push-forward)", blocks(world, ds), right)
        add("the other pool direction", blocks(W["right"], [(dd + 1) % tf.POOL for dd in ds]), right)
        if len(set(ds)) > 1:
            add("blocks permuted (push-forward)", tuple(None if a is None else np.roll(a, 1, axis=0) for a in right), right)
            add("direction-fastest layout", tuple(None if a is None else fastest(a) for a in right), right)
    elif b in ("hvp", "newton_cg"):
        def hvp(world, cc=c, dd=d, **kw):
            gen, ops, x, _, _ = world
            tl, tx = refs.hvp(gen, ops, x, st.expand_dir(st.dirs()[dd]), p, cc, t, **kw)
            return tl, tx
        tl, tx = hvp(W["right"])
        right = (st.project(tl + tx),)
        assert np.abs(right[0]).max() > 0
        zr = zero_rows(c)
        for name, world in W.items():
            if name in ("stale pulse", "previous operators", "raw coordinates"):
                add(name + " (HVP)", (st.project(sum(hvp(world))),), right, zr)
        x = W["right"][2]
        Gt = refs.vjp_of_tangent(st.gen, st.ops, x, p, t)
        add("the Lam' B' Xdot term dropped", (st.project(tl),), right, ctx["N"] == 1)
        if ctx["N"] > 1:                                      # (Lamd_s = P_s' (Lamd_{s+1} + V_s' Lam_{s+1}) + ... runs over s = N-1 .. 1:
            add("the V' Lam term dropped", (st.project(Gt + tx),), right)         # with one slice the term does not exist)
        add("xdot taken for zero", (st.project(Gt),), right)
        add("cotangent and its tangent swapped", (st.project(sum(hvp(W["right"], swap=True))),), right)
        add("the other pool direction (HVP)", (st.project(sum(hvp(W["right"], dd=(d + 1) % tf.POOL))),), right)
        add("the other pool cotangent (HVP)", (st.project(sum(hvp(W["right"], cc=other_c(c)))),), right)
        if E > 1:
            add("ensemble weights folded in (HVP)", (st.project(sum(hvp(W["right"], weights=wts))),), right)
    elif b in ("gnvp", "gn_cg"):
        w, wf, blocks_ = tf.weight_arrays(probe, wi, E)
        wd = probe["weights"][wi]

        def gn(world, dd=d, **kw):
            gen, ops, x, si, so = world
            return (st.project(so * refs.gnvp(gen, ops, x, si * st.expand_dir(st.dirs()[dd]), p, wi, **kw)),)
        right = gn(W["right"])
        assert np.abs(right[0]).max() > 0
        for name, world in W.items():                         # (N = 1: the pulse enters through X_1 X_1' alone, which unitary
            if name != "right":                               # propagation of square unitary initial states makes the identity)
                add(name + " (GNVP)", gn(world), right, ctx["N"] == 1 and name in ("stale pulse", "raw coordinates"))
        add("the other pool direction (GNVP)", gn(W["right"], dd=(d + 1) % tf.POOL), right)
        if w is not None and blocks_:
            add("rr and ii swapped", gn(W["right"], w=w[::-1].copy(), wf=wf, blocks=True, tag="swapped"), right)
            add("ri dropped", gn(W["right"], w=np.stack([w[0], np.zeros_like(w[1]), w[2]]), wf=wf, blocks=True, tag="no ri"), right)
        if w is not None and wf is not None:
            add("wf dropped", gn(W["right"], w=w, wf=None, blocks=blocks_, tag="no wf"), right, E > 1 and not wf[2:].any() and wf[0] == 0)
        if wd["member"] and E > 1:
            w0 = np.ascontiguousarray(w[:, 0])
            add("member 0's weights read for all", gn(W["right"], w=w0, wf=wf, blocks=True, tag="member 0"), right)
        if E > 1:
            wm = None if w is None else tf.weight_arrays(probe, wi, E, True)[0] * (wts[:, None, None] if not blocks_ else wts[None, :, None, None])
            wm = None if wm is None else (wm if wd["member"] or True else wm)
            add("ensemble weights folded in (GNVP)", gn(W["right"], w=wm, wf=None if wf is None else wf * wts, blocks=blocks_, tag="wts"), right)
    elif b in ("observe_mean", "jvp_mean"):
        v = refs.v_of(st, vi)

        def members(world):
            gen, ops, x, _, _ = world
            return refs.observe(gen, ops, x, p) if b == "observe_mean" else push(world, d)

        def mean(world, vv):
            y, Xf = members(world)
            return (None if y is None else tm.member_sum(vv, y)), tm.member_sum(vv, Xf)
        right = mean(W["right"], v)
        for name, world in W.items():
            if name in ("stale pulse", "previous operators", "raw coordinates") or (b == "jvp_mean" and name == "slope left out"):
                add(name + " (mean)", mean(world, v), right)
        if b == "jvp_mean":
            gen, ops, x, si, _ = W["right"]
            yd, Xd = refs.jvp(gen, ops, x, si * st.expand_dir(st.dirs()[(d + 1) % tf.POOL]), p, mode)
            add("the other pool direction (mean)", ((None if yd is None else tm.member_sum(v, yd)), tm.member_sum(v, Xd)), right)
        if E > 1:
            other = ctx["vs"][1] if ctx["vs"][vi] is None else wts
            add("the other weights in place of v", mean(W["right"], other), right)
            add("uniform v", mean(W["right"], np.ones(E)), right)
            if st.risk is not None:
                add("risk weights in place of v", mean(W["right"], refs.fg(st, i)[2]), right)
    elif b == "vjp_mean":
        v = refs.v_of(st, vi)

        def mean_pull(world, vv, cc=c):
            gen, ops, x, _, so = world
            return (st.project(refs.vjp_mean(gen, ops, x, p, cc, vv, mode) * so),)
        right = mean_pull(W["right"], v)
        assert np.abs(right[0]).max() > 0
        zr = zero_rows(c)
        for name, world in W.items():
            if name not in ("right", "slope applied once"):
                add(name + " (mean pull-back)", mean_pull(world, v), right, zr)
        add("the other pool cotangent (mean pull-back)", mean_pull(W["right"], v, other_c(c)), right)
        if E > 1:
            other = ctx["vs"][1] if ctx["vs"][vi] is None else wts
            add("the other weights in place of v (pull-back)", mean_pull(W["right"], other), right, zr)
            add("uniform v (pull-back)", mean_pull(W["right"], np.ones(E)), right, zr)
            add("ensemble weights folded in (mean pull-back)", mean_pull(W["right"], v * wts), right, zr)
            if st.risk is not None:
                add("risk weights in place of v (pull-back)", mean_pull(W["right"], refs.fg(st, i)[2]), right, zr)
    return out


@pytest.mark.parametrize("seed", tf.SEEDS)
def test_no_mix_up_can_hide_under_the_parity_bar(oracle, seed):
    """every family check of the seed that runs: the answer under each likely mix-up -- multi blocks permuted, the block index
    fastest instead of slowest, the other pool direction or cotangent, the stale pulse, the previous operators, raw instead of
    physical coordinates, the slope left out or (GNVP) applied once, rr / ii swapped, ri dropped, wf dropped, one member's
    weights read for all, a term of the HVP dropped, cotangent and tangent swapped, other weights in place of v, ensemble or
    risk weights folded in -- is further than HIDE_MARGIN (1e-6 of the reference's scale,
    test_trajectory_sequences_host.py) from the reference.  Excepted by name, listed, and at most 10 % of the checks: N = 1
    (one slice: the Gauss-Newton operator depends on the pulse through X_1 X_1' alone, and the HVP's Xdot term can vanish),
    the cotangent draw with whole zero rows, and a wf whose entries behind the zero one are all zero."""
    hidden, excepted, looked = [], [], 0
    for ci, (ctx, steps) in enumerate(tf.walk_seed(seed)):
        st, refs = tf.FState(ctx), tf.FRefs(oracle, ctx)
        for si, step in enumerate(steps):
            op = step["op"]
            if op in tf.FAMILY_CHECK_OPS and op != "linear" and tf.runs(st, step) and ctx["served"]:
                found = mixups(refs, st, step)
                looked += bool(found)
                for name, differs, excusable in found:
                    if not differs:
                        where = f"seed {seed} context {ci} ({tf.context_line(ctx)}) step {si} {tf.step_line(step)}: {name}"
                        (excepted if excusable else hidden).append(where)
            st.apply(step)
            if st.refusal:
                st.clear("eval")
    print(f"seed {seed}: {looked} checks looked at, {len(excepted)} excepted")
    print("\n".join(excepted))
    assert not hidden, hidden
    assert len(excepted) <= 0.1 * looked, (len(excepted), looked)


# ---- the references are consistent on the walk's inputs ----------------------------------------------------------------------
def test_gnvp_ref_is_vjp_ref_of_the_weighted_jvp_ref_on_the_walks_inputs(oracle):
    """gnvp_reference.gnvp_ref (recurrences on expm propagators) against vjp_reference.vjp_ref (the double sum) of the weighted
    jvp_reference.jvp_ref (the double sum), for every weight draw of the first eight seeds' served contexts: 1e-12 of the
    scale -- two summation orders of one bilinear form"""
    done = 0
    for seed in list(tf.SEEDS)[:8]:
        for ctx, _ in tf.walk_seed(seed):
            if not ctx["served"] or ctx["N"] > 65:
                continue
            o, x, xdot = ctx["ops"], ctx["pool"][0], ctx["xdots"][1]
            for probe in ctx["probes"]:
                for wi in range(len(probe["weights"])):
                    w, wf, blocks = tf.weight_arrays(probe, wi, ctx["E"])
                    Gn = gr.gnvp_ref(o["A"], o["B"], o["Xi"], x, xdot, ctx["T"], probe["O"] if w is not None else None, w, wf,
                                     probe["per_member"], ctx["variant"], blocks=blocks)
                    O = probe["O"] if probe["n_obs"] else o["Xi"][0]
                    yd, Xd = tf.jr.jvp_ref(o["A"], o["B"], o["Xi"], x, xdot, ctx["T"], O, probe["per_member"] and probe["n_obs"] > 0,
                                           ctx["variant"])
                    ybar = gr.apply_weights(w, yd, blocks) if w is not None else None
                    Gc = vr.vjp_ref(o["A"], o["B"], o["Xi"], x, ctx["T"], probe["O"] if w is not None else None, ybar,
                                    None if wf is None else wf[:, None, None] * Xd, probe["per_member"], ctx["variant"])
                    scale = max(np.abs(Gc).max(), np.abs(Gn).max())
                    assert scale > 0 and np.abs(Gn - Gc).max() <= 1e-12 * scale, (tf.context_line(ctx), wi, np.abs(Gn - Gc).max(), scale)
                    done += 1
    print(f"{done} weight draws")
    assert done >= 60


def test_hvp_ref_against_the_difference_quotient_of_its_model_on_the_walks_inputs(oracle):
    """hvp_reference.hvp_ref against hvp_model_fd (central differences of the VJP recurrence over expm(eps V_s) P_s) on one
    context per kind -- lane and pair kernel, member-chunked, long -- with the walk's own pulses, probes, cotangents and
    tangents: eps = 1e-4, so the quotient's O(eps^2) error and its rounding error ~ 1e-16 / eps both stay below 1e-7 of the
    scale, the bar"""
    seen = {}
    for seed in tf.SEEDS:
        for ctx, _ in tf.walk_seed(seed):
            kind = "long" if ctx["long"] else "chunked" if ctx["chunked"] else ctx["kernel"]
            if ctx["served"] and kind not in seen and (ctx["long"] or 3 <= ctx["N"] <= 20):
                seen[kind] = ctx
        if len(seen) == 4:
            break
    assert sorted(seen) == ["chunked", "lane", "long", "pair"], sorted(seen)
    for kind, ctx in seen.items():
        o, x, xdot = ctx["ops"], ctx["pool"][1], ctx["xdots"][2]
        for p, probe in enumerate(ctx["probes"]):
            for c, t in ((0, 0), (len(probe["cots"]) - 1, 1)):
                (yb, xb), (ybd, xbd) = probe["cots"][c], probe["tans"][t]
                args = (o["A"], o["B"], o["Xi"], x, xdot, ctx["T"])
                kw = dict(O=probe["O"], ybar=yb, xbar=xb, ybar_dot=ybd, xbar_dot=xbd, per_member=probe["per_member"], variant=ctx["variant"])
                G = sum(hr.hvp_ref(*args, **kw))
                Gfd = hr.hvp_model_fd(*args, 1e-4, **kw)
                scale = np.abs(G).max()
                assert scale > 0 and np.abs(G - Gfd).max() <= 1e-7 * scale, (kind, p, c, t, np.abs(G - Gfd).max(), scale)
