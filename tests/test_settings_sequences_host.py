"""The settings soak's generator (tests/settings_sequences.py) on the CPU: the 24 committed seeds of
test_gpu_settings_soak.py walk the transitions they are there for, no term of the reference can hide under the parity bar,
and the reference cache returns what an uncached call returns.  Needs neither a GPU nor the library."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import settings_sequences as ss  # noqa: E402

CHECKS_WITH_G = ("eval", "batch", "device", "members")
FOMS = ("fom", "fom_members", "fom_batch")


def transitions(seeds):
    """how often each transition of interest is walked; a transition counts when a check observes it"""
    cnt = Counter()
    for seed in seeds:
        for ctx, steps in ss.walk_seed(seed):
            st = ss.State(ctx)
            flip = None                                   # an upload under a standing running cost flipped the flow
            basis_was_on = basis_dropped = pen_upload = False
            for step in steps:
                op = step["op"]
                before = st.ops["herm"]
                st.apply(step)
                if op == "upload":
                    if st.rc is not None and before != st.ops["herm"]:
                        flip = "herm->non" if before else "non->herm"
                    if st.pen is not None:
                        pen_upload = True
                if st.rc is None:
                    flip = None
                if st.pen is None:
                    pen_upload = False
                if op in ("basis_on", "basis_per_control"):
                    basis_was_on, basis_dropped = True, False
                if op == "basis_off" and basis_was_on:
                    basis_dropped = True
                if st.refused:                            # (run_context evaluates right behind the refusal)
                    cnt["rc refused on a partial-class context, then a check"] += 1
                    continue
                if op not in ss.CHECK_OPS or op == "controls":
                    continue
                cnt["checks"] += 1
                batch3 = op == "batch" and ctx["max_batch"] == 3
                if st.rc is not None:
                    if flip:
                        cnt[f"rc on, upload {flip}, check"] += 1
                        flip = None
                    if batch3 and not st.ops["herm"]:
                        cnt["rc on, batch, non-Hermitian"] += 1
                    if batch3 and ctx["chunked"]:
                        cnt["rc on, batch, member-chunked"] += 1
                    if st.rc["J"] == 4:
                        cnt["rc J=4"] += 1
                    if ctx["K"] in (1, 5):
                        cnt[f"rc K={ctx['K']}"] += 1
                    if ctx["T"] == 24.0:
                        cnt["rc T=24"] += 1
                    if st.basis is not None and st.pen is not None:
                        cnt["basis + rc + penalties"] += 1
                if basis_dropped and st.basis is None:
                    cnt["basis off after on, check"] += 1
                    basis_dropped = False
                if pen_upload:
                    cnt["penalties on, upload, check"] += 1
                    pen_upload = False
                if op in FOMS:
                    for name, on in (("penalties", st.pen), ("basis", st.basis), ("rc", st.rc)):
                        if on is not None:
                            cnt[f"fom with {name}"] += 1
    return cnt


WANTED = ["rc on, upload herm->non, check", "rc on, upload non->herm, check", "rc on, batch, non-Hermitian",
          "rc on, batch, member-chunked", "rc J=4", "rc K=1", "rc K=5", "rc T=24", "basis + rc + penalties",
          "basis off after on, check", "penalties on, upload, check", "fom with penalties", "fom with basis", "fom with rc",
          "rc refused on a partial-class context, then a check"]


def test_the_committed_seeds_walk_every_transition():
    cnt = transitions(ss.SEEDS)
    print(dict(cnt))
    short = {k: cnt[k] for k in WANTED if cnt[k] < 5}
    assert not short, short


def test_the_generator_is_a_pure_function_of_the_seed():
    a, b = ss.walk_seed(3), ss.walk_seed(3)
    assert [ss.context_line(c) for c, _ in a] == [ss.context_line(c) for c, _ in b]
    assert [[ss.step_line(s) for s in st] for _, st in a] == [[ss.step_line(s) for s in st] for _, st in b]
    assert np.array_equal(a[0][0]["pool"], b[0][0]["pool"]) and np.array_equal(a[-1][0]["ops"]["A"], b[-1][0]["ops"]["A"])
    for ctx, steps in a:
        assert 3 <= len(steps) <= 9 and steps[-1]["op"] in ss.CHECK_OPS
        assert all(s["op"] in ss.SETTING_OPS + ss.CHECK_OPS for s in steps)


@pytest.mark.parametrize("seed", range(6))
def test_no_term_can_hide_under_the_parity_bar(oracle, seed):
    """the visible() condition of test_gpu_running_cost.py for every setting that is on, and a gradient of size: with both,
    a wrong or missing term moves the result by far more than 1e-10 of max |G_ref|, and no floor for small gradients is needed"""
    hidden = []
    for ci, (ctx, steps) in enumerate(ss.walk_seed(seed)):
        st = ss.State(ctx)
        for si, step in enumerate(steps):
            st.apply(step)
            if (step["op"] not in ss.CHECK_OPS and not st.refused) or step["op"] == "controls":
                continue
            i = si % 3 if st.refused else step["i"]
            F, G, parts, _ = ss.state_reference(oracle, st, st.pulses()[i], (seed, ci))
            where = f"seed {seed} context {ci} ({ss.context_line(ctx)}) step {si} {ss.step_line(step)}"
            gmax = np.abs(G).max()
            if gmax < 1e-3:
                hidden.append((where, "max |G_ref|", gmax))
            for name in ("pen", "rc"):
                if name in parts:
                    share = np.abs(st.project(parts[name][1])).max()
                    if share < 1e-3 * gmax:
                        hidden.append((where, name, share, gmax))
            if step["op"] == "members":                   # the member rows are held to the bar one by one: none of them
                mG = parts["members"][1]                  # is a cancelled remainder next to the others
                for k in range(ctx["E"]):
                    if np.abs(mG[k]).max() < 1e-3 * np.abs(mG).max():
                        hidden.append((where, f"member {k}", np.abs(mG[k]).max(), np.abs(mG).max()))
    assert not hidden, hidden


def test_the_reference_cache_returns_what_an_uncached_call_returns(oracle):
    ctx, steps = ss.walk_seed(0)[0]
    for ctx, steps in ss.walk_seed(0):
        if ctx["full"]:
            break
    st = ss.State(ctx)
    st.apply(dict(op="pen_on", amp=np.full(ctx["K"], 0.3), var=None))
    st.apply(dict(op="rc_on", **ss._draw_rc(np.random.default_rng(5), ctx, ctx["ops"]["Xt"], 2)))
    th = ctx["pool"][1]
    first = ss.state_reference(oracle, st, th, ("cache", 0))
    again = ss.state_reference(oracle, st, th, ("cache", 0))
    plain = ss.state_reference(oracle, st, th, None)
    for a, b in ((first, again), (first, plain)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
        for name in ("plain", "pen", "rc", "members"):
            assert np.array_equal(a[2][name][0], b[2][name][0]) and np.array_equal(a[2][name][1], b[2][name][1])
    assert again[2]["rc"][1] is first[2]["rc"][1] and not first[2]["rc"][1].flags.writeable      # shared, and left unchanged
    assert plain[2]["rc"][1] is not first[2]["rc"][1]
    # a new running cost or new operators are new entries
    st.apply(dict(op="rc_change", **ss._draw_rc(np.random.default_rng(6), ctx, ctx["ops"]["Xt"], 3)))
    other = ss.state_reference(oracle, st, th, ("cache", 0))
    assert other[0] != first[0] and other[2]["plain"][1] is first[2]["plain"][1]
