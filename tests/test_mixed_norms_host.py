"""The inputs of test_gpu_mixed_norms.py without a GPU: for every row of its table, the pulse built by mixed_norm_cases.py has
the spread of squaring counts, the forward/backward asymmetry and the exact zeros the GPU file relies on, no slice sits on a
switch point of squarings_for, and the two CPU references -- the C oracle (Pade, oracle/grape_oracle.c) and the SciPy
restatement (oracle/grape_numpy.py, Al-Mohy & Higham) -- agree on these inputs to 1e-12, a hundred times inside the GPU bar
(measured over the table, n = 2 .. 66, bounds 0 .. 6.9: 1.7e-14 of max |G| and 7.6e-15 on F at worst, sixty times inside).
The oracle's exact gradient is checked against central differences on one n = 4 case (measured: 1.5e-8 and 5.9e-8 relative
for the two objectives, against the 1e-6 bar)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixed_norm_cases as mn  # noqa: E402
from test_gpu_mixed_norms import ROWS, case_of  # noqa: E402

CASE_KEYS = ("n", "K", "N", "E", "sys_type", "herm", "order", "seed")


def _distinct_cases():
    """rows that share their inputs (one case on several flows) are checked once: {first row of the case: the variants its
    rows run}"""
    first, out = {}, {}
    for rid, r in ROWS.items():
        key = tuple(r[k] for k in CASE_KEYS) + tuple(sorted(r["case"].items()))
        out.setdefault(first.setdefault(key, rid), set()).update(r["variants"])
    return out


VARIANTS = _distinct_cases()
CASES = list(VARIANTS)


@pytest.fixture(scope="module")
def bounds():
    cache = {}

    def get(rid):
        if rid not in cache:
            A, B, Xi, Xt, wts, x, T = case_of(rid)
            b = mn.slice_bounds(A, B, x, T / ROWS[rid]["N"])
            b.setflags(write=False)
            cache[rid] = (A, B, x, T, b)
        return cache[rid]
    return get


def test_squarings_restates_squarings_for():
    assert [mn.squarings(t) for t in (0.0, 0.05, 0.08, 0.0801, 0.16, 0.1601, 6.4, 10.24, 10.25)] == [0, 0, 0, 1, 1, 2, 7, 7, 8]
    M = np.array([[1 + 2j, 0.5], [-3, 1j]])
    assert mn.norm1_bound(M) == 6.0 and mn.norm1_bound(mn.unit(M)) == 1.0


def test_every_flow_of_the_issue_has_a_row():
    ids = " ".join(ROWS)
    for flow in ("lane-", "pair-", "pair-vec-", "fom-lane-", "fom-pair-", "exact-lane-", "exact-pair-w1-", "exact-pair-debug-",
                 "tile-", "hoist1-", "hoist2-", "split-expm-", "chunked-", "action-parts-", "action-whole-", "action-thin2-",
                 "chain-prop-", "exact-tile-", "grid-", "grid-exact-", "any-"):
        assert flow in ids, flow
    for rid, r in ROWS.items():
        assert r["kernels"] or r["info"], f"{rid} asserts no kernel"
        if rid.startswith("action-") and r["order"] != "spikes":
            assert r["order"] == "ramp"                              # the vector flow's shared plan needs the asymmetry


@pytest.mark.parametrize("rid", CASES)
def test_spread_of_the_squaring_counts(bounds, rid):
    r = ROWS[rid]
    b = bounds(rid)[4]
    s = np.array([[mn.squarings(v) for v in row] for row in b])
    print(f"{rid}: bounds {b.min():.4f} .. {b.max():.4f}; squarings per member: " + "; ".join(" ".join(map(str, row)) for row in s))
    if r["order"] == "spikes":                                       # two levels by construction: the bottom and the top
        assert {0, r["s_top"]} <= set(s[0])
    else:
        assert set(s[0]) == set(range(r["s_top"] + 1)), f"member 0 takes {sorted(set(s[0]))}"
    for k in range(r["E"]):
        assert s[k].max() - s[k].min() >= r["s_top"] - 2, f"member {k}: {s[k].min()} .. {s[k].max()}"
    if r["order"] == "shuffled":                                     # neighbouring slices jump by many squarings
        assert np.abs(np.diff(s[0])).max() >= r["s_top"] // 2
    if r["case"].get("top_last"):
        assert s[0][-1] == r["s_top"]


@pytest.mark.parametrize("rid", [c for c in CASES if ROWS[c]["order"] == "ramp"])
def test_a_ramp_is_asymmetric_under_time_reversal(bounds, rid):
    """slice t (forward chain) and slice N-1-t (backward chain, same loop iteration of the vector flow): member 0's bounds differ
    by a factor of 8 or more for at least a third of the slices"""
    b = bounds(rid)[4][0]
    ratio = np.maximum(b, b[::-1]) / np.maximum(np.minimum(b, b[::-1]), 1e-300)
    assert np.count_nonzero(ratio >= 8.0) * 3 >= len(b), ratio


@pytest.mark.parametrize("rid", CASES)
def test_exact_zeros(bounds, rid):
    r = ROWS[rid]
    A, B, x, T, b = bounds(rid)
    zero = np.flatnonzero(np.all(x == 0.0, axis=0))
    assert len(zero) >= 1
    if r["order"] == "spikes":
        assert list(zero) == [1] and b[0][0] > 50 * b[0][1] and b[0][2] < b[0][0] / 10     # a zero column right after a spike
    if r["case"].get("zero_drift_member"):
        assert np.all(A[0] == 0.0) and np.all(b[0][zero] == 0.0)
        for t in zero:
            assert np.all((T / r["N"]) * (A[0] + np.tensordot(x[:, t], B[0], 1)) == 0.0)
    if not r["case"].get("shared_controls", True):
        s = B[:, 0, 0, 0] / B[0, 0, 0, 0]
        assert np.ptp(s.real) > 0.05 and np.allclose(B, s[:, None, None, None] * B[0][None], rtol=1e-14, atol=0)


@pytest.mark.parametrize("rid", CASES)
def test_no_slice_on_a_switch_point(bounds, rid):
    """no bound within 1 % of 0.08 * 2^j: which side a rounding falls on decides nothing"""
    b = bounds(rid)[4]
    for v in b[b > 0].ravel():
        j = np.round(np.log2(v / mn.THETA8))
        if j >= 0:
            assert abs(v / (mn.THETA8 * 2.0 ** j) - 1.0) > 0.01, f"bound {v} is within 1 % of 0.08 * 2^{int(j)}"


def _reference_rows():
    """every distinct case under the formula variants its rows run"""
    return [(rid, v) for rid in CASES for v in sorted(VARIANTS[rid])]


@pytest.mark.parametrize("rid,variant", _reference_rows())
def test_the_two_references_agree(oracle, rid, variant):
    from oracle import grape_numpy
    r = ROWS[rid]
    A, B, Xi, Xt, wts, x, T = case_of(rid)
    D = r["case"].get("distinct_members")
    if D:                                                            # (the other members are copies of the first D)
        assert all(np.array_equal(A[k], A[k % D]) and np.array_equal(Xt[k], Xt[k % D]) for k in range(r["E"]))
        A, B, Xi, Xt, wts = A[:D], B[:D], Xi[:D], Xt[:D], wts[:D]
    F, G = oracle.ensemble_eval(r["sys_type"], A, B, Xi, Xt, wts, x, T, variant=variant)
    F2, G2 = grape_numpy.ensemble_eval(r["sys_type"], A, B, Xi, Xt, wts, x, T, variant=variant)
    eg, ef = np.abs(G - G2).max() / np.abs(G).max(), abs(F - F2) / max(abs(F), 1.0)
    print(f"{rid} v{variant}: |G - G2|_inf / |G|_inf = {eg:.3e}, |F - F2| / max(|F|, 1) = {ef:.3e}")
    assert eg <= 1e-12 and ef <= 1e-12


@pytest.mark.parametrize("objective", [0, 1])
def test_exact_gradient_is_the_derivative_on_a_mixed_norm_pulse(oracle, objective):
    """oracle.ensemble_exact on the n = 4 ramp of the exact-gradient rows against central differences of its own F: step 1e-6,
    1e-6 relative (tests/test_risk_host.py's choice)"""
    rid = "exact-pair-w1-n4-ramp"
    r = ROWS[rid]
    A, B, Xi, Xt, wts, x, T = case_of(rid)

    def f(xx):
        return oracle.ensemble_exact(r["sys_type"], A, B, Xi, Xt, wts, xx, T, variant=0, objective=objective)[0]
    G = oracle.ensemble_exact(r["sys_type"], A, B, Xi, Xt, wts, x, T, variant=0, objective=objective)[1]
    h = 1e-6
    entries = [(0, 0), (1, 1), (0, 2), (1, r["N"] // 2), (0, r["N"] - 3), (1, r["N"] - 1), (0, r["N"] - 1)]     # zero, low, top levels
    fd = {}
    for c, t in entries:
        xp, xm = x.copy(), x.copy()
        xp[c, t] += h
        xm[c, t] -= h
        fd[c, t] = (f(xp) - f(xm)) / (2 * h)
    scale = max(abs(v) for v in fd.values())
    err = max(abs(G[c, t] - fd[c, t]) for c, t in entries) / scale
    print(f"objective {objective}: max |G - fd| / max |fd| = {err:.3e} over {entries}")
    assert err <= 1e-6
