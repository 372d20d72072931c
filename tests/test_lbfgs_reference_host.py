"""tests/lbfgs_reference.py without a GPU: the long-double two-loop recursion the GPU memory tests are held to
(test_gpu_lbfgs_memory.py) is itself held to oracle/optim_lbfgs.py, the NumPy restatement of Optim.jl's LBFGS(), driven by
the C oracle on the C3-shaped StateTransfer ensemble (E = 4) with a history of 1, 3 and 12 pairs for 16 iterations -- the
ring wraps after 1, 3 and 12 commits.  One step ahead (lbfgs_reference.py): the direction recomputed from the run's own
iterates, gradients and step lengths against the step the run took.

Bars: 1e-13 of max |d_k|.  A double-precision recursion against a long-double one differs by rounding only -- 4.7e-15 at
worst over these runs -- and the bar is about twenty times that.  The mutant -- a window of m + 1 pairs, i.e. an eviction off
by one -- must miss by more than 1e-6 (it misses by 3e-4 .. 1 from the first step after the ring is full): the check can see
a wrong eviction."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_reference as lr  # noqa: E402

MEMORIES = (1, 3, 12)
N_IT = 16
BAR = 1e-13
MUTANT_FLOOR = 1e-6


def _run(qoc, oracle, N, m):
    """one run of the restatement: (iterates x_0 .. x_16, gradients g_0 .. g_16, step lengths, evaluations per iteration)"""
    from oracle import optim_lbfgs
    args, x0 = lr.state_transfer_problem(qoc, N)
    sys_type, A, B, Xi, Xt, wts, T, _ = args

    def fg(x):
        return oracle.ensemble_eval(sys_type, A, B, Xi, Xt, wts, x, T)
    res = optim_lbfgs.lbfgs(fg, x0, m=m, iterations=N_IT)
    tr = res["trace"]
    xs = [np.asarray(x0, float).reshape(-1)] + [t["x"] for t in tr]
    gs = [np.asarray(fg(x.reshape(np.shape(x0)))[1]).reshape(-1) for x in xs]
    per_it = np.diff([1] + [t["evaluations"] for t in tr])
    return res, xs, gs, [t["alpha"] for t in tr], per_it


@pytest.fixture(scope="module")
def runs_100(qoc, oracle):
    """computed once, read-only"""
    return {m: _run(qoc, oracle, 100, m) for m in MEMORIES}


def _check(run, m, what):
    res, xs, gs, alphas, per_it = run
    assert res["status"] == "max_iterations" and len(alphas) == N_IT, (what, res["status"], len(alphas))
    assert per_it.max() <= 15, (what, list(per_it))               # no bisection down to eps(b): the pairs carry information
    ratios, ref = lr.errors(xs, gs, alphas, m)
    print(f"{what}: worst one-step direction error {max(ratios):.2e} of max|d|, pairs per step {ref.n_pairs}")
    assert len(ratios) == N_IT
    assert not any(ref.skipped) and not any(ref.reset), (what, ref.skipped, ref.reset)
    assert ref.n_pairs == [min(k, m) for k in range(N_IT)]
    for k, r in enumerate(ratios):
        assert r <= BAR, (what, k, r)
    # the mutant: an eviction off by one
    mutant, _ = lr.errors(xs, gs, alphas, m + 1)
    print(f"{what}: window m + 1: {['%.1e' % r for r in mutant]}")
    assert max(mutant[:m + 1]) <= BAR                             # the same until the ring is full ...
    assert max(mutant[m + 1:]) > MUTANT_FLOOR, (what, mutant)     # ... and visibly another direction behind it
    return ratios


@pytest.mark.parametrize("m", MEMORIES)
def test_reference_matches_the_restatement_one_step_ahead(runs_100, m):
    _check(runs_100[m], m, f"N=100 m={m}")


@pytest.mark.parametrize("m", MEMORIES)
def test_reference_matches_the_restatement_on_long_vectors(qoc, oracle, m):
    """K N = 2400: the vectors of the block kernel's tests"""
    _check(_run(qoc, oracle, 600, m), m, f"N=600 m={m}")


def test_mpmath_backend_agrees_with_long_double(runs_100):
    """the 50-digit fallback (for platforms whose long double is a double) runs the same code: same directions, same flags"""
    _, xs, gs, alphas, _ = runs_100[3]
    n = 8
    a = lr.direction(xs[:n + 1], gs, alphas[:n], 3)
    b = lr.direction(xs[:n + 1], gs, alphas[:n], 3, force_mpmath=True)
    assert b.mpmath and a.skipped == b.skipped and a.reset == b.reset and a.n_pairs == b.n_pairs
    if not a.mpmath:
        for k in range(n):
            assert np.abs(a.d64[k] - b.d64[k]).max() <= 1e-15 * np.abs(b.d64[k]).max(), k


def test_rules_fire_on_constructed_histories():
    """the curvature rule and the reset, on histories built to trip them"""
    rng = np.random.default_rng(3)
    x0, d = rng.standard_normal(7), rng.standard_normal(7)
    H = np.diag(np.linspace(1.0, 3.0, 7))
    xs = [x0, x0 + d, x0 + 2 * d, x0 + 3 * d]
    gs = [H @ x for x in xs]
    gs[2] = gs[1] - H @ d                                         # negative curvature along the second step: s.y < 0
    ref = lr.direction(xs, gs, [1.0, 1.0, 1.0], 2)
    assert ref.skipped == [False, False, True] and ref.n_pairs == [0, 1, 1] and not any(ref.reset)
    assert np.array_equal(ref.d64[0], -gs[0])
    # H^-1-scaled steepest descent from one pair, by hand: d = -(gamma (g - a y) + (a - b) s)
    s, y, g = xs[1] - xs[0], gs[1] - gs[0], gs[1]
    a = (s @ g) / (s @ y)
    q = (s @ y) / (y @ y) * (g - a * y)
    q = q + (a - (y @ q) / (s @ y)) * s
    assert np.abs(ref.d64[1] + q).max() <= 1e-15 * np.abs(q).max()
    with pytest.raises(ValueError):
        lr.direction(xs, gs, [1.0, 1.0], 2)
