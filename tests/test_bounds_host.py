"""grape_set_bounds without a GPU: the entry point is declared and exported under the unchanged ABI version 8, the Python
layer validates as the library does, the map / inverse / slope agree with NumPy written out from the header's formula, the
chain rule G_u = G_x s holds against central differences of the oracle's F, GRAPE(bounds=...) starts where it says, and the
random walks of bounds_sequences.py cover every pairing they claim."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_sequences as bs  # noqa: E402
import rc_reference as rcr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def test_header_declares_set_bounds_under_abi_8(qoc):
    hdr = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    assert re.search(r"int grape_set_bounds\(grape_ctx \*ctx, const double \*lo, const double \*hi\);", hdr)
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", hdr).group(1)) == 8 == qoc.engine.ABI_VERSION
    assert "grape_set_bounds" in qoc.engine.EXPORTS
    assert "slope vanishes" in hdr                           # the limit of the method is documented where the ABI is


def test_set_bounds_refuses_a_null_context(qoc):
    lib = qoc.load_library()
    lo, hi = -np.ones(2), np.ones(2)
    assert lib.grape_set_bounds(None, lo.ctypes.data, hi.ctypes.data) == -1
    assert lib.grape_set_bounds(None, None, None) == -1


def test_python_layer_validates_like_the_library(qoc):
    bv = qoc.bounds.bounds_vectors
    assert bv(None, None, 3) == (None, None)
    lo, hi = bv(-0.5, 2.0, 3)                                # scalars broadcast
    assert np.array_equal(lo, [-0.5] * 3) and np.array_equal(hi, [2.0] * 3) and lo.dtype == np.float64
    lo, hi = bv([-1, -INF], [1, INF], 2)                     # mixed finite / free controls
    assert np.array_equal(lo, [-1, -INF]) and np.array_equal(hi, [1, INF])
    for bad_lo, bad_hi in ((-1.0, INF), (-INF, 1.0),         # one-sided
                           (1.0, 1.0), (2.0, 1.0),           # lo >= hi
                           (np.nan, 1.0), (-1.0, np.nan),
                           (INF, INF), (-INF, -INF), (INF, -INF),
                           (None, 1.0), (-1.0, None),
                           ([-1, -1, -1], [1, 1, 1]), ([-1], 1.0)):   # wrong-length vectors for K = 2
        with pytest.raises(ValueError):
            bv(bad_lo, bad_hi, 2)
    with pytest.raises(ValueError):
        bv([-1, 0.5], [1, 0.5], 2)                           # one bad control among good ones
    # GrapeEngine.set_bounds refuses before the library is reached, and keeps what it had
    eng = object.__new__(qoc.GrapeEngine)
    eng.K, eng.N, eng.E, eng._h = 2, 5, 1, None
    assert eng.bounds is None
    for bad in ((-1.0, INF), (1.0, 1.0), (np.nan, 1.0), ([-1, -1, -1], [1, 1, 1])):
        with pytest.raises(ValueError):
            qoc.GrapeEngine.set_bounds(eng, *bad)
    assert eng.bounds is None


@pytest.mark.parametrize("K,N", [(1, 1), (2, 7), (3, 40)])
def test_map_inverse_and_slope_against_numpy(qoc, K, N):
    rng = np.random.default_rng(10 * K + N)
    lo, hi = bs.draw_bounds(rng, K)
    u = rng.uniform(-2, 2, (K, N))
    x, s = qoc.bounds.saturate(u, lo, hi)
    for c in range(K):                                       # the header's formula, written out
        if np.isfinite(lo[c]):
            mid, half = (lo[c] + hi[c]) / 2, (hi[c] - lo[c]) / 2
            th = np.tanh((u[c] - mid) / half)
            assert np.allclose(x[c], mid + half * th, rtol=0, atol=4e-16 * max(abs(lo[c]), abs(hi[c])))
            assert np.allclose(s[c], 1 - th ** 2, rtol=0, atol=4e-16)
            assert np.all(x[c] > lo[c]) and np.all(x[c] < hi[c])
        else:
            assert np.array_equal(x[c], u[c]) and np.all(s[c] == 1.0)
    x2, s2 = bs.sat(u, lo, hi)                               # the tests' own reference says the same
    assert np.allclose(x, x2, rtol=0, atol=1e-15) and np.allclose(s, s2, rtol=0, atol=1e-15)
    # slope = dx/du: central differences, h^2 x'''/6 with |x'''| <= 2 / half^2
    h = 1e-5
    fd = (qoc.bounds.saturate(u + h, lo, hi)[0] - qoc.bounds.saturate(u - h, lo, hi)[0]) / (2 * h)
    half_min = np.min(np.where(np.isfinite(lo), (hi - lo) / 2, 1.0))
    assert np.abs(fd - s).max() <= h * h / (3 * half_min ** 2) + 1e-10
    # the slope is 1 at mid, and the map is the identity there to first order
    mid = np.array([(lo[c] + hi[c]) / 2 if np.isfinite(lo[c]) else 0.3 for c in range(K)])
    xm, sm = qoc.bounds.saturate(np.repeat(mid[:, None], N, 1), lo, hi)
    assert np.array_equal(sm, np.ones((K, N))) and np.allclose(xm, mid[:, None], rtol=0, atol=1e-16)
    # inverse: moderate arguments come back to rounding, amplified by 1 / slope
    back = qoc.bounds.unsaturate(x, lo, hi)
    assert np.all(np.abs(back - u) <= 8e-16 * (1 + np.abs(u)) / s)
    with pytest.raises(ValueError):
        qoc.bounds.unsaturate(np.full((K, N), 5.0), np.full(K, -1.0), np.full(K, 1.0))
    # no bounds at all
    x0, s0 = qoc.bounds.saturate(u, None, None)
    assert np.array_equal(x0, u) and np.all(s0 == 1.0)


def _adgrape_problem(rng, n, K, E, N, T):
    A, B, Xi, wts = rcr.random_problem(rng, n, n, K, E, hermitian=True, scale=0.8)
    Xt = rcr.perturbed_target(A, B, Xi, rng.uniform(-1, 1, (K, N)), T, rng, 1)
    return A, B, Xi, Xt, wts


def test_chain_rule_against_central_differences_of_the_oracle(oracle):
    """The ADGRAPE functional (gradient exact, objective c1): its G_x IS the derivative of its F, so F(sat(u)) must have the
    gradient G_x(sat(u)) s -- checked entry by entry with central differences, h = 1e-5: the truncation term h^2 F'''/6 and
    the rounding term eps |F| / h are both below 1e-8 for F of order 1."""
    n, N, K, E, T = 2, 7, 2, 3, 1.3
    rng = np.random.default_rng(5)
    A, B, Xi, Xt, wts = _adgrape_problem(rng, n, K, E, N, T)
    lo, hi = np.array([-0.7, -0.4]), np.array([0.9, 1.1])
    u = rng.uniform(-1.2, 1.2, (K, N))

    def F_of(uu):
        return oracle.ensemble_exact("UnitaryGate", A, B, Xi, Xt, wts, bs.sat(uu, lo, hi)[0], T, 1, 1)[0]

    x, s = bs.sat(u, lo, hi)
    _, Gx = oracle.ensemble_exact("UnitaryGate", A, B, Xi, Xt, wts, x, T, 1, 1)[:2]
    Gu = Gx * s
    h, fd = 1e-5, np.zeros((K, N))
    for c in range(K):
        for t in range(N):
            d = np.zeros((K, N))
            d[c, t] = h
            fd[c, t] = (F_of(u + d) - F_of(u - d)) / (2 * h)
    print(f"max |fd - G_x s| = {np.abs(fd - Gu).max():.3e}, max |G_x s| = {np.abs(Gu).max():.3e}, "
          f"max |G_x s - G_x| = {np.abs(Gu - Gx).max():.3e}")
    assert np.abs(Gu).max() > 1e-3 and np.abs(Gu - Gx).max() > 1e-3      # the slope matters at this pulse
    assert np.abs(fd - Gu).max() <= 1e-7 * max(1.0, np.abs(Gu).max())


def test_grape_bounds_start_point_rule(qoc):
    alg = qoc.GRAPE(n_slices=6)
    assert alg.bounds is None
    assert qoc.GRAPE(n_slices=6, bounds=(-1.0, 1.0)).bounds == (-1.0, 1.0)
    lo, hi = np.array([-1.0, -INF, 0.0]), np.array([0.5, INF, 4.0])
    guess = np.array([[-3.0, -0.9, 0.0, 0.2, 0.499999, 7.0],
                      [-30.0, -1.0, 0.0, 1.0, 2.0, 30.0],
                      [0.0, 0.5, 2.0, 3.9, 4.0, 9.0]])
    keep = guess.copy()
    u0 = qoc.bounds.bounds_start(guess, lo, hi)
    assert np.array_equal(guess, keep) and u0 is not guess   # the guess object is not modified
    assert np.array_equal(u0[1], guess[1])                   # a free control starts at its guess
    x0, s0 = bs.sat(u0, lo, hi)
    mid, half = np.array([-0.25, 0.0, 2.0]), np.array([0.75, 1.0, 2.0])
    clipped = np.clip(guess, (mid - 0.999 * half)[:, None], (mid + 0.999 * half)[:, None])
    clipped[1] = guess[1]
    assert np.allclose(x0, clipped, rtol=0, atol=1e-13)      # the start is the inverse map of the CLIPPED guess
    # ... so the slope at the start is at least 1 - 0.999^2: the optimiser sees a gradient on every entry
    assert s0.min() >= (1 - 0.999 ** 2) * (1 - 1e-9)
    assert np.all(np.isfinite(u0))
    assert np.array_equal(qoc.bounds.bounds_start(guess, None, None), guess)
    assert np.array_equal(qoc.bounds.bounds_start(guess[:1], -50.0, 50.0)[0, 2:4], [0.0, 50 * np.arctanh(0.2 / 50)])


def test_the_walks_pair_the_bounds_with_every_other_setting():
    cnt = bs.pairings()
    print(cnt)
    for name in ("bounds + basis", "bounds + penalties", "bounds + running cost", "bounds, upload, check",
                 "bounds off after on, check"):
        assert cnt[name] >= 3, (name, cnt)
    a, b = bs.walk_seed(2), bs.walk_seed(2)                  # a pure function of the seed
    assert [[s["op"] for s in st] for _, st in a] == [[s["op"] for s in st] for _, st in b]
    assert np.array_equal(a[0][0]["pool"], b[0][0]["pool"])
    for seed in bs.SEEDS:
        for ctx, steps in bs.walk_seed(seed):
            assert 2 <= ctx["n"] <= 4 and steps[-1]["op"] in bs.CHECK_OPS
            assert all(s["op"] in bs.SETTING_OPS + bs.CHECK_OPS for s in steps)


def test_no_bounded_check_hides_under_the_parity_bar(oracle):
    """every check of the walks with bounds in force: the gradient has size, and the slope moves it by far more than the
    1e-10 bar -- a missing slope cannot pass"""
    hidden = []
    for seed in bs.SEEDS:
        for ci, (ctx, steps) in enumerate(bs.walk_seed(seed)):
            st = bs.BState(ctx)
            for si, step in enumerate(steps):
                st.apply(step)
                if step["op"] not in ("eval", "batch", "device") or st.bounds is None:
                    continue
                th = st.pulses()[step["i"]]
                F, G, x = bs.bounded_reference(oracle, st, th, ("host", seed, ci))
                _, s = st.physical(th)
                if np.abs(G).max() < 1e-3 or np.abs(s - 1).max() < 1e-3:
                    hidden.append((seed, ci, si, np.abs(G).max(), np.abs(s - 1).max()))
    assert not hidden, hidden
