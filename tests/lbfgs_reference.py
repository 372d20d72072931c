"""grape_lbfgs' history ring: the high-precision reference the memory tests are held to.  Shared by test_lbfgs_reference_host.py
(the reference against oracle/optim_lbfgs.py, on the CPU) and test_gpu_lbfgs_memory.py (the device against it).  No test
functions here.

The check is ONE STEP AHEAD: from a run's own iterates x_k, their gradients g_k and the accepted step lengths alpha_k the
direction of every step is recomputed from scratch and compared with the one the run took, (x_{k+1} - x_k) / alpha_k.  Every
step is judged from the run's own history, so nothing accumulates: the bar stays at rounding level deep into a run, where an
iterate-by-iterate comparison of two optimisers has long drifted apart.  A ring that keeps one pair too many or too few, reads
a stale row after a wrap or pairs a row with another row's rho gives another direction from the first step after the wrap.

  direction   the L-BFGS direction of every step from the pairs s_j = x_{j+1} - x_j, y_j = g_{j+1} - g_j: the two-loop
              recursion of Nocedal & Wright alg. 7.4, newest -> oldest -> newest over the last (at most m) KEPT pairs,
              rho_j = 1 / s_j.y_j, scaled by gamma = s.y / y.y of the newest kept pair (the identity while there is none),
              with the two rules csrc/lbfgs.hip states for itself:
                 * a pair is kept only if s.y > 1e-10 sqrt(s.s y.y) and y.y > 0
                 * if g.d >= 0 the direction is -g and the history is dropped
  taken       the direction a run took: (x_{k+1} - x_k) / alpha_k
  errors      max |taken - direction| / max |direction| per step

All arithmetic in np.longdouble (x87: eps 1.1e-19); where that is no wider than a double (eps not below 1e-18), mpmath at 50
digits on object arrays -- the same code runs on both."""
from types import SimpleNamespace

import numpy as np

LONGDOUBLE_IS_WIDE = bool(np.finfo(np.longdouble).eps < 1e-18)
CURVATURE_RTOL = 1e-10                       # lbfgs.hip: push = sy > 1e-10 * sqrt(ss * yy) && yy > 0.0


class _Wide:
    """vectors and scalars of the wide format: np.longdouble arrays, or object arrays of mpmath.mpf"""

    def __init__(self, mp):
        self.mp = mp
        if mp:
            import mpmath
            self.mpmath = mpmath
            self.ctx = mpmath.mp.clone()
            self.ctx.dps = 50

    def vec(self, a):
        flat = np.asarray(a, dtype=np.float64).reshape(-1)
        if not self.mp:
            return flat.astype(np.longdouble)
        return np.array([self.ctx.mpf(float(v)) for v in flat], dtype=object)

    def scalar(self, v):
        return self.ctx.mpf(v) if self.mp else np.longdouble(v)

    def sqrt(self, v):
        return self.ctx.sqrt(v) if self.mp else np.sqrt(v)

    def maxabs(self, a):
        return max(abs(v) for v in a) if self.mp else np.abs(a).max()

    def to_double(self, a):
        return np.array([float(v) for v in a]) if self.mp else np.asarray(a, dtype=np.float64)


def _wide(force_mpmath):
    return _Wide(force_mpmath or not LONGDOUBLE_IS_WIDE)


def direction(xs, gs, alphas, m, force_mpmath=False):
    """xs: the iterates x_0 .. x_n, gs: the gradients g_0 .. g_{n-1} (more are ignored), alphas: the n accepted step lengths
    (their count is the number of steps), m: the memory.  Returns a namespace with, per step k = 0 .. n-1,
      d[k]        the direction, in the wide format (d64[k]: rounded to double)
      skipped[k]  the pair (s_{k-1}, y_{k-1}) formed on entry to step k was NOT kept (first rule)
      reset[k]    g_k.d_k >= 0: the direction is -g_k and the history was dropped (second rule)
      n_pairs[k]  pairs the recursion ran over"""
    n = len(alphas)
    if len(xs) != n + 1 or len(gs) < n or m < 1:
        raise ValueError(f"{len(xs)} iterates, {len(gs)} gradients, {n} step lengths, memory {m}")
    w = _wide(force_mpmath)
    X = [w.vec(x) for x in xs]
    G = [w.vec(g) for g in gs[:n]]
    hist = []                                                     # kept pairs (s, y, s.y, y.y), oldest first
    out = SimpleNamespace(d=[], d64=[], skipped=[], reset=[], n_pairs=[], mpmath=w.mp)
    for k in range(n):
        skipped = False
        if k > 0:
            s, y = X[k] - X[k - 1], G[k] - G[k - 1]
            sy, yy, ss = np.dot(s, y), np.dot(y, y), np.dot(s, s)
            if sy > w.scalar(CURVATURE_RTOL) * w.sqrt(ss * yy) and yy > 0:
                hist.append((s, y, sy, yy))
                del hist[:-m]                                     # the ring holds the newest m
            else:
                skipped = True
        q = G[k].copy()
        a = []
        for s, y, sy, _ in reversed(hist):                        # newest -> oldest
            a_j = np.dot(s, q) / sy
            a.append(a_j)
            q = q - a_j * y
        if hist:
            q = (hist[-1][2] / hist[-1][3]) * q                   # gamma of the newest kept pair
        for (s, y, sy, _), a_j in zip(hist, reversed(a)):         # oldest -> newest
            b_j = np.dot(y, q) / sy
            q = q + (a_j - b_j) * s
        d = -q
        reset = not (np.dot(G[k], d) < 0)
        out.n_pairs.append(len(hist))
        if reset:
            d = -G[k]
            hist.clear()
        out.d.append(d)
        out.d64.append(w.to_double(d))
        out.skipped.append(skipped)
        out.reset.append(bool(reset))
    return out


def taken(xs, alphas, force_mpmath=False):
    """the direction each step took, (x_{k+1} - x_k) / alpha_k, in the wide format"""
    w = _wide(force_mpmath)
    X = [w.vec(x) for x in xs]
    return [(X[k + 1] - X[k]) / w.scalar(float(alphas[k])) for k in range(len(alphas))]


def errors(xs, gs, alphas, m, force_mpmath=False):
    """(ratios, ref): ratios[k] = max |taken_k - d_k| / max |d_k| (float), ref = direction(xs, gs, alphas, m)"""
    w = _wide(force_mpmath)
    ref = direction(xs, gs, alphas, m, force_mpmath)
    steps = taken(xs, alphas, force_mpmath)
    return [float(w.maxabs(t - d) / w.maxabs(d)) for t, d in zip(steps, ref.d)], ref


def state_transfer_problem(qoc, N, E=4):
    """the C3-shaped StateTransfer ensemble of test_gpu_lbfgs.py::_ensemble_case("c3_state_transfer") with E members and N
    slices (K = 4 controls, 4 x 4): (engine / oracle arguments up to T, N, start pulse)"""
    w = qoc.workloads.config("C3", E=E, N=N)
    rho0 = np.zeros((4, 4), complex)
    rho0[0, 0] = 1
    psi = np.array([1, 1j, -1, 0.5]) / np.linalg.norm([1, 1j, -1, 0.5])
    Xi = np.broadcast_to(rho0, (w.E, 4, 4)).copy()
    Xt = np.broadcast_to(np.outer(psi, psi.conj()), (w.E, 4, 4)).copy()
    return ("StateTransfer", w.A, w.B, Xi, Xt, w.wts, w.T, w.N), w.x
