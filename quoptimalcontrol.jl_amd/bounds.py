"""Smooth amplitude bounds (grape_set_bounds, include/grape_hip.h): the host-side arithmetic of the map the device applies.

    x = mid + half tanh((u - mid) / half),   dx/du = 1 - tanh^2(...),   mid = (lo + hi) / 2,  half = (hi - lo) / 2

per control; a control with lo = -inf, hi = +inf is the identity.  Nothing here touches the device: set_bounds validates
with bounds_vectors, solve() finds its start point with bounds_start, and the tests use saturate as their reference."""
import numpy as np

START_MARGIN = 0.999     # a guess is clipped to mid +- START_MARGIN * half before the map is inverted (bounds_start)


def bounds_vectors(lo, hi, K):
    """(lo, hi) as float64 K-vectors, or (None, None) for lo = hi = None (bounds off).  Scalars broadcast to K.  Every
    control needs finite lo < hi, or lo = -inf with hi = +inf (that control is free); anything else is a ValueError, as it
    is GRAPE_ERR_INVALID_ARG in the library."""
    if lo is None and hi is None:
        return None, None
    if lo is None or hi is None:
        raise ValueError("bounds: lo and hi must both be given (use -inf, +inf for a free control), or both be None")
    out = []
    for name, v in (("lo", lo), ("hi", hi)):
        v = np.asarray(v, dtype=np.float64)
        v = np.full(K, float(v)) if v.ndim == 0 else np.ascontiguousarray(v)
        if v.shape != (K,):
            raise ValueError(f"bounds: {name} must be a scalar or have {K} entries")
        out.append(v)
    lo, hi = out
    for c in range(K):
        free = lo[c] == -np.inf and hi[c] == np.inf
        if not free and not (np.isfinite(lo[c]) and np.isfinite(hi[c]) and lo[c] < hi[c]):
            raise ValueError(f"bounds: control {c}: need finite lo < hi, or lo = -inf and hi = +inf (got {lo[c]}, {hi[c]})")
    return lo, hi


def _mid_half(lo, hi):
    fin = np.isfinite(lo)
    mid = np.where(fin, (np.where(fin, lo, 0.0) + np.where(fin, hi, 0.0)) / 2, 0.0)
    half = np.where(fin, (np.where(fin, hi, 1.0) - np.where(fin, lo, -1.0)) / 2, 1.0)
    return fin[:, None], mid[:, None], half[:, None]


def saturate(u, lo, hi):
    """(x, s): the physical pulse of the raw pulse u (..., K, N) and the slope dx/du, per entry."""
    u = np.asarray(u, dtype=np.float64)
    lo, hi = bounds_vectors(lo, hi, u.shape[-2])
    if lo is None:
        return u.copy(), np.ones_like(u)
    fin, mid, half = _mid_half(lo, hi)
    th = np.tanh((u - mid) / half)
    return np.where(fin, mid + half * th, u), np.where(fin, 1.0 - th * th, 1.0)


def unsaturate(x, lo, hi):
    """The raw pulse u with saturate(u) = x; x must lie strictly inside the bounds."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = bounds_vectors(lo, hi, x.shape[-2])
    if lo is None:
        return x.copy()
    fin, mid, half = _mid_half(lo, hi)
    r = np.where(fin, (x - mid) / half, 0.0)
    if np.any(np.abs(r) >= 1.0):
        raise ValueError("unsaturate: x must lie strictly inside the bounds")
    return np.where(fin, mid + half * np.arctanh(r), x)


def bounds_start(guess, lo, hi):
    """The raw start point of an optimisation from a physical guess (K, N): the guess clipped to mid +- 0.999 half on every
    bounded control, then the inverse map.  The clip keeps the start out of deep saturation, where the slope -- and with it
    the gradient the optimiser sees -- vanishes.  Returns a new array; the guess is not modified."""
    g = np.array(guess, dtype=np.float64)
    lo, hi = bounds_vectors(lo, hi, g.shape[-2])
    if lo is None:
        return g
    fin, mid, half = _mid_half(lo, hi)
    g = np.where(fin, np.clip(g, mid - START_MARGIN * half, mid + START_MARGIN * half), g)
    return unsaturate(g, lo, hi)
