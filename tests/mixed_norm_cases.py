"""Pulses whose slices differ widely in norm -- the inputs of test_mixed_norms_host.py and test_gpu_mixed_norms.py.

Every kernel that forms or applies exp(G_t), G_t = -i dt (A_k + sum_c x[c, t] B_kc), picks its work per slice from the norm
bound of G_t (squarings_for / act_make_plan: the max column sum of |re| + |im|).  The rest of the suite scales whole problems
and draws x ~ U(-1, 1), so neighbouring slices need the same number of squarings.  Here the amplitude of control 0 is set
slice by slice from the levels l_j = 0.05 * 2^j, j = 0 .. s_top, and the level exactly 0 (an envelope's first and last
samples), so that within ONE pulse the squaring count runs from 0 to s_top, jumps by many between neighbours ("shuffled"),
differs between slice t and its mirror N-1-t ("ramp"), or sits at the bottom with isolated spikes ("spikes").

NumPy only; importable without a GPU.

One constant differs from the round number one would write first: the drift is unit(H_k) * (0.0175 / dt) * 4^(k mod 3), not
0.02 / dt.  With 0.02 the members k mod 3 = 1, 2 have drift bounds of exactly 0.08 and 0.32 -- ON two switch points of
squarings_for (0.08 * 2^j), where the count on an all-zero control column would hang on the last bit of a sum; 0.0175 puts the
three drift bounds (0.0175, 0.07, 0.28) an eighth below them and keeps every member's spread (max - min squarings) at
s_top - 2 or more."""
import numpy as np

THETA8 = 0.08                    # kTheta8 of csrc/cmat.hpp
DRIFT = 0.0175                   # bound of dt * A_k for d_k = 1 (see the module docstring)
T = 1.0


def norm1_bound(M):
    """csrc's norm1_bound: max_j sum_i (|Re M_ij| + |Im M_ij|)"""
    M = np.asarray(M)
    return float((np.abs(M.real) + np.abs(M.imag)).sum(axis=-2).max())


def unit(M):
    return M / norm1_bound(M)


def squarings(theta):
    """squarings_for: 0 for theta <= 0.08, else the smallest s with theta / 2^s <= 0.08"""
    s = 0
    while theta > THETA8:
        theta *= 0.5
        s += 1
    return s


def slice_bounds(A, B, x, dt):
    """(E, N): norm1_bound(dt (A_k + sum_c x[c, t] B_kc))"""
    E, N = len(A), x.shape[1]
    out = np.empty((E, N))
    for k in range(E):
        for t in range(N):
            out[k, t] = norm1_bound(dt * (A[k] + np.tensordot(x[:, t], B[k], 1)))
    return out


def level_indices(N, s_top, order, rng, top_last=False):
    """per slice: -1 (the level exactly 0) or j of l_j = 0.05 * 2^j"""
    if order == "spikes":
        lv = np.zeros(N, dtype=int)
        lv[[0, N // 2, N - 1]] = s_top
        if N > 1:
            lv[1] = -1
        return lv
    kinds = [-1] + list(range(s_top, -1, -1))                # a balanced multiset: the zero level, then the top level down
    lv = np.array([kinds[i % len(kinds)] for i in range(N)])
    if order == "ramp":
        return np.sort(lv)                                   # the zero level first, then ascending in (near) equal runs
    assert order == "shuffled", order
    lv = lv[rng.permutation(N)]
    if top_last:                                             # (the ragged last chunk of a chunked time axis gets the top level)
        i = int(np.flatnonzero(lv == s_top)[0])
        lv[i], lv[N - 1] = lv[N - 1], lv[i]
    return lv


def make_case(n, K, N, E, sys_type, herm, order, s_top, seed, cols=None, shared_controls=True, zero_drift_member=False,
              rank_one=True, top_last=False, distinct_members=None):
    """A, B, Xi, Xt, wts, x, T in the shapes GrapeEngine and the oracle take; distinct_members = D: an ensemble of E members
    that repeats D different ones (member k is member k mod D) -- large ensembles with few enough bounds to keep them all off
    the switch points"""
    rng = np.random.default_rng(seed)
    dt = T / N
    E_all, E = E, (distinct_members or E)

    def rnd():
        return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))

    def hermitian():
        M = rnd()
        return (M + M.conj().T) / 2

    B1 = np.array([unit(hermitian()) for _ in range(K)])
    if shared_controls:
        B = np.broadcast_to(B1, (E, K, n, n)).copy()
    else:                                                    # the scaled-controls mode: B_kc = s_k B_c
        B = B1[None] * rng.uniform(0.8, 1.2, E)[:, None, None, None]
    A = np.empty((E, n, n), complex)
    for k in range(E):
        M = rnd()
        H = (M + M.conj().T) / 2
        if not herm:
            H = H + 0.05 * (M - M.conj().T) / 2              # near-unitary propagators: squaring amplifies nothing
        A[k] = unit(H) * (DRIFT / dt) * 4.0 ** (k % 3)
    if zero_drift_member:
        A[0] = 0.0

    lv = level_indices(N, s_top, order, rng, top_last)
    ell = np.where(lv < 0, 0.0, 0.05 * 2.0 ** np.maximum(lv, 0))
    x = np.empty((K, N))
    x[0] = rng.choice([-1.0, 1.0], N) * ell / dt
    for c in range(1, K):
        x[c] = 0.1 * ell / dt * rng.uniform(-1, 1, N)
    x[:, lv < 0] = 0.0

    def vec():
        v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        return v / np.linalg.norm(v)

    def rho():
        if rank_one:
            v = vec()
            return np.outer(v, v.conj())
        return sum(p * np.outer(v, v.conj()) for p, v in zip((0.6, 0.3, 0.1), (vec(), vec(), vec())))

    if sys_type == "UnitaryGate":
        if cols is None:
            Xi = np.array([np.eye(n, dtype=complex)] * E)
            Xt = np.array([np.linalg.qr(rnd())[0] for _ in range(E)])
        else:
            def block():
                M = rng.standard_normal((n, cols)) + 1j * rng.standard_normal((n, cols))
                return M / np.linalg.norm(M)
            Xi = np.array([block() for _ in range(E)])
            Xt = np.array([block() for _ in range(E)])
    else:
        Xi = np.array([rho() for _ in range(E)])
        Xt = np.array([rho() for _ in range(E)])
    wts = rng.uniform(0.2, 1.0, E)
    if E_all != E:
        k = np.arange(E_all) % E
        A, B, Xi, Xt, wts = A[k], B[k], Xi[k], Xt[k], wts[k]
    return A, B, Xi, Xt, wts, x, T
