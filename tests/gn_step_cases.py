"""The cases of tests/test_gpu_gn_step.py and tests/test_gn_step_host.py and their NumPy reference (tests/gn_step_reference.py),
computed once and shared.

  shape cases   the rows of gnvp_cases.SHAPES (by import) with the probes and weights of gnvp_cases.shape_problem and random
                targets of order 1; loss and gradient for every (way, n_obs, per_member) of gnvp_cases, the solve for ONE of
                them per row (SOLVE_WAYS in turn)
  extra cases   (K, N) with Q = K N = 1, 7, 65 and 1 200: below, at and above the CG kernels' workgroup of 1 024 threads
The damping is lam = |H|_2 / 25: from the reference's dense H where Q <= DENSE_MAX = 200, so that cond(H + lam) <= 26 (H is
positive semi-definite); elsewhere from 20 power iterations, an estimate between half the norm and the norm from a random
start, so that cond < 51.
"""
import numpy as np

import gn_step_reference as gsr
import gnvp_cases as gc
from gnvp_cases import COMBOS, SHAPES, WAYS
from rc_reference import propagators
from test_gpu_running_cost import make_case

DENSE_MAX = 200
# (way, n_obs, per_member) of the solve on row i of SHAPES: i modulo the list
SOLVE_WAYS = [("scalar_shared_wf", 3, 1), ("blocks_member", 1, 0), ("final_only", 0, 0), ("scalar_shared_wf", 16, 0),
              ("blocks_member", 3, 1)]
# name: n, m, N, E, hermitian, K
EXTRA = {"Q1": (2, 1, 1, 2, True, 1), "Q7": (2, 2, 7, 3, False, 1), "Q65": (3, 2, 13, 2, True, 5), "Q1200": (2, 2, 300, 2, True, 4)}


def shape_targets(row):
    """(y_target (E, 16, N+1), xf_target (E, n, m)) of a row of SHAPES: random, of order 1"""
    n, m, N, E = row[:4]
    rng = np.random.default_rng(9700 + 100 * n + 10 * m + N + E)
    return gc.cplx(rng, E, 16, N + 1), gc.cplx(rng, E, n, m)


def call_arguments(row, way, n_obs, pm):
    """(c, dict(ops, y_target, w, xf_target, wf, per_member)) of one call on a row of SHAPES"""
    c, d = gc.shape_problem(*row[:6])
    ops, w, wf = gc.call_arguments(d, way, n_obs, pm)
    yt, xt = shape_targets(row)
    return c, dict(ops=ops, y_target=None if w is None else yt[:, :n_obs], w=w, xf_target=None if wf is None else xt, wf=wf,
                   per_member=bool(pm))


def all_calls(row):
    return [(way, n_obs, pm) for way in WAYS for n_obs, pm in (COMBOS if way != "final_only" else [(0, 0)])]


def problem_of(c, a, P=None):
    return gsr.GnProblem(c["A"], c["B"], c["Xi"], c["x"], c["T"], a["ops"], a["y_target"], a["w"], a["xf_target"], a["wf"],
                         a["per_member"], c["variant"], P=P)


_LG, _SOLVE = {}, {}


def loss_and_gradient(row):
    """{(way, n_obs, pm): (L, g)} of a row of SHAPES, read-only"""
    key = tuple(row[:6])
    if key not in _LG:
        c, _ = gc.shape_problem(*key)
        P = propagators(np.asarray(c["A"], complex), np.asarray(c["B"], complex), c["x"], c["T"], c["variant"])
        out = {}
        for call in all_calls(row):
            pr = problem_of(*call_arguments(row, *call), P=P)
            pr.g.setflags(write=False)
            out[call] = (pr.L, pr.g)
        _LG[key] = out
    return _LG[key]


def _solve(c, a, seed):
    pr = problem_of(c, a)
    Q = pr.K * pr.N
    if Q <= DENSE_MAX:
        H = pr.dense()
        H = 0.5 * (H + H.T)
        ev = np.linalg.eigvalsh(H)
        lam = ev[-1] / 25.0
        cond = (ev[-1] + lam) / (max(ev[0], 0.0) + lam)
        p_star = gsr.gn_step_ref(pr, lam, H)
        for v in (H, p_star):
            v.setflags(write=False)
    else:
        H, cond, p_star = None, None, None
        lam = pr.norm_estimate(np.random.default_rng(seed)) / 25.0
    pr.g.setflags(write=False)
    return dict(c=c, args=a, problem=pr, Q=Q, H=H, lam=float(lam), cond=cond, p_star=p_star)


def solve_case(which):
    """the solve of row i of SHAPES (which = i) or of an extra case (which = its name): dict(c, args, problem, Q, H, lam, cond,
    p_star); H, cond and p_star are None above DENSE_MAX"""
    if which not in _SOLVE:
        if isinstance(which, str):
            n, m, N, E, herm, K = EXTRA[which]
            c = make_case(9800 + N, n, m, N, E, K=K, hermitian=herm)
            rng = np.random.default_rng(9801 + N)
            a = dict(ops=gc.cplx(rng, 3, n, m), y_target=gc.cplx(rng, E, 3, N + 1), w=rng.uniform(0.2, 1.5, (3, N + 1)),
                     xf_target=gc.cplx(rng, E, n, m), wf=rng.uniform(0.2, 1.5, E), per_member=False)
            _SOLVE[which] = _solve(c, a, 9802 + N)
        else:
            row = SHAPES[which]
            c, a = call_arguments(row, *SOLVE_WAYS[which % len(SOLVE_WAYS)])
            _SOLVE[which] = _solve(c, a, 9900 + which)
    return _SOLVE[which]


SOLVES = list(range(len(SHAPES))) + list(EXTRA)

__all__ = ["SHAPES", "EXTRA", "SOLVES", "SOLVE_WAYS", "DENSE_MAX", "all_calls", "call_arguments", "loss_and_gradient", "solve_case",
           "problem_of"]
