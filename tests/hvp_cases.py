"""The parity cases of tests/test_gpu_hvp.py and their NumPy reference (tests/hvp_reference.py), computed once and shared:
test_hvp_host.py asserts on the same reference values that neither term of Gdot can hide under the GPU tests' tolerance."""
import numpy as np

import hvp_reference as hr
from rc_reference import propagators
from test_gpu_running_cost import SHAPES, make_case

COMBOS = [(1, 0), (3, 1), (16, 0)]                                # (n_obs, per_member)
WAYS = ["dots", "no_dots", "final_only"]                          # (ybar_dot, Xbar_dot) given / NULL / n_obs = 0 with Xbar alone


def cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def shape_problem(n, m, N, E, herm, variant):
    """the case of a row of SHAPES: the problem, probes for every combination, a direction and both pairs of cotangents"""
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    rng = np.random.default_rng(9000 + 100 * n + 10 * m + N + E)
    d = dict(O_mem=cplx(rng, E, 16, n, m), O_sh=cplx(rng, 16, n, m), xdot=rng.standard_normal((c["K"], N)),
             ybar=cplx(rng, E, 16, N + 1), xbar=cplx(rng, E, n, m), ybd=cplx(rng, E, 16, N + 1), xbd=cplx(rng, E, n, m))
    return c, d


def call_arguments(d, way, n_obs, pm):
    """(ops, ybar, xbar, ybar_dot, xbar_dot) of one call"""
    if way == "final_only":
        return None, None, d["xbar"], None, d["xbd"]
    ops = d["O_mem"][:, :n_obs] if pm else d["O_sh"][:n_obs]
    dots = way == "dots"
    return ops, d["ybar"][:, :n_obs], d["xbar"], d["ybd"][:, :n_obs] if dots else None, d["xbd"] if dots else None


_REF = {}


def shape_reference(row):
    """{(way, n_obs, pm): (term of Lamd, term of Xd)} of a row of SHAPES, read-only"""
    key = tuple(row[:6])
    if key not in _REF:
        c, d = shape_problem(*key)
        P = propagators(np.asarray(c["A"], complex), np.asarray(c["B"], complex), c["x"], c["T"], c["variant"])
        out = {}
        for way in WAYS:
            for n_obs, pm in (COMBOS if way != "final_only" else [(0, 0)]):
                ops, yb, xb, ybd, xbd = call_arguments(d, way, n_obs, pm)
                terms = hr.hvp_ref(c["A"], c["B"], c["Xi"], c["x"], d["xdot"], c["T"], ops, yb, xb, ybd, xbd, bool(pm), c["variant"], P)
                for a in terms:
                    a.setflags(write=False)
                out[(way, n_obs, pm)] = terms
        _REF[key] = out
    return _REF[key]


__all__ = ["SHAPES", "COMBOS", "WAYS", "shape_problem", "call_arguments", "shape_reference", "cplx"]
