"""The parity cases of tests/test_gpu_gnvp.py and their NumPy reference (tests/gnvp_reference.py), computed once and shared."""
import numpy as np

import gnvp_reference as gr
from rc_reference import propagators
from test_gpu_running_cost import SHAPES, make_case

COMBOS = [(1, 0), (3, 1), (16, 0)]                                # (n_obs, per_member)
# scalar weights shared by the members, with wf / full blocks per member, without wf / n_obs = 0 with wf alone
WAYS = ["scalar_shared_wf", "blocks_member", "final_only"]


def cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def psd_blocks(rng, *shape):
    """planes (3, *shape) of positive definite 2x2 blocks L L' with L = [[a, 0], [b, c]]"""
    a, b, c = rng.uniform(0.3, 1.2, shape), rng.standard_normal(shape), rng.uniform(0.3, 1.2, shape)
    return np.stack([a * a, a * b, b * b + c * c])


def shape_problem(n, m, N, E, herm, variant):
    """the case of a row of SHAPES: the problem, probes for every combination, a direction and both kinds of weights"""
    c = make_case(100 * n + 10 * m + N + E, n, m, N, E, hermitian=herm, variant=variant)
    rng = np.random.default_rng(9500 + 100 * n + 10 * m + N + E)
    d = dict(O_mem=cplx(rng, E, 16, n, m), O_sh=cplx(rng, 16, n, m), xdot=rng.standard_normal((c["K"], N)),
             w_sh=rng.uniform(0.2, 1.5, (16, N + 1)), w_mem=psd_blocks(rng, E, 16, N + 1), wf=rng.uniform(0.2, 1.5, E))
    return c, d


def call_arguments(d, way, n_obs, pm):
    """(ops, w, wf) of one call"""
    if way == "final_only":
        return None, None, d["wf"]
    ops = d["O_mem"][:, :n_obs] if pm else d["O_sh"][:n_obs]
    if way == "scalar_shared_wf":
        return ops, d["w_sh"][:n_obs], d["wf"]
    return ops, d["w_mem"][:, :, :n_obs], None


_REF = {}


def shape_reference(row):
    """{(way, n_obs, pm): Gn} of a row of SHAPES, read-only"""
    key = tuple(row[:6])
    if key not in _REF:
        c, d = shape_problem(*key)
        P = propagators(np.asarray(c["A"], complex), np.asarray(c["B"], complex), c["x"], c["T"], c["variant"])
        out = {}
        for way in WAYS:
            for n_obs, pm in (COMBOS if way != "final_only" else [(0, 0)]):
                ops, w, wf = call_arguments(d, way, n_obs, pm)
                Gn = gr.gnvp_ref(c["A"], c["B"], c["Xi"], c["x"], d["xdot"], c["T"], ops, w, wf, bool(pm), c["variant"], P)
                Gn.setflags(write=False)
                out[(way, n_obs, pm)] = Gn
        _REF[key] = out
    return _REF[key]


__all__ = ["SHAPES", "COMBOS", "WAYS", "shape_problem", "call_arguments", "shape_reference", "cplx", "psd_blocks"]
