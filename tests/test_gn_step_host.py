"""grape_gn_step on the host: the NumPy reference of tests/gn_step_reference.py against the references it is built on; the
conditioning the cases promise; gauss_newton._cg -- the restatement the GPU tests hold the call to -- on the reference operator
against numpy.linalg.solve; the ctypes mirrors, the export and every argument check that needs no device.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_step_cases as gsc  # noqa: E402
import gn_step_reference as gsr  # noqa: E402
import gnvp_reference as gr  # noqa: E402
import vjp_reference as vr  # noqa: E402
from test_abi import C_TYPES, header_struct  # noqa: E402

DENSE = [w for w in gsc.SOLVES if (gsc.EXTRA[w][2] * gsc.EXTRA[w][5] if isinstance(w, str) else 2 * gsc.SHAPES[w][2]) <= gsc.DENSE_MAX]
BAR = 1e-12                                                       # of |ref|_inf: two routes through the same f64 model


@pytest.mark.parametrize("which", [1, 5, "Q7"])
def test_the_reference_is_the_composition_of_the_shipped_references(which):
    """L and g from observe + apply_weights + vjp_recurrence, the operator from gnvp_ref: GnProblem only keeps the propagators"""
    s = gsc.solve_case(which)
    c, a, pr = s["c"], s["args"], s["problem"]
    L, ybar, xbar = 0.0, None, None
    y, Xf = vr.observe(c["A"], c["B"], c["Xi"], c["x"], c["T"], a["ops"], a["per_member"], c["variant"]) if a["ops"] is not None \
        else (None, pr.X[-1])
    if a["y_target"] is not None:
        r = y - a["y_target"]
        ybar = gr.apply_weights(a["w"], r)
        L += 0.5 * float(np.sum(np.real(np.conj(r) * ybar)))
    if a["xf_target"] is not None:
        d = Xf - a["xf_target"]
        xbar = a["wf"][:, None, None] * d
        L += 0.5 * float(np.sum(np.real(np.conj(d) * xbar)))
    g = vr.vjp_recurrence(c["A"], c["B"], c["Xi"], c["x"], c["T"], a["ops"], ybar, xbar, a["per_member"], c["variant"])
    assert abs(pr.L - L) <= BAR * L and np.abs(pr.g - g).max() <= BAR * np.abs(g).max()
    v = np.random.default_rng(5).standard_normal(c["x"].shape)
    want = gr.gnvp_ref(c["A"], c["B"], c["Xi"], c["x"], v, c["T"], a["ops"], a["w"], a["wf"], a["per_member"], c["variant"])
    assert np.abs(pr.apply(v) - want).max() <= BAR * np.abs(want).max()


@pytest.mark.parametrize("which", DENSE)
def test_cases_are_conditioned_as_promised_and_cg_reaches_the_dense_solution(which):
    """cond(H + lam) <= 26 with lam = |H|_2 / 25 on a positive semi-definite H; gauss_newton._cg on the reference operator
    with cg_rtol = 1e-13 then reaches p* to 1e-10 |p*| (cond * rtol < 5e-12): the inputs let the reference itself pass"""
    from quoptimalcontrol_jl_amd.gauss_newton import _cg
    s = gsc.solve_case(which)
    pr, lam, p_star = s["problem"], s["lam"], s["p_star"]
    ev = np.linalg.eigvalsh(s["H"])
    print(f"{which}: Q={s['Q']} eigenvalues of H in [{ev[0]:.3e}, {ev[-1]:.3e}] lam={lam:.3e} cond={s['cond']:.2f}")
    assert np.abs(pr.g).max() > 0 and ev[-1] > 0 and ev[0] >= -1e-12 * ev[-1]
    assert s["cond"] <= 26.0
    count = [0]

    def apply(v):
        count[0] += 1
        return pr.apply(v) + lam * v

    p, Ap = _cg(apply, -pr.g, min(4 * s["Q"], 400), 1e-13)
    err, size = np.linalg.norm(p - p_star), np.linalg.norm(p_star)
    print(f"{which}: {count[0]} applications, |p - p*| = {err:.3e} of {size:.3e}")
    assert size > 0 and err <= 1e-10 * size
    assert np.linalg.norm(Ap + pr.g) <= 1e-10 * np.linalg.norm(pr.g)


def test_the_power_iteration_never_overestimates():
    s = gsc.solve_case("Q65")
    est = s["problem"].norm_estimate(np.random.default_rng(3))
    top = np.linalg.eigvalsh(s["H"])[-1]
    print(f"|H|_2 = {top:.6e}, 20 power iterations: {est:.6e}")
    assert 0.5 * top <= est <= top * (1 + 1e-12)


# ---- the binding -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,pyname", [("grape_gn_options", "GrapeGnOptions"), ("grape_gn_result", "GrapeGnResult")])
def test_ctypes_mirrors_match_the_header(qoc, cname, pyname):
    want = header_struct(cname)
    got = getattr(qoc.engine, pyname)._fields_
    assert [f for f, _, _ in want] == [f for f, _ in got]
    for (field, ctype, arr), (_, pyt) in zip(want, got):
        assert arr == 0 and pyt == C_TYPES[ctype][0], field
    sizes = {"grape_gn_options": 24, "grape_gn_result": 56}       # doubles, then two int32: no padding
    assert C.sizeof(getattr(qoc.engine, pyname)) == sizes[cname]


def test_julia_mirrors_match_the_header():
    import re
    from conftest import ROOT
    jl = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    for cname, jname in (("grape_gn_options", "GrapeGnOptions"), ("grape_gn_result", "GrapeGnResult")):
        body = re.search(r"struct %s\n(.*?)\nend" % jname, jl, flags=re.S).group(1)
        got = re.findall(r"^\s*(\w+)::(\w+)", body, flags=re.M)
        want = header_struct(cname)
        assert [f for f, _ in got] == [f for f, _, _ in want]
        assert [t for _, t in got] == [C_TYPES[ctype][1] for _, ctype, _ in want]
    assert "function gn_step(" in jl and ":grape_gn_step" in jl


def test_exported_and_refuses_a_null_context(qoc):
    lib = qoc.load_library()
    assert "grape_gn_step" in qoc.engine.EXPORTS
    opts, res = qoc.engine.GrapeGnOptions(0.1, 1e-10, 5, 0), qoc.engine.GrapeGnResult()
    assert lib.grape_gn_step(None, None, 0, 0, None, None, 0, None, None, None, C.byref(opts), None, None, C.byref(res)) == -1
    assert b"grape_gn_step" in lib.grape_last_error(None)


class _Shapes:
    """the attributes GrapeEngine.gn_step reads before it calls the library (which this stand-in does not have)"""
    K, _cols, n, m, E, N = 2, 9, 3, 2, 4, 9
    _lib = _h = None


def test_wrong_shapes_raise_before_the_library_is_called(qoc):
    eng = _Shapes()
    for name in ("_jvp_probes", "_gnvp_weights"):
        setattr(eng, name, getattr(qoc.GrapeEngine, name).__get__(eng))
    step = qoc.GrapeEngine.gn_step.__get__(eng)
    rng = np.random.default_rng(1)
    x, O = rng.standard_normal((2, 9)), rng.standard_normal((3, 3, 2)) + 0j
    yt, xt = np.zeros((4, 3, 10), complex), np.zeros((4, 3, 2), complex)
    bad = [lambda: step(x[:, :5], O, yt), lambda: step(x, O), lambda: step(x, None, yt), lambda: step(x, O, None, w=np.ones((3, 10))),
           lambda: step(x, O, yt[:, :2]), lambda: step(x, O, yt, w=np.ones((3, 9))), lambda: step(x, O, yt, w=np.ones((2, 3, 10))),
           lambda: step(x, None, xf_target=xt[:3]), lambda: step(x, None, xf_target=xt, wf=np.ones(3)),
           lambda: step(x, None, wf=np.ones(4)), lambda: step(x, O[:, :2], yt), lambda: step(x, O, yt, per_member=True)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(AttributeError):                           # a well-formed call reaches the library
        step(x, O, yt, xf_target=xt)
