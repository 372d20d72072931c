"""GPU: the lane-pair sweep's copying prologue against its building one (sweep_pair.hip).  By default a context
keeps, per member, a prebuilt record of what the sweep's prologue stages in LDS -- both parity images of the operators, Xi Xt',
the anti-Hermitian sweep's gradient weights, the one-norm bounds -- written by pair_image_kernel wherever the operators are
uploaded, and the prologue copies it; GRAPE_PAIR_IMAGE=0 (read at grape_create) keeps the prologue that builds all of it from
the operators in every call.  The record is written with that prologue's arithmetic, so the two must give the same BITS.

Every case runs in two fresh child processes, one per setting (the variable is read when the context is created): F and G --
and the members' own rows where the context has them -- are compared bit for bit, and member 0 and the last member are held
to the C oracle at the project's 1e-10 bar.  The shapes are the ones at which a copy can go wrong, not the workload's: E = 5
(a last workgroup that is not full), N = 37 (ragged last chunk), K = 3 (odd), every flow and instantiation of the kernel
(anti-Hermitian and full unitary sweep, sandwich, general flow, vector sweep, n = 2, W_t dump), both variants, per-member
controls, a batch, member-chunked evaluation (the record is addressed by the member's number inside the launch), E = 1, and
the two ways a record could go stale: new operators on a live context, and a context whose launch changes between the image
kinds (exact running-cost derivative and back)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1.3
E0, N0, K0 = 5, 37, 3


# ---------------------------------------------------------------------------------------------- problems (parent and children)
def _unitary(rng, n):
    return np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0]


def _density(rng, n):
    M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    M = M @ M.conj().T
    return M / np.trace(M).real


def _problem(seed, E=E0, N=N0, K=K0, n=4, herm=True, states="unitary", shared_b=False):
    rng = np.random.default_rng(seed)

    def gen():
        M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        return (M + M.conj().T) / 2 if herm else M
    A = np.array([gen() for _ in range(E)]) * (0.7 if herm else 0.5)
    if shared_b:                                              # per-member control operators B_k = (1 + eps_k) B
        B0 = np.array([gen() for _ in range(K)]) * 0.5
        B = np.array([(1.0 + e) * B0 for e in rng.uniform(-0.1, 0.1, E)])
    else:
        B = np.array([[gen() for _ in range(K)] for _ in range(E)]) * (0.5 if herm else 0.3)
    if states == "unitary":
        Xi = np.array([_unitary(rng, n) for _ in range(E)])
        Xt = np.array([_unitary(rng, n) for _ in range(E)])
    elif states == "density":
        Xi = np.array([_density(rng, n) for _ in range(E)])
        Xt = np.array([_density(rng, n) for _ in range(E)])
    else:                                                     # n x 1
        Xi = rng.standard_normal((E, n, 1)) + 1j * rng.standard_normal((E, n, 1))
        Xt = rng.standard_normal((E, n, 1)) + 1j * rng.standard_normal((E, n, 1))
    wts = rng.uniform(0.2, 1.0, E)
    x = rng.uniform(-1, 1, (K, N))
    return A, B, Xi, Xt, wts, x


# name -> (system type, problem arguments, engine arguments, environment of the context, kind of run)
CASES = {
    "antiherm_v0": ("UnitaryGate", dict(seed=1), dict(variant=0), {}, "plain"),
    "antiherm_v1": ("UnitaryGate", dict(seed=2), dict(variant=1), {}, "plain"),
    "full_unitary_sweep": ("UnitaryGate", dict(seed=3), {}, {"GRAPE_PAIR_AH": "0"}, "plain"),
    "sandwich": ("StateTransfer", dict(seed=4, states="density"), {}, {}, "plain"),
    "general_flow": ("UnitaryGate", dict(seed=5, herm=False), {}, {}, "plain"),
    "vector_sweep": ("UnitaryGate", dict(seed=6, herm=False, states="vector"), {}, {}, "plain"),
    "two_by_two": ("UnitaryGate", dict(seed=7, n=2), {}, {"GRAPE_SMALL_KERNEL": "pair"}, "plain"),
    "per_member_controls": ("UnitaryGate", dict(seed=8, shared_b=True), {}, {}, "plain"),
    "batch_of_three": ("UnitaryGate", dict(seed=9), dict(max_batch=3), {}, "batch"),
    "member_chunked": ("UnitaryGate", dict(seed=10, E=9), {}, {}, "chunked"),
    "one_member": ("UnitaryGate", dict(seed=11, E=1), {}, {}, "plain"),
    "exact_gradient_w_dump": ("UnitaryGate", dict(seed=12), dict(gradient="exact"), {}, "plain"),
    "new_operators": ("UnitaryGate", dict(seed=13), {}, {}, "new_operators"),
    "running_cost_exact_and_back": ("UnitaryGate", dict(seed=14), {}, {}, "rc_switch"),
}
SECOND_SEED = 113                                             # the operators "new_operators" uploads on the live context


def _batch(x):
    return np.stack([x, 0.5 * x, -0.3 * x])


# ---------------------------------------------------------------------------------------------- the child: every case, one setting
def _run_case(qoc, name):
    sys_type, pk, ek, env, kind = CASES[name]
    A, B, Xi, Xt, wts, x = _problem(**pk)
    N = x.shape[1]
    for k, v in env.items():
        os.environ[k] = v
    out = {}

    def rows(eng, tag):
        F, G = eng.eval(x)
        foms, grads = eng.member_results()
        out[tag + "F"], out[tag + "G"] = np.float64(F), np.array(G)
        out[tag + "foms"], out[tag + "grads"] = np.array(foms), np.array(grads)
    try:
        if kind == "chunked":                                 # half the ensemble's propagators fit the budget
            with qoc.GrapeEngine(sys_type, A, B, Xi, Xt, wts, T, N, member_results=True, **ek) as eng:
                info = eng.info
            unit = info["slices_per_lane"] * 16 * (64 * info["waves_per_member"] // 2) * 16
            os.environ["GRAPE_MAX_WORKSPACE_BYTES"] = str(int(unit * len(A) / 2 * 1.05))
        with qoc.GrapeEngine(sys_type, A, B, Xi, Xt, wts, T, N, member_results=True, **ek) as eng:
            rows(eng, "")
            info = eng.info
            out["names"] = np.array(",".join(eng.kernel_names()))
            out["member_chunk"] = np.int64(info["member_chunk"])
            out["lane_pair"] = np.int64(info["lane_pair"])
            out["pair_antiherm"] = np.int64(info["pair_antiherm"])
            out["workspace_bytes"] = np.int64(info["workspace_bytes"])
            if kind == "batch":
                Fb, Gb = eng.eval_batch(_batch(x))
                out["batchF"], out["batchG"] = np.array(Fb), np.array(Gb)
            if kind == "new_operators":
                A2, B2, Xi2, Xt2, wts2, _ = _problem(seed=SECOND_SEED)
                eng.set_operators(A2, B2, Xi2, Xt2, wts2)
                rows(eng, "second_")
            if kind == "rc_switch":
                rng = np.random.default_rng(77)
                R = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
                eng.set_running_cost_derivative("exact")
                eng.set_running_cost(R, 0.01)
                F, G = eng.eval(x)
                out["rcF"], out["rcG"] = np.float64(F), np.array(G)
                eng.set_running_cost(None)
                eng.set_running_cost_derivative("first_order")
                rows(eng, "second_")
    finally:
        for k in list(env) + ["GRAPE_MAX_WORKSPACE_BYTES"]:
            os.environ.pop(k, None)
    return out


def _child(path):
    sys.path.insert(0, ROOT)
    import quoptimalcontrol_jl_amd as qoc
    res = {}
    for name in CASES:
        for key, val in _run_case(qoc, name).items():
            res[f"{name}/{key}"] = val
    np.savez(path, **res)


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


# ---------------------------------------------------------------------------------------------- the tests
from conftest import assert_parity  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    """{"copy": results of every case with the default, "build": with GRAPE_PAIR_IMAGE=0}, one fresh process each"""
    d = tmp_path_factory.mktemp("pair_prologue")
    res = {}
    for tag, val in (("copy", None), ("build", "0")):
        env = {k: v for k, v in os.environ.items() if k not in ("GRAPE_PAIR_IMAGE", "GRAPE_PAIR_AH", "GRAPE_SMALL_KERNEL",
                                                                "GRAPE_MAX_WORKSPACE_BYTES")}
        if val is not None:
            env["GRAPE_PAIR_IMAGE"] = val
        path = str(d / f"{tag}.npz")
        run = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (tag, run.stdout[-2000:], run.stderr[-2000:])
        with np.load(path) as z:
            res[tag] = {k: z[k] for k in z.files}
    return res


def _get(leg, name):
    return {k.split("/", 1)[1]: v for k, v in leg.items() if k.startswith(name + "/")}


def _member_refs(oracle, name, seed=None):
    sys_type, pk, ek, _, _ = CASES[name]
    A, B, Xi, Xt, wts, x = _problem(**(dict(pk, seed=seed) if seed is not None else pk))
    if seed is not None:
        x = _problem(**pk)[5]                                 # (the live context keeps evaluating the first problem's pulse)
    f = oracle.member_exact if ek.get("gradient") == "exact" else oracle.member_eval
    return {m: f(sys_type, A[m], B[m], Xi[m], Xt[m], x, T, ek.get("variant", 0)) for m in sorted({0, len(A) - 1})}


@pytest.mark.parametrize("name", list(CASES))
def test_copying_and_building_prologue_give_the_same_bits(legs, oracle, name):
    a, b = _get(legs["copy"], name), _get(legs["build"], name)
    assert sorted(a) == sorted(b) and "F" in a
    n = CASES[name][1].get("n", 4)
    for leg in (a, b):
        assert leg["lane_pair"] == 1 and "sweep_pair" in str(leg["names"]), (leg["lane_pair"], leg["names"])
    assert str(a["names"]) == str(b["names"])                 # the same flow in both
    if name == "member_chunked":
        assert a["member_chunk"] < 9 and b["member_chunk"] == a["member_chunk"], (a["member_chunk"], b["member_chunk"])
    if name == "vector_sweep":
        assert "sweep_pair_vec_kernel" in str(a["names"])
    if name in ("antiherm_v0", "antiherm_v1", "full_unitary_sweep", "exact_gradient_w_dump"):
        assert a["pair_antiherm"] == (1 if name.startswith("antiherm") else 0)
    # the copying leg holds the records -- and nothing else differs: E records of both parity images (n = 4: twice, with the
    # B'_c^T images and with the anti-Hermitian sweep's weights) and the K + 1 norm bounds
    E, K = len(a["foms"]), a["G"].shape[0]
    ps = (2 * K + 4) * (n * n // 2) + 8
    assert a["workspace_bytes"] - b["workspace_bytes"] == E * 16 * ((4 if n == 4 else 2) * ps + (K + 2) // 2), \
        (a["workspace_bytes"], b["workspace_bytes"])
    for key in sorted(a):
        if key in ("names", "workspace_bytes"):
            continue
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), \
            (key, float(np.abs(np.asarray(a[key], float) - np.asarray(b[key], float)).max()))
    checks = [("", None)]
    if "second_F" in a:
        checks.append(("second_", SECOND_SEED if name == "new_operators" else None))
    for tag, seed in checks:
        refs = _member_refs(oracle, name, seed=seed)
        for m, (F_ref, G_ref) in refs.items():
            for what, leg in (("copy", a), ("build", b)):
                assert_parity(leg[tag + "foms"][m], leg[tag + "grads"][m], F_ref, G_ref, n, what=f"{name} {tag}{what} member {m}")
    if name == "new_operators":                               # the results follow the new operators
        assert not np.array_equal(a["G"], a["second_G"]) and a["F"] != a["second_F"]
    if name == "running_cost_exact_and_back":                 # back on the anti-Hermitian sweep: the first evaluation's bits again
        assert np.array_equal(a["G"], a["second_G"]) and a["F"] == a["second_F"]
        assert a["rcF"] != a["F"]
    if name == "batch_of_three":
        assert a["batchF"][0] == a["F"] and np.array_equal(a["batchG"][0], a["G"])
        sys_type, pk, _, _, _ = CASES[name]
        A, B, Xi, Xt, wts, x = _problem(**pk)
        for i, xb in enumerate(_batch(x)):
            F_ref, G_ref = oracle.ensemble_eval(sys_type, A, B, Xi, Xt, wts, xb, T)
            assert_parity(a["batchF"][i], a["batchG"][i], F_ref, G_ref, n, what=f"batch array {i}")
