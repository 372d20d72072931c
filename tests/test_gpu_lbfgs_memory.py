"""GPU: grape_lbfgs' history ring -- every memory size class and the wrap-around, on every kernel that keeps its own copy
of the ring logic (csrc/lbfgs.hip):

  lbfgs_step_kernel         one wave, K N <= 512                                     (GRAPE_LBFGS_MB=0, or memory > 10)
  lbfgs_step_reg_kernel     512 < K N <= 2048, memory <= 10: history in registers    (GRAPE_LBFGS_MB=0)
  lbfgs_step_block_kernel   1024 threads: K N > 2048, or K N > 512 with memory > 10  (GRAPE_LBFGS_MB=0, or memory > 10)
  lbfgs_dots_kernel + lbfgs_step_mb_kernel   the default for memory <= 10: recursion on scalars from Gram matrices
  lbfgs_direction_kernel + lbfgs_select_kernel   the ladder search

The check is one step ahead (tests/lbfgs_reference.py, held to oracle/optim_lbfgs.py by test_lbfgs_reference_host.py): the
device iterates x_k = lbfgs(x0, iterations = k), k = 1 .. 16 (the runs are bitwise reproducible), their gradients
g_k = eval(x_k) and the accepted step lengths of the longest run's trace give, in long double, the direction a history of
`memory` pairs yields at every step; the device took (x_{k+1} - x_k) / alpha_k.  Bar: PARITY_RTOL = 1e-10 of max |d_k| per
step, on all 16 steps -- nothing accumulates, every step is judged from the device's own history.  Scale: two double
recursions differ from the long-double one by 4.7e-15 at worst on these problems; a ring that keeps one pair too many
misses by 3e-4 .. 1 from the first step after the wrap (test_lbfgs_reference_host.py shows both).

All on the C3-shaped StateTransfer ensemble (E = 4, K = 4: K N picks the kernel), where every line search is regular:
the reference reports no skipped pair and no reset, which each case asserts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_reference as lr  # noqa: E402
from conftest import PARITY_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

N_IT = 16
STEP_KERNELS = {"lbfgs_step_kernel", "lbfgs_step_reg_kernel", "lbfgs_step_block_kernel"}
WORST = {}                                   # kernel -> worst ratio seen so far in this session (printed, never asserted)


def expected_kernel(KN, m, mb_env):
    """csrc/lbfgs.hip launch_lbfgs_step and grape_lbfgs' choice of the many-workgroup step"""
    if mb_env is None and m <= 10:
        return "lbfgs_step_mb_kernel"
    if KN <= 512:
        return "lbfgs_step_kernel"
    if KN <= 2048 and m <= 10:
        return "lbfgs_step_reg_kernel"
    return "lbfgs_step_block_kernel"


@pytest.fixture(scope="module")
def engines(qoc):
    """one context per problem for the whole module (grape_lbfgs reads its options and environment switches per call)"""
    made = {}

    def get(N, E=4, max_batch=1, unitary=False):
        key = (N, E, max_batch, unitary)
        if key not in made:
            if unitary:
                w = qoc.workloads.config("C3", E=E, N=N)
                args, x0 = (w.sys_type, w.A, w.B, w.Xi, w.Xt, w.wts, w.T, w.N), w.x
            else:
                args, x0 = lr.state_transfer_problem(qoc, N, E)
            made[key] = (qoc.GrapeEngine(*args, max_batch=max_batch), x0)
        return made[key]
    yield get
    for eng, _ in made.values():
        eng.close()


def device_history(eng, x0, m, n_it, line_search):
    """(x_0 .. x_n, g_0 .. g_{n-1}, the longest run's trace alphas, its info and kernel names)"""
    xs = [np.array(x0, dtype=np.float64)]
    for k in range(1, n_it + 1):
        xk, info = eng.lbfgs(x0, memory=m, iterations=k, line_search=line_search)
        assert info["iterations"] == k and info["status"] == 2, (k, info)      # 2: stopped by the iteration limit
        xs.append(xk)
    al, _ = eng.lbfgs_trace()
    names = eng.kernel_names()
    gs = [eng.eval(x)[1] for x in xs[:-1]]
    return xs, gs, al, info, names


def one_step_check(eng, x0, m, n_it, line_search, kernel, what):
    """(a)'s check: kernel asserted, all n_it steps compared at PARITY_RTOL, no rule fired; returns the ratios"""
    xs, gs, al, info, names = device_history(eng, x0, m, n_it, line_search)
    ran = STEP_KERNELS & set(names)
    if kernel == "lbfgs_step_mb_kernel":                          # (the first direction, before any commit, is a single-workgroup launch)
        assert "lbfgs_step_mb_kernel" in names and "lbfgs_dots_kernel" in names, (what, names)
    else:
        assert ran == {kernel} and "lbfgs_step_mb_kernel" not in names and "lbfgs_dots_kernel" not in names, (what, names)
    assert info["ladder_fallbacks"] == 0 and "lbfgs_direction_kernel" not in names, (what, info, names)
    assert len(al) == n_it, (what, len(al))
    ratios, ref = lr.errors(xs, gs, al, m)
    WORST[kernel] = max(WORST.get(kernel, 0.0), max(ratios))
    print(f"{what}: {kernel} worst {max(ratios):.2e} of max|d| (alpha {min(al):.2g} .. {max(al):.3g}); "
          f"worst so far {', '.join(f'{k} {v:.2e}' for k, v in sorted(WORST.items()))}")
    assert len(ratios) == n_it
    assert not any(ref.skipped) and not any(ref.reset), (what, ref.skipped, ref.reset)
    assert ref.n_pairs == [min(k, m) for k in range(n_it)], (what, ref.n_pairs)
    for k, r in enumerate(ratios):
        assert r <= PARITY_RTOL, (what, k, r, ratios)
    return ratios


HZ, OPTIM, OFF = "hagerzhang", "optim", "0"
# (N, memory, GRAPE_LBFGS_MB, line search): 6 x 6 x 2 x 2 thinned to every (kernel, memory class) pair on both sides of the
# K N = 512 and 2048 dispatch limits (N = 128 | 129, 512 | 513) and with tails that fill neither a wave nor the 1024-thread
# stride (N = 100, 129, 513, 600); both line searches for each kernel at memory 1 and 3
CASES = [
    # lbfgs_dots_kernel + lbfgs_step_mb_kernel (the default, memory <= 10)
    (100, 1, None, HZ), (100, 1, None, OPTIM), (100, 3, None, HZ), (100, 3, None, OPTIM), (100, 10, None, HZ),
    (128, 2, None, HZ), (128, 5, None, OPTIM),
    (129, 1, None, HZ), (129, 3, None, OPTIM), (129, 10, None, HZ),
    (512, 2, None, OPTIM), (512, 5, None, HZ),
    (513, 1, None, OPTIM), (513, 3, None, HZ), (513, 10, None, OPTIM),
    (600, 1, None, HZ), (600, 2, None, HZ), (600, 3, None, OPTIM), (600, 5, None, HZ), (600, 10, None, HZ),
    # lbfgs_step_kernel (one wave)
    (100, 1, OFF, HZ), (100, 1, OFF, OPTIM), (100, 3, OFF, HZ), (100, 3, OFF, OPTIM), (100, 5, OFF, HZ), (100, 10, OFF, HZ),
    (128, 1, OFF, OPTIM), (128, 2, OFF, HZ), (128, 3, OFF, HZ), (128, 5, OFF, OPTIM), (128, 10, OFF, OPTIM),
    (100, 12, None, HZ), (100, 12, OFF, OPTIM), (128, 12, OFF, HZ), (128, 12, None, OPTIM),
    # lbfgs_step_reg_kernel (history in registers)
    (129, 1, OFF, HZ), (129, 1, OFF, OPTIM), (129, 3, OFF, HZ), (129, 3, OFF, OPTIM), (129, 2, OFF, HZ), (129, 10, OFF, HZ),
    (512, 1, OFF, HZ), (512, 3, OFF, OPTIM), (512, 2, OFF, OPTIM), (512, 5, OFF, HZ), (512, 10, OFF, OPTIM),
    # lbfgs_step_block_kernel (1024 threads)
    (513, 1, OFF, HZ), (513, 1, OFF, OPTIM), (513, 3, OFF, HZ), (513, 3, OFF, OPTIM), (513, 5, OFF, HZ), (513, 10, OFF, OPTIM),
    (600, 1, OFF, OPTIM), (600, 2, OFF, HZ), (600, 3, OFF, HZ), (600, 5, OFF, OPTIM), (600, 10, OFF, HZ),
    (129, 12, OFF, HZ), (512, 12, None, OPTIM), (513, 12, None, HZ), (600, 12, OFF, OPTIM), (600, 12, None, HZ),
]


def _set_mb(monkeypatch, mb):
    if mb is None:
        monkeypatch.delenv("GRAPE_LBFGS_MB", raising=False)
    else:
        monkeypatch.setenv("GRAPE_LBFGS_MB", mb)


def test_the_cases_reach_every_kernel_and_memory_class():
    """the thinned cross product keeps what it must: each kernel at a memory that wraps within 16 steps, on both sides of
    each dispatch limit, with both line searches at memory 1 and 3; the wave and block kernels at memory 12"""
    seen = {}
    for N, m, mb, ls in CASES:
        seen.setdefault(expected_kernel(4 * N, m, mb), set()).add((N, m, ls))
    assert set(seen) == STEP_KERNELS | {"lbfgs_step_mb_kernel"}
    for kernel, hit in seen.items():
        for m in (1, 3):
            assert {ls for _, mm, ls in hit if mm == m} == {HZ, OPTIM}, (kernel, m)
        assert {1, 2, 3, 5, 10} <= {mm for _, mm, _ in hit}, kernel
    assert {N for N, m, _ in seen["lbfgs_step_kernel"] if m == 12} == {100, 128}
    assert {N for N, m, _ in seen["lbfgs_step_block_kernel"] if m == 12} == {129, 512, 513, 600}
    assert {N for N, _, _ in seen["lbfgs_step_mb_kernel"]} == {100, 128, 129, 512, 513, 600}
    assert {N for N, m, _ in seen["lbfgs_step_reg_kernel"]} == {129, 512}
    assert len(CASES) == len(set(CASES)) and 55 <= len(CASES) <= 65


@pytest.mark.parametrize("N,m,mb,line_search", CASES,
                         ids=[f"N{N}-m{m}-{'mb' if mb is None else 'mb0'}-{ls}" for N, m, mb, ls in CASES])
def test_direction_one_step_ahead(engines, monkeypatch, N, m, mb, line_search):
    """(a) every step-kernel path, 16 steps each"""
    _set_mb(monkeypatch, mb)
    eng, x0 = engines(N)
    one_step_check(eng, x0, m, N_IT, line_search, expected_kernel(4 * N, m, mb), f"N={N} m={m} MB={mb} {line_search}")


@pytest.mark.parametrize("N", [100, 600])
@pytest.mark.parametrize("m", [1, 3])
def test_iterates_match_the_host_restatement_with_a_small_memory(engines, monkeypatch, N, m):
    """(b) grape_lbfgs(line_search = "optim", memory = m) against oracle/optim_lbfgs.lbfgs(m = m) driven by the same device
    evaluation, with the bars of test_gpu_lbfgs.py::test_iterates_match_the_host_restatement -- accepted step length to
    1e-6, iterate to 1e-9, evaluations per iteration equal -- over all 12 iterations: the ring wraps after 1 / 3 of them.
    (Two double restatements that differ only in summation order drift apart by 3.5e-14 in x and 6.9e-13 in alpha over 16
    iterations of these problems: the bars hold with room.)"""
    from oracle import optim_lbfgs
    monkeypatch.delenv("GRAPE_LBFGS_MB", raising=False)
    eng, x0 = engines(N)
    n_it = 12
    ref = optim_lbfgs.lbfgs(lambda x: eng.eval(x), x0, m=m, iterations=n_it)
    xs = []
    for k in range(1, n_it + 1):
        xk, info = eng.lbfgs(x0, memory=m, iterations=k, line_search="optim")
        assert info["iterations"] == k and info["status"] == 2, (k, info)
        xs.append(xk)
    al, ev = eng.lbfgs_trace()
    tr = ref["trace"]
    assert len(tr) == n_it and len(al) == n_it
    per_dev = np.diff(np.concatenate([[1], ev]))
    per_ref = np.diff([1] + [t["evaluations"] for t in tr])
    assert per_ref.max() <= 15, list(per_ref)                     # regular line searches throughout
    for i in range(n_it):
        a_ref, x_ref = tr[i]["alpha"], tr[i]["x"].reshape(np.shape(x0))
        assert abs(al[i] - a_ref) <= 1e-6 * abs(a_ref), (i, al[i], a_ref)
        assert np.abs(xs[i] - x_ref).max() <= 1e-9 * max(1.0, np.abs(x_ref).max()), i
        assert per_dev[i] == per_ref[i], (i, list(per_dev), list(per_ref))


def _power_of_two_step(dx, d_ref):
    """the power of two nearest to the least-squares step length of dx along d_ref"""
    return 2.0 ** int(np.rint(np.log2(float(np.dot(dx, d_ref) / np.dot(d_ref, d_ref)))))


@pytest.mark.parametrize("start", ["guess", "fourth_iterate"])
@pytest.mark.parametrize("m", [1, 3])
def test_ladder_search_keeps_its_own_ring(engines, monkeypatch, m, start):
    """(c) line_search = "ladder" runs lbfgs_direction_kernel + lbfgs_select_kernel (the pair is pushed inside select).  No
    trace is kept there; the accepted step is one of a factor-2 ladder from 1, so x_{k+1} - x_k = 2^j d_ref with an integer j,
    at the same 1e-10 bar on all 12 steps.  The ladder accepts on sufficient decrease alone, so the reference's two rules may
    fire and are applied as the kernels state them.
    From the guess they fire on EVERY step: the gradient there is small (Hager-Zhang's first step is ~400 long), the ladder
    takes twelve steps of length 1 along -g, each with s.y <= 0, no pair is ever kept and the ring is never used -- measured,
    and asserted here so that a change of that behaviour is seen.  From the fourth iterate of the default run the ladder's
    steps of length 1 or 1/2 all keep their pair (the same on the CPU with the oracle): the ring fills and wraps, which is
    what this test is for."""
    monkeypatch.delenv("GRAPE_LBFGS_MB", raising=False)
    eng, x0 = engines(100, max_batch=4)
    n_it = 12
    if start == "fourth_iterate":
        x0, info = eng.lbfgs(x0, iterations=4, line_search="optim")
        assert info["iterations"] == 4
    xs = [np.array(x0, dtype=np.float64)]
    for k in range(1, n_it + 1):
        xk, info = eng.lbfgs(x0, memory=m, iterations=k, line_search="ladder")
        assert info["iterations"] == k and info["status"] == 2 and info["probes"] == 4, (k, info)
        xs.append(xk)
    names = eng.kernel_names()
    assert "lbfgs_direction_kernel" in names and "lbfgs_select_kernel" in names, names
    assert not (STEP_KERNELS | {"lbfgs_step_mb_kernel", "lbfgs_dots_kernel"}) & set(names), names
    gs = [eng.eval(x)[1] for x in xs[:-1]]
    ref = lr.direction(xs, gs, [1.0] * n_it, m)
    alphas = [_power_of_two_step((xs[k + 1] - xs[k]).reshape(-1), ref.d64[k]) for k in range(n_it)]
    ratios, _ = lr.errors(xs, gs, alphas, m)
    WORST["lbfgs_direction_kernel"] = max(WORST.get("lbfgs_direction_kernel", 0.0), max(ratios))
    print(f"ladder m={m} from the {start}: worst {max(ratios):.2e} of max|d|, steps 2^{[int(np.log2(a)) for a in alphas]}, "
          f"pairs {ref.n_pairs}, skipped {[int(v) for v in ref.skipped]}, reset {[int(v) for v in ref.reset]}")
    assert len(ratios) == n_it
    if start == "guess":
        assert ref.n_pairs == [0] * n_it and not any(ref.reset), (ref.n_pairs, ref.reset)
    else:
        assert not any(ref.skipped) and not any(ref.reset), (ref.skipped, ref.reset)
        assert ref.n_pairs == [min(k, m) for k in range(n_it)], ref.n_pairs           # eight / ten steps behind the wrap
    for k, r in enumerate(ratios):
        assert r <= PARITY_RTOL, (m, start, k, r, ratios)


def test_unitary_gate_run_with_ladder_fallbacks(engines, monkeypatch):
    """(d) UnitaryGate, C3 at E = 4, N = 150, memory = 3: the reference's gradient is not the derivative of its figure of
    merit there, a Hager-Zhang search may find no bracket and hand the iteration to the ladder, after which the host leaves the
    Gram path for the single-workgroup kernels.  One step ahead on every step the run takes, the reference's rules firing where
    they do.  The trace holds the Hager-Zhang iterations only: a step whose least-squares length matches the next trace entry
    takes it, any other step is a ladder step and must be a power of two -- and there must be as many of those as the run
    reports accepted fallbacks.
    Measured: this run is SHORT.  Its first two iterations both fall back to the ladder, the third finds no acceptable step on
    the ladder either and the run ends there (status 3, ladder_fallbacks = 3, 230 evaluations): two steps are compared, both
    from lbfgs_direction_kernel + lbfgs_select_kernel behind a failed Hager-Zhang search, and lbfgs_step_mb_kernel never
    commits.  The ring does not wrap here; that is (a)'s and (c)'s business."""
    monkeypatch.delenv("GRAPE_LBFGS_MB", raising=False)
    eng, x0 = engines(150, unitary=True)
    m = 3
    xs = [np.array(x0, dtype=np.float64)]
    for k in range(1, N_IT + 1):
        xk, info = eng.lbfgs(x0, memory=m, iterations=k)
        if info["iterations"] < k:                                # the run ended by itself: every step it took is in xs
            break
        xs.append(xk)
    al, _ = eng.lbfgs_trace()
    names = eng.kernel_names()
    n = len(xs) - 1
    assert n >= 2 and info["iterations"] == n, (n, info)
    gs = [eng.eval(x)[1] for x in xs[:-1]]
    ref = lr.direction(xs, gs, [1.0] * n, m)
    alphas, at, ladder_steps = [], 0, 0
    for k in range(n):
        dx = (xs[k + 1] - xs[k]).reshape(-1)
        est = float(np.dot(dx, ref.d64[k]) / np.dot(ref.d64[k], ref.d64[k]))
        if at < len(al) and abs(al[at] - est) <= 1e-6 * abs(est):
            alphas.append(float(al[at]))
            at += 1
        else:
            alphas.append(_power_of_two_step(dx, ref.d64[k]))
            ladder_steps += 1
    ratios, _ = lr.errors(xs, gs, alphas, m)
    print(f"UnitaryGate N=150 m=3: {n} steps, status {info['status']}, ladder_fallbacks {info['ladder_fallbacks']}, "
          f"worst {max(ratios):.2e} of max|d|, alphas {['%.3g' % a for a in alphas]}, pairs {ref.n_pairs}, "
          f"skipped {[int(v) for v in ref.skipped]}, reset {[int(v) for v in ref.reset]}, kernels {names}")
    # accepted ladder steps: every fallback but a last one that found no step (status 3: the run ends without moving)
    failed_last = 1 if info["status"] == 3 else 0
    assert at == len(al) and ladder_steps == info["ladder_fallbacks"] - failed_last, (at, len(al), ladder_steps, info)
    if info["ladder_fallbacks"]:
        assert "lbfgs_select_kernel" in names and "lbfgs_direction_kernel" in names, names
    assert len(ratios) == n
    for k, r in enumerate(ratios):
        assert r <= PARITY_RTOL, (k, r, ratios)


# ---- (e) the option itself --------------------------------------------------------------------------------------------------
def test_memory_zero_is_the_default_of_ten(engines, monkeypatch):
    """memory = 0 and memory = 10: the same bits, past the 11th commit (the first eviction of a ten-pair ring)"""
    eng, x0 = engines(100)
    for mb in (None, OFF):
        _set_mb(monkeypatch, mb)
        xa, ia = eng.lbfgs(x0, memory=0, iterations=14)
        xb, ib = eng.lbfgs(x0, memory=10, iterations=14)
        assert np.array_equal(xa, xb) and ia["minimum"] == ib["minimum"] and ia["evaluations"] == ib["evaluations"]
        assert ia["iterations"] == 14


@pytest.mark.parametrize("N,kernel", [(100, "lbfgs_step_kernel"), (600, "lbfgs_step_block_kernel")])
def test_the_largest_memory(engines, monkeypatch, N, kernel):
    """memory = 64, the largest accepted: the wave kernel's 64 recursion coefficients behind its vector in LDS, the block
    kernel's 64-entry table"""
    monkeypatch.delenv("GRAPE_LBFGS_MB", raising=False)
    eng, x0 = engines(N)
    assert expected_kernel(4 * N, 64, None) == kernel
    one_step_check(eng, x0, 64, N_IT, HZ, kernel, f"N={N} m=64")


def test_memory_beyond_64_is_refused(qoc, engines):
    eng, x0 = engines(100)
    with pytest.raises(qoc.GrapeError) as ei:
        eng.lbfgs(x0, memory=65, iterations=2)
    assert ei.value.status == -1                                  # GRAPE_ERR_INVALID_ARG
    x1, info = eng.lbfgs(x0, memory=64, iterations=2)             # the context serves the next call
    assert info["iterations"] == 2


@pytest.mark.parametrize("mb", [None, OFF])
def test_the_option_reaches_the_kernels(engines, monkeypatch, mb):
    """memory = 1 and memory = 3 walk together while both hold one pair and apart once the smaller ring has evicted"""
    _set_mb(monkeypatch, mb)
    eng, x0 = engines(100)
    x1 = [eng.lbfgs(x0, memory=1, iterations=k)[0] for k in (2, 6)]
    x3 = [eng.lbfgs(x0, memory=3, iterations=k)[0] for k in (2, 6)]
    scale = max(1.0, np.abs(x1[0]).max())
    assert np.abs(x1[0] - x3[0]).max() <= 1e-12 * scale           # one pair each: the same direction up to rounding
    assert np.abs(x1[1] - x3[1]).max() > 1e-6 * scale             # (the m + 1 window misses by 3e-4 .. 1 per direction)


@pytest.mark.parametrize("mb", [None, OFF])
def test_the_longest_control_array(qoc, engines, monkeypatch, mb):
    """K N = 16384, the limit (sixteen elements per thread of the block kernel; 64 workgroups of the many-workgroup step),
    memory = 3, 8 iterations; one slice more is refused"""
    _set_mb(monkeypatch, mb)
    eng, x0 = engines(4096, E=2)
    one_step_check(eng, x0, 3, 8, HZ, expected_kernel(16384, 3, mb), f"N=4096 E=2 m=3 MB={mb}")


def test_one_slice_beyond_the_longest_is_refused(qoc):
    args, x0 = lr.state_transfer_problem(qoc, 4097, E=2)
    with qoc.GrapeEngine(*args) as eng:
        with pytest.raises(qoc.GrapeError) as ei:
            eng.lbfgs(x0, memory=3, iterations=2)
        assert ei.value.status == -2                              # GRAPE_ERR_UNSUPPORTED
