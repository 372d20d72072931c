"""grape_set_bounds: the NumPy reference the bounds tests are held to, and a small random walk over the settings that live
on a context with the bounds among them.  Shared by test_bounds_host.py (the map, the chain rule, what the walks cover -- on
the CPU), test_gpu_bounds.py and test_gpu_bounds_sequences.py (on the device).  No test functions here.

  sat                  x = mid + half tanh((a - mid) / half) and its slope 1 - tanh^2, straight from the header's formula
  bounded_reference    expansion in NumPy -> sat -> settings_sequences.composed_reference (oracle + penalty_ref +
                       running_cost_ref) on the physical pulse -> slope -> projection in NumPy.  No device result enters it.
  draw_context / draw_steps / BState   the walk: pure functions of the generator state.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import settings_sequences as ss  # noqa: E402

SEEDS = range(8)
CONTEXTS_PER_SEED = 3
SETTING_OPS = ("upload", "bounds_on", "bounds_change", "bounds_off", "basis_on", "basis_per_control", "basis_off", "pen_on",
               "pen_off", "rc_on", "rc_off")
CHECK_OPS = ("eval", "F_only", "batch", "device", "fom", "controls")


def sat(a, lo, hi):
    """(x, s) of the header's map, per control; a control with infinite bounds is the identity"""
    a = np.asarray(a, dtype=np.float64)
    x, s = a.copy(), np.ones_like(a)
    for c in range(a.shape[-2]):
        if np.isfinite(lo[c]):
            mid, half = (lo[c] + hi[c]) / 2, (hi[c] - lo[c]) / 2
            th = np.tanh((a[..., c, :] - mid) / half)
            x[..., c, :] = mid + half * th
            s[..., c, :] = 1 - th ** 2
    return x, s


def draw_bounds(rng, K, mixed=True):
    """per control: finite (lo, hi) around 0, not symmetric; or (-inf, inf) -- at least one control is bounded"""
    lo, hi = -rng.uniform(0.3, 1.2, K), rng.uniform(0.3, 1.2, K)
    if mixed and K > 1:
        free = rng.random(K) < 0.4
        free[int(rng.integers(0, K))] = False
        lo[free], hi[free] = -np.inf, np.inf
    return lo, hi


class BState(ss.State):
    """settings_sequences.State and the bounds"""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.bounds = None

    def apply(self, step):
        op = step["op"]
        if op in ("bounds_on", "bounds_change"):
            self.refused = False
            self.bounds = (step["lo"], step["hi"])
        elif op == "bounds_off":
            self.refused = False
            self.bounds = None
        else:
            super().apply(step)

    def physical(self, theta):
        """(x, slope) of a raw pulse / coefficient array"""
        a, _ = self.expand(theta)
        if self.bounds is None:
            return np.asarray(a, dtype=np.float64), np.ones_like(a)
        return sat(a, *self.bounds)


def bounded_reference(oracle, st, theta, cid=None):
    """(F, G in the space the calls work in, x) of the state's settings at the raw pulse / coefficient array theta"""
    ctx = st.ctx
    x, s = st.physical(theta)
    key = None if cid is None else (cid, st.gen, st.rc_gen)
    F, G, _ = ss.composed_reference(oracle, st.ops, x, ctx["T"], ctx["variant"], st.pen, st.rc, ctx["sys_type"], key)
    return F, st.project(G * s), x


def draw_context(rng):
    n = int(rng.choice([2, 3, 4]))
    ctx = dict(full=True, sys_type="UnitaryGate", n=n, m=int(rng.integers(1, n + 1)), K=int(rng.choice([1, 2, 3])),
               E=int(rng.choice([1, 2, 3])), N=int(rng.choice([1, 3, 8, 20, 65])), T=float(rng.uniform(0.3, 1.5)),
               scale=float(rng.uniform(0.5, 1.0)), variant=int(rng.integers(0, 2)), max_batch=int(rng.choice([1, 3])),
               kernel="lane" if n == 3 else str(rng.choice(["lane", "pair"])))
    ctx["ops"] = ss.full_operators(rng, ctx)
    ctx["pool"] = rng.uniform(-1.5, 1.5, (3, ctx["K"], ctx["N"]))
    return ctx


def draw_steps(rng, ctx):
    """6 to 12 steps; the bounds come on early, a check stands behind the last setting change"""
    steps, st = [], BState(ctx)
    n_steps = int(rng.integers(6, 13))
    while len(steps) < n_steps:
        last = len(steps) == n_steps - 1
        if len(steps) == 0:
            op = "bounds_on"
        elif not last and rng.random() < 0.55:
            menu = ["upload", "basis_on", "basis_per_control", "pen_on", "rc_on"]
            menu += ["bounds_on"] * 3 if st.bounds is None else ["bounds_change", "bounds_off"]
            if st.basis is not None:
                menu += ["basis_off"]
            if st.pen is not None:
                menu += ["pen_off"]
            if st.rc is not None:
                menu += ["rc_off"]
            op = str(rng.choice(menu))
        else:
            op = None
        if op is None:
            menu = ["eval", "eval", "F_only", "batch", "device", "fom"] + (["controls"] * 2 if st.bounds is not None else [])
            step = dict(op=str(rng.choice(menu)), i=int(rng.integers(0, 3)))
        else:
            step = dict(op=op)
            if op == "upload":
                step["ops"] = ss._full_operators(rng, ctx, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
            elif op in ("bounds_on", "bounds_change"):
                step["lo"], step["hi"] = draw_bounds(rng, ctx["K"])
            elif op in ("basis_on", "basis_per_control"):
                step.update(ss._draw_basis(rng, ctx, op == "basis_per_control"))
            elif op == "pen_on":
                step.update(ss._draw_pen(rng, ctx["K"]))
            elif op == "rc_on":
                step.update(ss._draw_rc(rng, ctx, st.ops["Xt"], int(rng.choice([1, 2]))))
        st.apply(step)
        steps.append(step)
    return steps


def walk_seed(seed, contexts=CONTEXTS_PER_SEED):
    rng = np.random.default_rng(7000 + seed)
    out = []
    for _ in range(contexts):
        ctx = draw_context(rng)
        out.append((ctx, draw_steps(rng, ctx)))
    return out


def pairings(seeds=SEEDS):
    """how often a check observes the bounds together with each other setting, and behind an operator upload"""
    cnt = {"bounds + basis": 0, "bounds + penalties": 0, "bounds + running cost": 0, "bounds, upload, check": 0,
           "bounds off after on, check": 0, "checks": 0}
    for seed in seeds:
        for ctx, steps in walk_seed(seed):
            st = BState(ctx)
            uploaded = was_on = dropped = False
            for step in steps:
                st.apply(step)
                op = step["op"]
                if op == "upload" and st.bounds is not None:
                    uploaded = True
                if op in ("bounds_on", "bounds_change"):
                    was_on, dropped = True, False
                if op == "bounds_off":
                    uploaded, dropped = False, was_on
                if op not in CHECK_OPS:
                    continue
                cnt["checks"] += 1
                if dropped and st.bounds is None:
                    cnt["bounds off after on, check"] += 1
                    dropped = False
                if st.bounds is None:
                    continue
                cnt["bounds + basis"] += st.basis is not None
                cnt["bounds + penalties"] += st.pen is not None
                cnt["bounds + running cost"] += st.rc is not None
                if uploaded:
                    cnt["bounds, upload, check"] += 1
                    uploaded = False
    return cnt


def run_context(qoc, oracle, ctx, steps, setenv, cid, log):
    """one context and its steps on the device, every check through conftest.assert_parity against bounded_reference"""
    import torch
    from conftest import assert_parity
    setenv("GRAPE_SMALL_KERNEL", ctx["kernel"])
    n, K, N, T, mb = ctx["n"], ctx["K"], ctx["N"], ctx["T"], ctx["max_batch"]
    st, o, checks = BState(ctx), ctx["ops"], 0
    log("context: " + ss.context_line(dict(ctx, S=0, W=0, budget=None)))
    with qoc.GrapeEngine("UnitaryGate", o["A"], o["B"], o["Xi"], o["Xt"], o["wts"], T, N, variant=ctx["variant"],
                         max_batch=mb) as eng:
        for si, step in enumerate(steps):
            op = step["op"]
            log(f"step {si}: {op} " + str({k: step[k] for k in ("i", "M", "J", "lo", "hi") if k in step}))
            if op == "upload":
                so = step["ops"]
                eng.set_operators(so["A"], so["B"], so["Xi"], so["Xt"], so["wts"])
            elif op in ("bounds_on", "bounds_change"):
                eng.set_bounds(step["lo"], step["hi"])
            elif op == "bounds_off":
                eng.set_bounds(None)
            elif op in ("basis_on", "basis_per_control"):
                eng.set_basis(step["phi"], step["x0"])
            elif op == "basis_off":
                eng.set_basis(None)
            elif op == "pen_on":
                eng.set_penalties(step["amp"], step["var"])
            elif op == "pen_off":
                eng.set_penalties(None, None)
            elif op == "rc_on":
                eng.set_running_cost(step["R"], step["rho"])
            elif op == "rc_off":
                eng.set_running_cost(None)
            st.apply(step)
            if op in SETTING_OPS:
                continue
            checks += 1
            what = f"step {si} {op}"
            th = st.pulses()[step["i"]]
            F_ref, G_ref, x_ref = bounded_reference(oracle, st, th, cid)
            cols = th.shape[1]
            if op == "eval":
                F, G = eng.eval(th)
                assert_parity(F, G, F_ref, G_ref, n, what=what)
            elif op == "F_only":
                F, G = eng.eval(th, want_G=False)
                assert G is None
                assert_parity(F, G_ref, F_ref, G_ref, n, what=what)
            elif op == "fom":
                assert_parity(eng.fom(th), G_ref, F_ref, G_ref, n, what=what)
            elif op == "device":
                xd = torch.as_tensor(np.ascontiguousarray(th.T), device="cuda")
                fg = torch.zeros(K * cols + 1, dtype=torch.float64, device="cuda")
                eng.eval_device(xd.data_ptr(), fg.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                h = fg.cpu().numpy()
                assert_parity(h[-1], h[:-1].reshape(cols, K).T, F_ref, G_ref, n, what=what)
            elif op == "batch":
                ths = np.array([st.pulses()[(step["i"] + b) % 3] for b in range(mb)])
                Fs, Gs = eng.eval_batch(ths)
                for b in range(mb):
                    Fr, Gr, _ = bounded_reference(oracle, st, ths[b], cid)
                    assert_parity(Fs[b], Gs[b], Fr, Gr, n, what=f"{what} entry {b}")
            elif op == "controls":
                xc = eng.controls(th)
                tol = 1e-10 * max(1.0, np.abs(x_ref).max())
                assert xc.shape == (K, N) and np.abs(xc - x_ref).max() <= tol, f"{what}: physical pulse"
                lo, hi = st.bounds
                for c in range(K):
                    if np.isfinite(lo[c]):
                        assert np.all(xc[c] > lo[c]) and np.all(xc[c] < hi[c]), f"{what}: control {c} leaves its bounds"
            else:
                raise AssertionError(f"unknown step {op}")
    return checks
