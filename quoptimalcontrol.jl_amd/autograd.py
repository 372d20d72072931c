"""torch.autograd on top of the trajectory read-out: any differentiable loss written in torch on the expectation values
y[k, j, s] = tr(O_kj' X_ks) and on the final states X_final gets its gradient with respect to the controls from the device
(GrapeEngine.observe forward, GrapeEngine.observe_vjp backward; include/grape_hip.h: grape_eval_observables /
grape_eval_vjp).  No new kernel or setting per loss; the basis, the bounds and the optimisers stay usable, since x is whatever
the engine takes (theta / u with a basis / bounds in force) and the gradient comes back in the same coordinates.

torch is imported here and nowhere else in the package: `import quoptimalcontrol_jl_amd` never pulls it in.

    from quoptimalcontrol_jl_amd import autograd
    x = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    y, X_final = autograd.trajectory(eng, x, ops)
    loss = -torch.log(1 - y[0, 0].abs() ** 2).sum()          # a log-barrier on a population
    loss.backward()                                         # x.grad: first order in dt, like the running cost's gradient

Forward mode: both functions carry a jvp, so torch.autograd.forward_ad dual numbers pass through them -- the tangent of
(y, X_final) along the tangent of x is GrapeEngine.observe_jvp's (grape_eval_jvp), the exact transpose of the backward.
(torch.func.jvp needs the setup_context form of a Function and is not served.)

Which derivative: the engine's setting carries through.  By default both directions are first order in dt
(GrapeEngine.trajectory_derivative == "first_order"), so torch.autograd.gradcheck on these functions FAILS -- the backward is
the transpose of a first-order linearisation, not of the forward's true derivative.  After
eng.set_trajectory_derivative("exact") the backward and the jvp differentiate the propagators the forward used, exactly:
gradcheck passes and a quasi-Newton solve on a custom loss converges to its own gradient tolerance.

Second order: trajectory(..., twice=True) makes the backward differentiable as well (GrapeEngine.observe_hvp, grape_eval_hvp),
so torch.autograd.grad(..., create_graph=True) and torch.autograd.functional.hvp give Hessian-vector products of a loss on
(y, X_final) -- first order in dt, engines without bounds in the first-order derivative mode.  twice=False (the default) is the
once-differentiable function it always was.

trajectory_mean is trajectory for a loss on the ENSEMBLE-AVERAGED read-out, sum_k v_k y[k] (what an experiment on an
inhomogeneously broadened ensemble measures): the sum, the broadcast of its cotangent and the sum of the tangents run on the
device (GrapeEngine.observe_mean / observe_vjp_mean / observe_jvp_mean), so the member axis never crosses the bus.

trajectory_device is the same for a workflow that lives on the GPU (once differentiable): x, y, X_final, the loss and x.grad are CUDA tensors on the
engine's device, the read-out and the pull-back run on torch's current stream (GrapeEngine.observe_device /
observe_vjp_device) and nothing crosses to the host.
"""
import numpy as np
import torch


class _Trajectory(torch.autograd.Function):
    """(y, X_final) = observe(x); backward = observe_vjp with the cotangents torch supplies (dl/dRe + i dl/dIm for a
    complex output of a real loss: the convention grape_eval_vjp takes).  A cotangent torch does not supply -- an output the
    loss never touched -- is passed as None."""

    @staticmethod
    def forward(ctx, x, engine, ops, per_member, final):
        xn = x.detach().numpy()
        out = engine.observe(xn, ops, per_member=per_member, final=final)
        y, Xf = out if final else (out, None)
        ctx.engine, ctx.ops, ctx.per_member, ctx.final = engine, ops, per_member, final
        ctx.xn = np.array(xn, copy=True)
        ctx.set_materialize_grads(False)
        y_t = torch.from_numpy(y)
        if final:
            return y_t, torch.from_numpy(Xf)
        return y_t

    @staticmethod
    def backward(ctx, ybar, xbar=None):
        if ybar is None and xbar is None:
            return None, None, None, None, None
        yb = None if ybar is None else ybar.detach().resolve_conj().numpy()
        xb = None if xbar is None else xbar.detach().resolve_conj().numpy()
        G = ctx.engine.observe_vjp(ctx.xn, ctx.ops, ybar=yb, xbar_final=xb, per_member=ctx.per_member)
        return torch.from_numpy(G), None, None, None, None

    @staticmethod
    def jvp(ctx, xdot, *_):
        """forward mode: the tangents of (y, X_final) -- of y alone with final=False -- along the tangent of x"""
        xd = xdot.detach().numpy()
        out = ctx.engine.observe_jvp(ctx.xn, xd, ctx.ops, per_member=ctx.per_member, final=ctx.final)
        if ctx.final:
            return torch.from_numpy(out[0]), torch.from_numpy(out[1])
        return torch.from_numpy(out)


def _np(t):
    return None if t is None else np.array(t.detach().resolve_conj().numpy(), copy=True)


class _TrajectoryHVP(torch.autograd.Function):
    """The backward of _TrajectoryVJP as a function of its upstream w (and of x, ybar, xbar, in which it is not differentiated
    again): (observe_hvp(x, xdot=w, ybar, xbar), observe_jvp(x, w)) -- linear in w.  torch.autograd.functional.hvp
    differentiates a backward with respect to its upstream (the double-backward trick), so this has a backward of its own:
    for upstream (u_x, u_y, u_X) the gradient with respect to w is observe_hvp(x, xdot=u_x, ybar, xbar, ybar_dot=u_y,
    xbar_final_dot=u_X) -- J' (u_y, u_X) exactly, and the curvature operator applied to u_x AS IT STANDS, where the transpose
    belongs: the operator of grape_eval_hvp is symmetric up to its same-slice block (first order in dt, include/grape_hip.h)."""

    @staticmethod
    def forward(ctx, x, w, ybar, xbar, engine, ops, per_member):
        xn, wn, yb, xb = _np(x), _np(w), _np(ybar), _np(xbar)
        ctx.engine, ctx.ops, ctx.per_member = engine, ops, per_member
        ctx.xn, ctx.yb, ctx.xb = xn, yb, xb
        ctx.set_materialize_grads(False)
        gx = engine.observe_hvp(xn, wn, ops, ybar=yb, xbar_final=xb, per_member=per_member)
        yd, Xd = engine.observe_jvp(xn, wn, ops, per_member=per_member, final=True)
        return torch.from_numpy(gx), torch.from_numpy(yd), torch.from_numpy(Xd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ux, uy, uX):
        if ux is None and uy is None and uX is None:
            return None, None, None, None, None, None, None
        xd = np.zeros_like(ctx.xn) if ux is None else _np(ux)
        gw = ctx.engine.observe_hvp(ctx.xn, xd, ctx.ops, ybar=ctx.yb, xbar_final=ctx.xb, ybar_dot=_np(uy), xbar_final_dot=_np(uX),
                                    per_member=ctx.per_member)
        return None, torch.from_numpy(gw), None, None, None, None, None


class _TrajectoryVJP(torch.autograd.Function):
    """G = observe_vjp(x; ybar, xbar) as a differentiable function of (x, ybar, xbar): the backward of _TrajectoryTwice.  Its
    own backward, for an upstream w on G: observe_hvp(x, xdot=w, ybar, xbar) for x (grape_eval_hvp) and, G being linear in the
    cotangents with the Jacobian's transpose, observe_jvp(x, w)'s (ydot, Xdot_final) for (ybar, xbar) -- through
    _TrajectoryHVP, so that it can be differentiated with respect to w in turn."""

    @staticmethod
    def forward(ctx, x, ybar, xbar, engine, ops, per_member):
        ctx.engine, ctx.ops, ctx.per_member = engine, ops, per_member
        ctx.has_y, ctx.has_X = ybar is not None, xbar is not None
        ctx.save_for_backward(x, *[t for t in (ybar, xbar) if t is not None])
        return torch.from_numpy(engine.observe_vjp(_np(x), ops, ybar=_np(ybar), xbar_final=_np(xbar), per_member=per_member))

    @staticmethod
    def backward(ctx, w):
        if w is None:
            return None, None, None, None, None, None
        saved = list(ctx.saved_tensors)
        x = saved.pop(0)
        ybar = saved.pop(0) if ctx.has_y else None
        xbar = saved.pop(0) if ctx.has_X else None
        gx, gy, gX = _TrajectoryHVP.apply(x, w, ybar, xbar, ctx.engine, ctx.ops, ctx.per_member)
        return gx, gy if ctx.has_y else None, gX if ctx.has_X else None, None, None, None


class _TrajectoryTwice(torch.autograd.Function):
    """_Trajectory whose backward is itself differentiable: it runs through _TrajectoryVJP, so a backward with
    create_graph=True (torch.autograd.functional.hvp, Newton-CG) reaches grape_eval_hvp."""

    @staticmethod
    def forward(ctx, x, engine, ops, per_member, final):
        xn = x.detach().numpy()
        out = engine.observe(xn, ops, per_member=per_member, final=final)
        y, Xf = out if final else (out, None)
        ctx.engine, ctx.ops, ctx.per_member, ctx.final = engine, ops, per_member, final
        ctx.xn = np.array(xn, copy=True)
        ctx.save_for_backward(x)
        ctx.set_materialize_grads(False)
        y_t = torch.from_numpy(y)
        if final:
            return y_t, torch.from_numpy(Xf)
        return y_t

    @staticmethod
    def backward(ctx, ybar, xbar=None):
        if ybar is None and xbar is None:
            return None, None, None, None, None
        (x,) = ctx.saved_tensors
        G = _TrajectoryVJP.apply(x, ybar, xbar, ctx.engine, ctx.ops, ctx.per_member)
        return G, None, None, None, None

    jvp = _Trajectory.jvp


def trajectory(engine, x, ops, per_member=False, final=True, twice=False):
    """y (E, n_obs, N+1) complex128 and -- final=True -- X_final (E, n, m) of the pulse x, a CPU float64 tensor of the shape
    engine.eval takes, differentiable with respect to x.  ops as in GrapeEngine.observe (at least one probe); it is not
    differentiated.  Returns (y, X_final), or y alone with final=False.
    twice=True makes the backward differentiable too (a second Function around observe_vjp whose backward is
    GrapeEngine.observe_hvp / observe_jvp): torch.autograd.grad(..., create_graph=True) and torch.autograd.functional.hvp work,
    first order in dt like everything here.  The engine must serve observe_hvp (no bounds, first-order trajectory derivative).
    trajectory_device stays once-differentiable."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device.type != "cpu":
        raise TypeError("trajectory: x must be a CPU float64 tensor")
    if ops is None:
        raise ValueError("trajectory: at least one probe is needed (GrapeEngine.observe(final=True) gives X_final alone)")
    ops = np.array(ops.detach().numpy() if isinstance(ops, torch.Tensor) else ops, dtype=np.complex128, copy=True)
    if twice:
        return _TrajectoryTwice.apply(x, engine, ops, bool(per_member), bool(final))
    return _Trajectory.apply(x, engine, ops, bool(per_member), bool(final))


class _TrajectoryMean(torch.autograd.Function):
    """(y_mean, X_mean) = observe_mean(x); backward = observe_vjp_mean, jvp = observe_jvp_mean: the member axis stays on the
    device in all three directions (include/grape_hip.h: grape_eval_observables_mean / _vjp_mean / _jvp_mean)."""

    @staticmethod
    def forward(ctx, x, engine, ops, v, per_member, final):
        xn = x.detach().numpy()
        out = engine.observe_mean(xn, ops, v=v, per_member=per_member, final=final)
        y, Xm = out if final else (out, None)
        ctx.engine, ctx.ops, ctx.v, ctx.per_member, ctx.final = engine, ops, v, per_member, final
        ctx.xn = np.array(xn, copy=True)
        ctx.set_materialize_grads(False)
        y_t = torch.from_numpy(y)
        if final:
            return y_t, torch.from_numpy(Xm)
        return y_t

    @staticmethod
    def backward(ctx, ybar, xbar=None):
        if ybar is None and xbar is None:
            return None, None, None, None, None, None
        yb = None if ybar is None else ybar.detach().resolve_conj().numpy()
        xb = None if xbar is None else xbar.detach().resolve_conj().numpy()
        G = ctx.engine.observe_vjp_mean(ctx.xn, ctx.ops, ybar_mean=yb, xbar_mean=xb, v=ctx.v, per_member=ctx.per_member)
        return torch.from_numpy(G), None, None, None, None, None

    @staticmethod
    def jvp(ctx, xdot, *_):
        """forward mode: the tangents of (y_mean, X_mean) -- of y_mean alone with final=False -- along the tangent of x"""
        xd = xdot.detach().numpy()
        out = ctx.engine.observe_jvp_mean(ctx.xn, xd, ctx.ops, v=ctx.v, per_member=ctx.per_member, final=ctx.final)
        if ctx.final:
            return torch.from_numpy(out[0]), torch.from_numpy(out[1])
        return torch.from_numpy(out)


def trajectory_mean(engine, x, ops, v=None, per_member=False, final=True):
    """trajectory with the member axis summed on the device: y_mean (n_obs, N+1) = sum_k v_k y[k] and -- final=True -- X_mean
    (n, m) = sum_k v_k X_final[k] of the pulse x, a CPU float64 tensor of the shape engine.eval takes, differentiable with respect
    to x (backward and forward_ad).  v (E,): the weights, not differentiated; None: the engine's ensemble weights.  What a loss
    on the averaged populations needs, at about the cost of its kernels: (N+1) n_obs numbers cross the bus in each direction
    instead of (N+1) n_obs E.  Once differentiable; the engine's trajectory-derivative setting carries through as in trajectory."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device.type != "cpu":
        raise TypeError("trajectory_mean: x must be a CPU float64 tensor")
    if ops is None:
        raise ValueError("trajectory_mean: at least one probe is needed (GrapeEngine.observe_mean(final=True) gives X_mean alone)")
    ops = np.array(ops.detach().numpy() if isinstance(ops, torch.Tensor) else ops, dtype=np.complex128, copy=True)
    if v is not None:
        v = np.array(v.detach().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64, copy=True)
    return _TrajectoryMean.apply(x, engine, ops, v, bool(per_member), bool(final))


def _dev_probes(ops, per_member):
    """(n_obs, n, m) / (E, n_obs, n, m) -> the library's column-major (n, m, [E,] n_obs), on the GPU"""
    return (ops.permute(1, 0, 3, 2) if per_member else ops.transpose(-1, -2)).contiguous()


class _TrajectoryDevice(torch.autograd.Function):
    """_Trajectory on device memory.  The backward pulls back along the trajectory the forward left in the engine's workspace
    (d_x = 0, no second sweep) when reuse is set and engine.calls says that nothing has touched the engine since; otherwise,
    and when the library finds the trajectory gone after all, it runs with the saved x."""

    @staticmethod
    def forward(ctx, x, engine, ops, per_member, final, reuse):
        E, n, m, N = engine.E, engine.n, engine.m, engine.N
        n_obs = ops.shape[1] if per_member else ops.shape[0]
        xf = x.detach().t().contiguous()                     # (K, cols) column-major
        Of = _dev_probes(ops, per_member)
        y = torch.empty((E, n_obs, N + 1), dtype=torch.complex128, device=x.device)
        Xf = torch.empty((E, m, n), dtype=torch.complex128, device=x.device) if final else None
        stream = torch.cuda.current_stream(x.device).cuda_stream
        engine.observe_device(xf.data_ptr(), n_obs, per_member, Of.data_ptr(), y.data_ptr(), Xf.data_ptr() if final else 0, 0, stream)
        ctx.engine, ctx.per_member, ctx.n_obs, ctx.reuse, ctx.final = engine, per_member, n_obs, reuse, final
        ctx.xf, ctx.Of, ctx.stamp = xf, Of, engine.calls
        ctx.set_materialize_grads(False)
        if final:
            return y, Xf.transpose(-1, -2)
        return y

    @staticmethod
    def backward(ctx, ybar, xbar=None):
        if ybar is None and xbar is None:
            return None, None, None, None, None, None
        eng = ctx.engine
        yb = None if ybar is None else ybar.detach().resolve_conj().contiguous()
        xb = None if xbar is None else xbar.detach().resolve_conj().transpose(-1, -2).contiguous()
        G = torch.empty_like(ctx.xf)
        stream = torch.cuda.current_stream(G.device).cuda_stream
        n_obs, Of = (ctx.n_obs, ctx.Of.data_ptr()) if yb is not None else (0, 0)
        args = (n_obs, ctx.per_member, Of, 0 if yb is None else yb.data_ptr(), 0 if xb is None else xb.data_ptr(), G.data_ptr(), stream)
        done = False
        if ctx.reuse and eng.calls == ctx.stamp:
            try:
                eng.observe_vjp_device(0, *args)
                done = True
            except Exception as exc:                         # (NOT_READY: a call that bypassed the engine's counter, a member chunk)
                if getattr(exc, "status", None) != -5:
                    raise
        if not done:
            eng.observe_vjp_device(ctx.xf.data_ptr(), *args)
        return G.t(), None, None, None, None, None

    @staticmethod
    def jvp(ctx, xdot, *_):
        """forward mode, under the backward's rule: along the stored trajectory (d_x = 0) when reuse is set and nothing has
        touched the engine since, else with the saved x.  Either way the workspace then holds the trajectory of the saved x,
        so the stamp moves on and a backward (or another jvp) that follows directly may reuse it."""
        eng = ctx.engine
        E, n, m, N = eng.E, eng.n, eng.m, eng.N
        xdf = xdot.detach().t().contiguous()                 # (K, cols) column-major
        yd = torch.empty((E, ctx.n_obs, N + 1), dtype=torch.complex128, device=xdf.device)
        Xd = torch.empty((E, m, n), dtype=torch.complex128, device=xdf.device) if ctx.final else None
        stream = torch.cuda.current_stream(xdf.device).cuda_stream
        args = (xdf.data_ptr(), ctx.n_obs, ctx.per_member, ctx.Of.data_ptr(), yd.data_ptr(), Xd.data_ptr() if ctx.final else 0, stream)
        done = False
        if ctx.reuse and eng.calls == ctx.stamp:
            try:
                eng.observe_jvp_device(0, *args)
                done = True
            except Exception as exc:                         # (NOT_READY: a call that bypassed the engine's counter, a member chunk)
                if getattr(exc, "status", None) != -5:
                    raise
        if not done:
            eng.observe_jvp_device(ctx.xf.data_ptr(), *args)
        ctx.stamp = eng.calls
        if ctx.final:
            return yd, Xd.transpose(-1, -2)
        return yd


def trajectory_device(engine, x, ops, per_member=False, final=True, reuse=True):
    """trajectory on the GPU: x is a CUDA float64 tensor on the engine's device, of the shape engine.eval takes; returns CUDA
    complex128 y (E, n_obs, N+1) and -- final=True -- X_final (E, n, m), differentiable with respect to x.  ops: (n_obs, n, m),
    or (E, n_obs, n, m) with per_member=True, a tensor or anything numpy converts; not differentiated.  Forward and backward
    run on torch's current stream; nothing crosses to the host.  reuse=True lets a backward that directly follows its forward
    skip the second sweep (same bits)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64:
        raise TypeError("trajectory_device: x must be a CUDA float64 tensor")
    cols = getattr(engine, "n_params", 0) or engine.N
    if tuple(x.shape) != (engine.K, cols):
        raise ValueError(f"trajectory_device: x must be ({engine.K},{cols})")
    if ops is None:
        raise ValueError("trajectory_device: at least one probe is needed")
    if not isinstance(ops, torch.Tensor):
        ops = torch.from_numpy(np.array(ops, dtype=np.complex128, copy=True))
    want = (engine.E, ops.shape[1] if ops.ndim == 4 else 0, engine.n, engine.m) if per_member else \
        (ops.shape[0] if ops.ndim == 3 else 0, engine.n, engine.m)
    if tuple(ops.shape) != want or not 1 <= ops.shape[-3] <= 16:
        raise ValueError(f"trajectory_device: ops must be {'(E, n_obs, n, m)' if per_member else '(n_obs, n, m)'} with "
                         f"E = {engine.E}, n = {engine.n}, m = {engine.m} and 1 <= n_obs <= 16")
    if x.device.type != "cuda":
        raise TypeError("trajectory_device: x must be a CUDA float64 tensor")
    ops = ops.detach().to(device=x.device, dtype=torch.complex128)
    return _TrajectoryDevice.apply(x, engine, ops, bool(per_member), bool(final), bool(reuse))
