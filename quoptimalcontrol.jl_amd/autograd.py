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
        ctx.engine, ctx.ops, ctx.per_member = engine, ops, per_member
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


def trajectory(engine, x, ops, per_member=False, final=True):
    """y (E, n_obs, N+1) complex128 and -- final=True -- X_final (E, n, m) of the pulse x, a CPU float64 tensor of the shape
    engine.eval takes, differentiable with respect to x.  ops as in GrapeEngine.observe (at least one probe); it is not
    differentiated.  Returns (y, X_final), or y alone with final=False."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device.type != "cpu":
        raise TypeError("trajectory: x must be a CPU float64 tensor")
    if ops is None:
        raise ValueError("trajectory: at least one probe is needed (GrapeEngine.observe(final=True) gives X_final alone)")
    ops = np.array(ops.detach().numpy() if isinstance(ops, torch.Tensor) else ops, dtype=np.complex128, copy=True)
    return _Trajectory.apply(x, engine, ops, bool(per_member), bool(final))
