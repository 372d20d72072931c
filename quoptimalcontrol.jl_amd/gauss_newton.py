"""Gauss-Newton / Levenberg-Marquardt on least-squares trajectory losses, over the host forms of the trajectory calls.

The loss is  L(x) = 1/2 sum_{k,j,s} r' W r  +  1/2 sum_k wf_k |X_{k,N} - Xf_target_k|^2  with r = y - y_target split into
(Re, Im) and W the real symmetric 2x2 block of the entry (scalar weights: W = w 1).  Its gradient is one observe_vjp with
ybar = W r, xbar_final = wf (X_N - Xf_target); its Gauss-Newton matrix J' W J is applied by GrapeEngine.observe_gnvp in one
trajectory pass ("fused"), or by observe_jvp -> weights -> observe_vjp ("composed": two passes and two (E, n_obs, N+1) arrays).
Tracking a population curve, fitting a measured transient, holding a state on a path are all of this form.
"""
import numpy as np

__all__ = ["apply_weights", "gn_operator", "fit_trajectory"]


def apply_weights(w, r, blocks=None):
    """W r for r (E, n_obs, N+1) complex: w of shape (n_obs, N+1) or (E, n_obs, N+1) is scalar; behind a leading axis of 3 it
    holds the planes rr, ri, ii.  blocks as in GrapeEngine.observe_gnvp: None infers it from the shape (an array of r's own
    shape is scalar weights per member -- at E = 3 that is also the shape of shared planes), True / False says it."""
    w = np.asarray(w, dtype=np.float64)
    shared, member = tuple(r.shape[1:]), tuple(r.shape)
    if blocks is not True and w.shape in (shared, member):
        return w * r
    if blocks is not False and w.shape in ((3,) + shared, (3,) + member):
        return (w[0] * r.real + w[1] * r.imag) + 1j * (w[1] * r.real + w[2] * r.imag)
    raise ValueError(f"w must be {shared} or {member}, or the three planes rr, ri, ii of either behind a leading axis of 3")


def gn_operator(engine, x, ops, w, wf, per_member=False, operator="fused", blocks=None):
    """v -> J' W J v at x (v and the result in x's shape and coordinates).  operator = "fused": one observe_gnvp per product;
    "composed": observe_jvp, the weights in NumPy, observe_vjp.  blocks: how w is read (GrapeEngine.observe_gnvp)."""
    if w is None and wf is None:
        raise ValueError("gn_operator: nothing to weight (w and wf are both None)")
    x = np.array(x, dtype=np.float64)
    probes = ops if w is not None else None                     # (probes without weights: nothing of theirs enters)
    pm = per_member and probes is not None
    if operator == "fused":
        return lambda v: engine.observe_gnvp(x, v, probes, w=w, wf=wf, per_member=pm, blocks=blocks)
    if operator != "composed":
        raise ValueError('gn_operator: operator must be "fused" or "composed"')

    def composed(v):
        yd, Xd = engine.observe_jvp(x, v, probes, per_member=pm, final=True)
        ybar = None if w is None else apply_weights(w, yd, blocks)
        xbar = None if wf is None else np.asarray(wf, dtype=np.float64)[:, None, None] * Xd
        return engine.observe_vjp(x, probes, ybar=ybar, xbar_final=xbar, per_member=pm)

    return composed


def _cg(apply, b, iters, rtol):
    """conjugate gradients on apply(p) = b from p = 0; stops at |residual| <= rtol |b| or on a direction of no curvature.
    Returns (p, apply(p)), the product accumulated from the iterations' own: no further application of the operator"""
    p, Ap, r = np.zeros_like(b), np.zeros_like(b), b.copy()
    d, rr = r.copy(), float(np.vdot(r, r))
    stop = rtol * rtol * rr
    for _ in range(iters):
        if rr <= stop:
            break
        Hd = apply(d)
        curv = float(np.vdot(d, Hd))
        if not curv > 0.0:
            break
        a = rr / curv
        p += a * d
        Ap += a * Hd
        r -= a * Hd
        rr_new = float(np.vdot(r, r))
        d = r + (rr_new / rr) * d
        rr = rr_new
    return p, Ap


def fit_trajectory(engine, x0, ops, y_target=None, w=None, xf_target=None, wf=None, max_iter=20, cg_iter=20, lam0=1e-2,
                   operator="fused", per_member=False, cg_rtol=1e-10, g_tol=0.0, blocks=None, solver="host"):
    """Levenberg-Marquardt on L(x) above, from x0.  y_target (E, n_obs, N+1) complex with w (None: ones), and / or xf_target
    (E, n, m) with wf (None: ones).  Per iteration: the gradient from observe_vjp, the step p from cg_iter CG iterations on
    (J' W J + lam 1) p = -g, and the usual rule on the gain ratio rho = (L(x) - L(x + p)) / (model decrease): rho > 0 accepts
    the step (lam / 3 when rho > 0.75, lam * 2 when rho < 0.25), otherwise lam * 4 and the step is retried at the same x.
    operator: "fused" | "composed" (gn_operator), or a callable x -> (v -> J' W J v) of the caller's own.  blocks: how w is
    read (GrapeEngine.observe_gnvp).  One operator application per CG iteration, none besides.
    solver: "host" runs the CG loop above over the host forms; "device" leaves an iteration to GrapeEngine.gn_step -- one call
    at x for L, g, p and the model decrease (one sweep, one upload, the CG iterations on the device), one with cg_iter = 0 at
    x + p for L(x + p) -- under the same accept and lam rules.  It applies the fused operator; a callable operator is refused.
    Returns dict(x, loss, losses (L at x0 and at every accepted iterate), steps (the accepted p), lam, iterations, accepted)."""
    if y_target is None and xf_target is None:
        raise ValueError("fit_trajectory: nothing to fit (y_target and xf_target are both None)")
    x = np.array(x0, dtype=np.float64)
    if y_target is not None:
        y_target = np.asarray(y_target, dtype=np.complex128)
        w = np.ones(y_target.shape[1:]) if w is None else np.asarray(w, dtype=np.float64)
    else:
        w = None
    if xf_target is not None:
        xf_target = np.asarray(xf_target, dtype=np.complex128)
        wf = np.ones(xf_target.shape[0]) if wf is None else np.asarray(wf, dtype=np.float64)
    else:
        wf = None
    probes = ops if w is not None else None
    if solver == "device":
        if callable(operator):
            raise ValueError('fit_trajectory: solver="device" applies the library\'s own operator; a callable operator needs solver="host"')
        return _fit_on_device(engine, x, probes, y_target, w, xf_target, wf, max_iter, cg_iter, lam0, per_member and probes is not None,
                              cg_rtol, g_tol, blocks)
    if solver != "host":
        raise ValueError('fit_trajectory: solver must be "host" or "device"')

    def residuals(xx):
        """(L, ybar, xbar) at xx"""
        y, Xf = engine.observe(xx, probes, per_member=per_member and probes is not None, final=True)
        L, ybar, xbar = 0.0, None, None
        if w is not None:
            r = y - y_target
            ybar = apply_weights(w, r, blocks)
            L += 0.5 * float(np.sum(np.real(np.conj(r) * ybar)))
        if wf is not None:
            d = Xf - xf_target
            xbar = wf[:, None, None] * d
            L += 0.5 * float(np.sum(np.real(np.conj(d) * xbar)))
        return L, ybar, xbar

    make = operator if callable(operator) else (lambda xx: gn_operator(engine, xx, probes, w, wf, per_member, operator, blocks))
    lam = float(lam0)
    L, ybar, xbar = residuals(x)
    losses, steps, it = [L], [], 0
    for it in range(1, max_iter + 1):
        g = engine.observe_vjp(x, probes, ybar=ybar, xbar_final=xbar, per_member=per_member and probes is not None)
        if np.abs(g).max() <= g_tol:
            it -= 1
            break
        H = make(x)
        p, Ap = _cg(lambda v: H(v) + lam * v, -g, cg_iter, cg_rtol)
        # the decrease the quadratic model predicts, -g'p - p'Hp / 2 with H p = (H + lam) p - lam p from CG's own products
        model = -float(np.vdot(g, p)) - 0.5 * (float(np.vdot(p, Ap)) - lam * float(np.vdot(p, p)))
        L_new, yb_new, xb_new = residuals(x + p)
        rho = (L - L_new) / model if model > 0.0 else -1.0
        if rho > 0.0 and L_new < L:
            x, L, ybar, xbar = x + p, L_new, yb_new, xb_new
            losses.append(L)
            steps.append(p)
            lam = lam / 3.0 if rho > 0.75 else (lam * 2.0 if rho < 0.25 else lam)
        else:
            lam *= 4.0
    return dict(x=x, loss=L, losses=losses, steps=steps, lam=lam, iterations=it, accepted=len(steps))


def _fit_on_device(engine, x, probes, y_target, w, xf_target, wf, max_iter, cg_iter, lam0, per_member, cg_rtol, g_tol, blocks):
    """fit_trajectory's loop with GrapeEngine.gn_step in place of residuals / observe_vjp / _cg"""
    def step(xx, lam, iters):
        return engine.gn_step(xx, probes, y_target=y_target, w=w, xf_target=xf_target, wf=wf, lam=lam, cg_iter=iters,
                              cg_rtol=cg_rtol, per_member=per_member, blocks=blocks)

    lam = float(lam0)
    if max_iter < 1:
        L = step(x, lam, 0)["loss"]
        return dict(x=x, loss=L, losses=[L], steps=[], lam=lam, iterations=0, accepted=0)
    L, losses, steps, it = None, [], [], 0
    for it in range(1, max_iter + 1):
        s = step(x, lam, cg_iter)
        if L is None:                                             # (the first call's own loss: no call for L(x0) alone)
            L = s["loss"]
            losses.append(L)
        if s["g_inf"] <= g_tol:
            it -= 1
            break
        p, model = s["p"], s["predicted"]
        L_new = step(x + p, lam, 0)["loss"]
        rho = (L - L_new) / model if model > 0.0 else -1.0
        if rho > 0.0 and L_new < L:
            x, L = x + p, L_new
            losses.append(L)
            steps.append(p)
            lam = lam / 3.0 if rho > 0.75 else (lam * 2.0 if rho < 0.25 else lam)
        else:
            lam *= 4.0
    return dict(x=x, loss=L, losses=losses, steps=steps, lam=lam, iterations=it, accepted=len(steps))
