"""Plain NumPy / SciPy reference of grape_gn_step (include/grape_hip.h), shared by test_gn_step_host.py and the GPU tests.
Built on the repository's own references: observe_reference.states for the read-out, gnvp_reference.apply_weights for the
weight blocks, hvp_reference.vjp_of_propagators for the pull-back, the tangent recurrence of jvp_reference for the operator --
on propagators from scipy.linalg.expm (tests/rc_reference.py), formed ONCE per linearisation point.  No chunks, no scans, no
conjugate gradients: the step is numpy.linalg.solve on the dense matrix.

  L  = 1/2 sum r' W r + 1/2 sum_k wf_k |X_{k,N} - Xf_target_k|^2,  r = y - y_target          (gauss_newton.py's module text)
  g  = vjp(ybar = W r, xbar = wf (X_N - Xf_target))
  H  = J' W J, column by column from unit directions;  p* = -(H + lam 1)^-1 g
"""
import numpy as np

import gnvp_reference as gr
import observe_reference as obr
from hvp_reference import vjp_of_propagators
from rc_reference import propagators
from vjp_reference import probes_per_member


class GnProblem:
    """the loss at one pulse: L, g (K, N), and v -> J' W J v on the stored propagators"""

    def __init__(self, A, B, Xi, x, T, O=None, y_target=None, w=None, xf_target=None, wf=None, per_member=False, variant=0,
                 blocks=None, P=None):
        self.A, self.B, self.Xi = (np.asarray(v, complex) for v in (A, B, Xi))
        self.x = np.asarray(x, float)
        self.K, self.N = self.x.shape
        self.E = self.A.shape[0]
        self.dt = T / self.N
        self.blocks = blocks
        self.P = propagators(self.A, self.B, self.x, T, variant) if P is None else P       # (P: the caller has them already)
        self.X = obr.states(self.P, self.Xi, False)               # (N+1, E, n, m)
        self.has_y, self.has_x = y_target is not None, xf_target is not None
        if not (self.has_y or self.has_x):
            raise ValueError("nothing to fit")
        self.Ok = probes_per_member(O, self.E, per_member) if self.has_y else None
        self.L, ybar, xbar = 0.0, None, None
        if self.has_y:
            y = np.einsum("kjab,skab->kjs", self.Ok.conj(), self.X)
            self.w = np.ones(y.shape[1:]) if w is None else np.asarray(w, float)
            r = y - np.asarray(y_target, complex)
            ybar = gr.apply_weights(self.w, r, blocks)
            self.L += 0.5 * float(np.sum(np.real(np.conj(r) * ybar)))
        if self.has_x:
            self.wf = np.ones(self.E) if wf is None else np.asarray(wf, float)
            d = self.X[-1] - np.asarray(xf_target, complex)
            xbar = self.wf[:, None, None] * d
            self.L += 0.5 * float(np.sum(np.real(np.conj(d) * xbar)))
        self.g = vjp_of_propagators(self.P, self.B, self.Xi, self.dt, self.Ok, ybar, xbar)

    def tangents(self, v):
        """D (N+1, E, n, m): jvp_reference.tangent_states_recurrence on the stored propagators and states"""
        D = [np.zeros_like(self.X[0])]
        for s in range(self.N):
            V = (-1j * self.dt) * np.einsum("c,kcab->kab", v[:, s], self.B)
            D.append(self.P[s] @ D[-1] + V @ self.X[s + 1])
        return np.array(D)

    def apply(self, v):
        """J' W J v: gnvp_reference.gnvp_ref without forming the propagators again"""
        D = self.tangents(np.asarray(v, float).reshape(self.K, self.N))
        ybar = gr.apply_weights(self.w, np.einsum("kjab,skab->kjs", self.Ok.conj(), D), self.blocks) if self.has_y else None
        xbar = self.wf[:, None, None] * D[-1] if self.has_x else None
        return vjp_of_propagators(self.P, self.B, self.Xi, self.dt, self.Ok, ybar, xbar)

    def dense(self):
        """H (Q, Q), index c N + t, column by column"""
        Q = self.K * self.N
        H = np.empty((Q, Q))
        for q in range(Q):
            e = np.zeros(Q)
            e[q] = 1.0
            H[:, q] = self.apply(e).reshape(-1)
        return H

    def norm_estimate(self, rng, iterations=20):
        """|H|_2 by power iteration from a random start (never above the true norm)"""
        v = rng.standard_normal((self.K, self.N))
        est = 0.0
        for _ in range(iterations):
            v /= np.linalg.norm(v)
            Hv = self.apply(v)
            est = float(np.linalg.norm(Hv))
            v = Hv
        return est


def gn_step_ref(problem, lam, H=None):
    """p* (K, N) = -(H + lam 1)^-1 g by numpy.linalg.solve on the dense H (built here unless given)"""
    H = problem.dense() if H is None else H
    Q = H.shape[0]
    return -np.linalg.solve(H + lam * np.eye(Q), problem.g.reshape(-1)).reshape(problem.K, problem.N)


def predicted_ref(g, p, Hp):
    """the decrease the quadratic model predicts, -g'p - p'Hp / 2"""
    return -float(np.sum(g * p)) - 0.5 * float(np.sum(p * Hp))


__all__ = ["GnProblem", "gn_step_ref", "predicted_ref"]
