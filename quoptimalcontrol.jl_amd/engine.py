"""ctypes binding of libgrape_hip.so (include/grape_hip.h) -- the only compute path.

There is deliberately no CPU fallback here: if the HIP library is missing or no gfx950
device is visible, construction raises GrapeError.  (The CPU restatement under oracle/ is
test infrastructure and is never imported from this package.)

This is the Python twin of julia/GrapeHIP.jl: both pack the operators once
(what init_ensemble produces, /root/reference/src/tools.jl:42-53), create a context
(init_GRAPE, src/grape_tools.jl:4-16) and then forward every call of the (F, G, x) closure
(src/solve.jl:164-196) to grape_eval.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SYS_TYPE_CODES = {"UnitaryGate": 0, "StateTransfer": 1, "CoherenceTransfer": 2}
FLAG_KEEP_COSTATES = 1
FLAG_TIME_KERNELS = 2
FLAG_PHASE_STAMPS = 4
FLAG_FORCE_GENERAL = 8
FLAG_MEMBER_RESULTS = 16
FLAG_FORCE_COLLECTIVE = 32
FLAG_TIME_SAMPLED = 64
FLAG_GROUP_PEER_SUM = 128
MAX_DEVICES = 8
MAX_JVP_DIRECTIONS = 8                                     # GRAPE_MAX_JVP_DIRECTIONS
MAX_VJP_COTANGENTS = 8                                     # GRAPE_MAX_VJP_COTANGENTS
ABI_VERSION = 8

STATUS = {0: "GRAPE_OK", -1: "GRAPE_ERR_INVALID_ARG", -2: "GRAPE_ERR_UNSUPPORTED",
          -3: "GRAPE_ERR_NO_DEVICE", -4: "GRAPE_ERR_HIP", -5: "GRAPE_ERR_NOT_READY",
          -6: "GRAPE_ERR_ALLOC", -7: "GRAPE_ERR_TIMEOUT", -8: "GRAPE_ERR_COMM"}

TRAJ_DERIVATIVE_CODES = {"first_order": 0, "exact": 1}    # grape_traj_derivative

# every symbol include/grape_hip.h declares
EXPORTS = ["grape_abi_version", "grape_create", "grape_destroy", "grape_set_operators", "grape_set_penalties",
           "grape_set_running_cost",
           "grape_set_basis", "grape_get_controls", "grape_set_bounds", "grape_set_risk", "grape_get_risk_weights",
           "grape_comm_unique_id", "grape_comm_attach", "grape_ipc_export", "grape_ipc_attach",
           "grape_eval", "grape_eval_device", "grape_eval_batch", "grape_eval_batch_device", "grape_eval_fom", "grape_eval_observables",
           "grape_eval_vjp", "grape_eval_observables_device", "grape_eval_vjp_device", "grape_eval_jvp", "grape_eval_jvp_device",
           "grape_eval_jvp_multi", "grape_eval_jvp_multi_device", "grape_eval_hvp", "grape_eval_hvp_device",
           "grape_eval_gnvp", "grape_eval_gnvp_device", "grape_gn_step",
           "grape_eval_vjp_multi", "grape_eval_vjp_multi_device",
           "grape_eval_observables_mean", "grape_eval_vjp_mean", "grape_eval_jvp_mean",
           "grape_set_trajectory_derivative", "grape_set_running_cost_derivative",
           "grape_lbfgs", "grape_lbfgs_get_trace",
           "grape_get_member_results", "grape_get_trajectory",
           "grape_get_kernel_time", "grape_get_kernel_samples", "grape_get_kernel_names", "grape_get_group_timing", "grape_get_phase_stamps",
           "grape_get_info",
           "grape_last_error"]


class GrapeError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS.get(status, status)}: {message}")
        self.status = status


class GrapeConfig(C.Structure):
    _fields_ = [("sys_type", C.c_int32), ("variant", C.c_int32), ("n", C.c_int32),
                ("n_controls", C.c_int32), ("n_slices", C.c_int32), ("n_ensemble", C.c_int32),
                ("duration", C.c_double), ("device", C.c_int32), ("flags", C.c_int32),
                ("slices_per_lane", C.c_int32), ("waves_per_member", C.c_int32),
                ("expm_squarings", C.c_int32), ("max_batch", C.c_int32),
                ("n_state_cols", C.c_int32), ("n_devices", C.c_int32), ("device_ids", C.c_int32 * MAX_DEVICES),
                ("gradient", C.c_int32), ("objective", C.c_int32)]


class GrapeInfo(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("compute_units", C.c_int32),
                ("slices_per_lane", C.c_int32), ("waves_per_member", C.c_int32),
                ("expm_squarings", C.c_int32), ("kernel_family", C.c_int32), ("unitary_flow", C.c_int32),
                ("expm_theta", C.c_double), ("workspace_bytes", C.c_uint64), ("arch", C.c_char * 32),
                ("n_devices", C.c_int32), ("comm_size", C.c_int32), ("comm_rank", C.c_int32),
                ("members_first_device", C.c_int32), ("lane_pair", C.c_int32),
                ("states_stored", C.c_int32), ("rank_one_chain", C.c_int32),
                ("sparse_controls", C.c_int32), ("fused_forward", C.c_int32),
                ("time_chunks", C.c_int32), ("hoisted_controls", C.c_int32),
                ("expm_action", C.c_int32), ("prop_chain", C.c_int32), ("member_chunk", C.c_int32), ("pair_antiherm", C.c_int32),
                ("workspace_budget_bytes", C.c_uint64), ("scaled_controls", C.c_int32), ("propagator_blocks", C.c_int32)]


class GrapeLbfgsOptions(C.Structure):
    _fields_ = [("memory", C.c_int32), ("max_iterations", C.c_int32), ("g_tol", C.c_double), ("f_tol", C.c_double),
                ("max_linesearch", C.c_int32), ("probes", C.c_int32), ("line_search", C.c_int32), ("reserved", C.c_int32)]


class GrapeLbfgsResult(C.Structure):
    _fields_ = [("minimum", C.c_double), ("g_norm", C.c_double), ("seconds", C.c_double), ("iterations", C.c_int32),
                ("evaluations", C.c_int32), ("status", C.c_int32), ("probes", C.c_int32),
                ("line_search", C.c_int32), ("ladder_fallbacks", C.c_int32)]


class GrapeGnOptions(C.Structure):
    _fields_ = [("lambda", C.c_double), ("cg_rtol", C.c_double), ("cg_max_iter", C.c_int32), ("reserved", C.c_int32)]


class GrapeGnResult(C.Structure):
    _fields_ = [("loss", C.c_double), ("g_norm", C.c_double), ("g_inf", C.c_double), ("residual", C.c_double),
                ("p_norm", C.c_double), ("predicted", C.c_double), ("cg_iterations", C.c_int32), ("status", C.c_int32)]


class GrapeCommId(C.Structure):
    _fields_ = [("bytes", C.c_char * 128)]


def library_path():
    """libgrape_hip.so next to this file; GRAPE_HIP_LIB points diagnostics (tools/ablate.sh) at another build."""
    return os.environ.get("GRAPE_HIP_LIB") or os.path.join(_HERE, "libgrape_hip.so")


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of csrc/ into libgrape_hip.so (in-tree)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return library_path()


def load_library():
    """dlopen libgrape_hip.so and declare the prototypes of include/grape_hip.h."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        try:                                   # a fresh checkout: build in-tree once (hipcc, gfx950)
            build_library()
        except Exception as exc:               # no hipcc / build failure: fail loudly, no fallback
            raise GrapeError(-3, f"{path} is not built and building it failed: {exc}") from exc
    L = C.CDLL(path)
    vp, dp, i32 = C.c_void_p, C.POINTER(C.c_double), C.c_int32
    L.grape_abi_version.restype = C.c_int
    L.grape_create.argtypes = [C.POINTER(GrapeConfig), C.POINTER(vp)]
    L.grape_destroy.argtypes = [vp]
    L.grape_set_operators.argtypes = [vp] * 6
    L.grape_set_penalties.argtypes = [vp, vp, vp]
    L.grape_set_running_cost.argtypes = [vp, i32, vp, vp]
    L.grape_set_basis.argtypes = [vp, i32, i32, vp, vp]
    L.grape_get_controls.argtypes = [vp, vp, vp]
    L.grape_set_bounds.argtypes = [vp, vp, vp]
    L.grape_set_risk.argtypes = [vp, C.c_double]
    L.grape_get_risk_weights.argtypes = [vp, vp]
    L.grape_comm_unique_id.argtypes = [C.POINTER(GrapeCommId)]
    L.grape_comm_attach.argtypes = [vp, C.POINTER(GrapeCommId), i32, i32]
    L.grape_ipc_export.argtypes = [vp, i32, vp]
    L.grape_ipc_attach.argtypes = [vp, vp, i32, i32]
    L.grape_eval.argtypes = [vp, vp, dp, vp]
    L.grape_eval_device.argtypes = [vp, vp, vp, vp]
    L.grape_eval_batch.argtypes = [vp, i32, vp, vp, vp]
    L.grape_eval_batch_device.argtypes = [vp, i32, vp, vp, vp]
    L.grape_eval_fom.argtypes = [vp, i32, vp, vp, vp]
    L.grape_eval_observables.argtypes = [vp, vp, i32, i32, vp, vp, vp, dp]
    L.grape_eval_vjp.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
    L.grape_eval_observables_device.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.grape_eval_vjp_device.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.grape_eval_jvp.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    L.grape_eval_jvp_device.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.grape_eval_vjp_multi.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.grape_eval_vjp_multi_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.grape_eval_jvp_multi.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp]
    L.grape_eval_jvp_multi_device.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp, vp]
    L.grape_eval_hvp.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.grape_eval_hvp_device.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.grape_eval_gnvp.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp]
    L.grape_eval_gnvp_device.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp]
    L.grape_gn_step.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, C.POINTER(GrapeGnOptions), vp, vp, C.POINTER(GrapeGnResult)]
    L.grape_eval_observables_mean.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, dp]
    L.grape_eval_vjp_mean.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.grape_eval_jvp_mean.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.grape_set_trajectory_derivative.argtypes = [vp, i32]
    L.grape_set_running_cost_derivative.argtypes = [vp, i32]
    L.grape_lbfgs.argtypes = [vp, vp, C.POINTER(GrapeLbfgsOptions), vp, C.POINTER(GrapeLbfgsResult)]
    L.grape_get_member_results.argtypes = [vp, vp, vp]
    L.grape_get_trajectory.argtypes = [vp, i32, vp, vp, vp]
    L.grape_get_kernel_time.argtypes = [vp, dp, C.POINTER(C.c_int64), i32]
    L.grape_get_kernel_samples.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.grape_get_kernel_names.argtypes = [vp, C.c_char_p, C.c_int32]
    L.grape_lbfgs_get_trace.argtypes = [vp, vp, vp, C.c_int32, C.POINTER(C.c_int32)]
    L.grape_get_group_timing.argtypes = [vp, vp, i32]
    L.grape_get_phase_stamps.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.grape_get_info.argtypes = [vp, C.POINTER(GrapeInfo)]
    L.grape_last_error.argtypes = [vp]
    L.grape_last_error.restype = C.c_char_p
    for name in EXPORTS:
        if name not in ("grape_last_error",):
            getattr(L, name).restype = C.c_int
    _LIB = L
    return L


def _cm(M):
    """[..., i, j] complex -> contiguous buffer with each matrix column-major (Julia layout)."""
    return np.ascontiguousarray(np.swapaxes(np.asarray(M, dtype=np.complex128), -1, -2))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def jacobian_columns(size, columns=None):
    """The flat indices of x (row-major over (K, cols)) whose Jacobian columns trajectory_jacobian returns, in the caller's
    order: all `size` of them for None; negative indices count from the end; out of range or repeated ones are refused."""
    if columns is None:
        return list(range(int(size)))
    out = []
    for c in columns:
        i = int(c)
        if i != c or not -size <= i < size:
            raise ValueError(f"trajectory_jacobian: column {c!r} is not an index into the {size} entries of x")
        out.append(i % size)
    if len(set(out)) != len(out):
        raise ValueError("trajectory_jacobian: a column is listed twice")
    if not out:
        raise ValueError("trajectory_jacobian: no column is listed")
    return out


def jacobian_blocks(columns, block=MAX_JVP_DIRECTIONS):
    """`columns` in consecutive blocks of at most `block`: the directions of one grape_eval_jvp_multi_device call each."""
    return [list(columns[i:i + block]) for i in range(0, len(columns), block)]


class _CountingLib:
    """The library as an engine sees it: every function fetched through it that evaluates or changes a setting -- everything
    but the read-only accessors -- bumps GrapeEngine.calls first."""

    def __init__(self, lib, engine):
        self.__dict__["_lib"], self.__dict__["_engine"] = lib, engine

    def __getattr__(self, name):
        if not (name.startswith("grape_get_") and name != "grape_get_controls") and name not in ("grape_last_error", "grape_lbfgs_get_trace"):
            self._engine.calls += 1
        return getattr(self._lib, name)


class GrapeEngine:
    """One context = one device + one shard of the ensemble.

    A (E,n,n), B (E,K,n,n), Xi/Xt (E,n,n), wts (E,) -- natural numpy matrices A[k][i,j].
    eval(x) -> (F, G) with x, G of shape (K, N) (x[j, i] as in the reference)."""

    n_params = 0                               # M of set_basis (parameter mode); 0: slice mode
    bounds = None                              # (lo, hi) of set_bounds while some control is bounded
    calls = 0                                  # library calls that evaluate or change a setting, so far: two equal readings
                                               # mean that nothing has touched the context in between (autograd's reuse)

    def __init__(self, sys_type, A, B, Xi, Xt, wts, T, n_slices, variant=0, device=-1, flags=0,
                 slices_per_lane=0, waves_per_member=0, expm_squarings=-1, member_results=False, max_batch=1,
                 devices=None, force_collective=False, gradient="reference", objective="fom"):
        """devices: list of HIP ordinals -> the library shards the ensemble over them itself
        (grape_config.n_devices / device_ids) and all-reduces [G, F] with RCCL once per evaluation.
        gradient: "reference" (the first-order grad_func!) or "exact" (derivative of the objective, 2 <= n <= 64);
        objective: "fom" (fom_func) or "c1" (the ADGRAPE functional C1(Xt, U Xi [U']); needs gradient="exact")."""
        self._h = None
        self._lib = _CountingLib(load_library(), self)
        A = np.asarray(A, dtype=np.complex128)
        B = np.asarray(B, dtype=np.complex128)
        if A.ndim != 3 or B.ndim != 4 or A.shape[1] != A.shape[2]:
            raise ValueError("A must be (E,n,n) and B (E,K,n,n)")
        E, n = A.shape[0], A.shape[1]
        K = B.shape[1]
        Xi = np.asarray(Xi, dtype=np.complex128)
        Xt = np.asarray(Xt, dtype=np.complex128)
        if Xi.ndim != 3 or Xi.shape[:2] != (E, n) or Xt.shape != Xi.shape or not 1 <= Xi.shape[2] <= n or B.shape != (E, K, n, n):
            raise ValueError("operator shapes disagree (B (E,K,n,n); Xi, Xt (E,n,m) with 1 <= m <= n)")
        m = Xi.shape[2]
        wts = np.ascontiguousarray(wts, dtype=np.float64)
        if wts.shape != (E,):
            raise ValueError("wts must have one weight per member")
        if member_results:
            flags |= FLAG_MEMBER_RESULTS
        if force_collective:
            flags |= FLAG_FORCE_COLLECTIVE
        devices = list(devices) if devices is not None else []
        if len(devices) > MAX_DEVICES:
            raise ValueError(f"at most {MAX_DEVICES} devices")
        code = SYS_TYPE_CODES[sys_type] if isinstance(sys_type, str) else int(sys_type)
        self.sys_type, self.n, self.K, self.N, self.E, self.T = sys_type, n, K, int(n_slices), E, float(T)
        self.m = m
        ids = (C.c_int32 * MAX_DEVICES)(*(devices + [0] * (MAX_DEVICES - len(devices))))
        if len(devices) == 1:
            device = devices[0]
        cfg = GrapeConfig(code, int(variant), n, K, int(n_slices), E, float(T), int(device), int(flags),
                          int(slices_per_lane), int(waves_per_member), int(expm_squarings), int(max_batch),
                          0 if m == n else m, len(devices) if len(devices) > 1 else 0, ids,
                          {"reference": 0, "exact": 1}[gradient], {"fom": 0, "c1": 1}[objective])
        self.max_batch = max(1, int(max_batch))
        self._traj_derivative = "first_order"
        self._rc_derivative = "first_order"
        h = C.c_void_p()
        rc = self._lib.grape_create(C.byref(cfg), C.byref(h))
        if rc:
            raise GrapeError(rc, self._lib.grape_last_error(None).decode())
        self._h = h
        self._F = C.c_double()
        self._check(self._lib.grape_set_operators(h, _p(_cm(A)), _p(_cm(B)), _p(_cm(Xi)), _p(_cm(Xt)),
                                                  _p(wts)))

    def set_operators(self, A, B, Xi, Xt, wts):
        """grape_set_operators again on the same context (same shapes): new members' operators, new states."""
        A, B = np.asarray(A, np.complex128), np.asarray(B, np.complex128)
        Xi, Xt = np.asarray(Xi, np.complex128), np.asarray(Xt, np.complex128)
        wts = np.ascontiguousarray(wts, dtype=np.float64)
        if A.shape != (self.E, self.n, self.n) or B.shape != (self.E, self.K, self.n, self.n) or \
                Xi.shape != (self.E, self.n, self.m) or Xt.shape != Xi.shape or wts.shape != (self.E,):
            raise ValueError("operator shapes must match the context")
        self._check(self._lib.grape_set_operators(self._h, _p(_cm(A)), _p(_cm(B)), _p(_cm(Xi)), _p(_cm(Xt)), _p(wts)))

    def set_penalties(self, amp=None, var=None):
        """grape_set_penalties: control-amplitude (C3) and control-variation (C4) weights, src/cost_functions.jl:29-39.
        Each of amp, var is None (term off), a scalar (every control) or a length-K vector of weights >= 0.  From now on
        every evaluation of this context returns F + sum_c amp_c sum_t x[c,t]^2 + sum_c var_c sum_t (x[c,t+1]-x[c,t])^2
        and its gradient (once per control array, not scaled by the ensemble weights); amp = var = None clears them."""
        def vec(w):
            if w is None:
                return None
            w = np.asarray(w, dtype=np.float64)
            w = np.full(self.K, float(w)) if w.ndim == 0 else np.ascontiguousarray(w)
            if w.shape != (self.K,):
                raise ValueError(f"penalty weights must be a scalar or have {self.K} entries")
            return w
        a, v = vec(amp), vec(var)
        self._check(self._lib.grape_set_penalties(self._h, _p(a), _p(v)))

    def set_running_cost(self, R, rho=None):
        """grape_set_running_cost: running costs on the intermediate states (the reference's C5 / C6 / C7,
        src/cost_functions.jl:44-61).  R: probe matrices (n_terms, E, n, m) or anything that broadcasts to it -- (n, m): one
        term, the same for every member; (E, n, m): one term per member; (n_terms, 1, n, m): shared by the members; at most 4
        terms.  rho: slice weights (n_terms, N), or (N,) / a scalar for every term; rho[j, s-1] weights the state after s
        slices.  From now on every evaluation returns F + sum_k w_k sum_j sum_s rho[j, s-1] |tr(R_kj' X_ks)|^2 and its
        gradient -- first order in dt, or exact after set_running_cost_derivative("exact") (include/grape_hip.h).  R=None
        switches the term off.  n = 2..4, UnitaryGate-type states, single-device contexts (gradient="exact" ones in the
        exact mode only); member_results() stays without it."""
        if R is None:
            self._check(self._lib.grape_set_running_cost(self._h, 0, None, None))
            return
        if rho is None:
            raise ValueError("set_running_cost: rho is needed with R")
        R = np.asarray(R, dtype=np.complex128)
        rho = np.asarray(rho, dtype=np.float64)
        if R.ndim < 2 or R.ndim > 4 or rho.ndim > 2:
            raise ValueError("set_running_cost: R must broadcast to (n_terms, E, n, m) and rho to (n_terms, N)")
        J = R.shape[0] if R.ndim == 4 else (rho.shape[0] if rho.ndim == 2 else 1)
        if not 1 <= J <= 4:
            raise ValueError("set_running_cost: 1 to 4 terms")
        try:
            Rf = np.broadcast_to(R, (J, self.E, self.n, self.m))
            rf = np.broadcast_to(rho, (J, self.N))
        except ValueError:
            raise ValueError(f"set_running_cost: R must broadcast to ({J}, {self.E}, {self.n}, {self.m}) and rho to "
                             f"({J}, {self.N})") from None
        rf = np.ascontiguousarray(rf)
        self._check(self._lib.grape_set_running_cost(self._h, J, _p(_cm(Rf)), _p(rf)))

    def set_basis(self, phi, x0=None):
        """grape_set_basis: restrict the pulse to x[c,t] = x0[c,t] + sum_m theta[c,m] phi[t,m] -- "parameter mode".
        phi: (N, M) (one basis for every control) or (K, N, M) (one per control), 1 <= M <= N; x0: (K, N) or None (0).
        From now on eval, eval_batch, fom, lbfgs and the device-pointer forms take theta (K, M) where they took x and
        return the gradient with respect to theta (K, M); F is that of the physical pulse, penalties included.
        member_results() and trajectory() stay in slice space.  phi=None switches the basis off again."""
        if phi is None:
            self._check(self._lib.grape_set_basis(self._h, 0, 1, None, None))
            self.n_params = 0
            return
        phi = np.asarray(phi, dtype=np.float64)
        if phi.ndim == 2 and phi.shape[0] == self.N:
            pf, nb = np.ascontiguousarray(phi.T), 1                          # [m][t]
        elif phi.ndim == 3 and phi.shape[:2] == (self.K, self.N):
            pf, nb = np.ascontiguousarray(np.swapaxes(phi, 1, 2)), self.K    # [c][m][t]
        else:
            raise ValueError(f"phi must be ({self.N}, M) or ({self.K}, {self.N}, M)")
        M = phi.shape[-1]
        xf = None
        if x0 is not None:
            x0 = np.asarray(x0, dtype=np.float64)
            if x0.shape != (self.K, self.N):
                raise ValueError(f"x0 must be ({self.K},{self.N})")
            xf = np.ascontiguousarray(x0.T)
        self._check(self._lib.grape_set_basis(self._h, M, nb, _p(pf), _p(xf)))
        self.n_params = M

    def set_bounds(self, lo, hi=None):
        """grape_set_bounds: smooth amplitude bounds.  lo, hi: scalars (every control) or length-K vectors with finite
        lo < hi, or lo = -inf with hi = +inf for a control that stays free.  From now on eval, eval_batch, fom, lbfgs and
        the device-pointer forms take the RAW pulse u (theta with a basis) and evaluate the physical pulse
        x = mid + half tanh((u - mid) / half), which lies strictly inside (lo, hi); the returned gradient is that with
        respect to u (theta), F that of the physical pulse, penalties and running costs evaluated on it.  controls(u)
        returns the physical pulse.  The gradient vanishes where the pulse saturates: start inside (bounds.bounds_start).
        set_bounds(None) switches the bounds off; bounds that leave every control free do the same.  A refused call
        (ValueError here, GrapeError from the library) leaves the previous bounds in force."""
        from .bounds import bounds_vectors
        lo, hi = bounds_vectors(lo, hi, self.K)
        self._check(self._lib.grape_set_bounds(self._h, _p(lo), _p(hi)))
        self.bounds = None if lo is None or not np.isfinite(lo).any() else (lo, hi)

    def set_risk(self, beta):
        """grape_set_risk: the soft worst case over the ensemble in place of its weighted mean.  With W = sum_k w_k every
        evaluation returns F_beta = (W / beta) log((1 / W) sum_k w_k exp(beta F_k)) and G_beta = sum_k p_k g_k,
        p_k = W w_k exp(beta F_k) / sum_j w_j exp(beta F_j): beta -> 0 is the mean, beta -> +inf W max_k F_k, beta -> -inf
        W min_k F_k.  Penalties are added behind it, a basis and bounds stay around it; member_results() and the
        member_F of fom() stay the unweighted F_k.  beta = 0 (or None) switches it off.  Single-device contexts without
        a running cost (include/grape_hip.h)."""
        self._check(self._lib.grape_set_risk(self._h, 0.0 if beta is None else float(beta)))

    def set_trajectory_derivative(self, mode):
        """grape_set_trajectory_derivative: "first_order" (the default: dP_t/dx[c,t] taken as (-i dt B_c) P_t) or "exact" --
        observe_vjp, observe_jvp, their device forms and the reuse forms then differentiate the sweep's own expm evaluation
        per slice (the Frechet derivative, exact to the rounding of the propagators): what torch.autograd.gradcheck on
        autograd.trajectory and a quasi-Newton solve on a custom loss need.  The contexts observe_vjp serves; a refused call
        (ValueError here, GrapeError from the library) leaves the previous mode in force.  The running cost's own
        gradient follows set_running_cost_derivative."""
        if mode not in TRAJ_DERIVATIVE_CODES:
            raise ValueError(f"mode must be one of {sorted(TRAJ_DERIVATIVE_CODES)}")
        self._check(self._lib.grape_set_trajectory_derivative(self._h, TRAJ_DERIVATIVE_CODES[mode]))
        self._traj_derivative = mode

    @property
    def trajectory_derivative(self):
        """the mode set_trajectory_derivative left in force: "first_order" or "exact" """
        return self._traj_derivative

    def set_running_cost_derivative(self, mode):
        """grape_set_running_cost_derivative: "first_order" (the default, the rule of set_running_cost) or "exact" -- the J part
        of every gradient (eval, eval_device, the batched forms, lbfgs) then differentiates the sweep's own expm evaluation per
        slice (the Frechet derivative, one per member and slice for all controls and terms); J itself keeps its bits.  Served
        where set_running_cost is, and on contexts created with gradient="exact" (either objective), which take a running
        cost in this mode only: set it BEFORE set_running_cost there, and switch the cost off before going back.  A refused
        call (ValueError here, GrapeError from the library) leaves the previous mode in force."""
        if mode not in TRAJ_DERIVATIVE_CODES:
            raise ValueError(f"mode must be one of {sorted(TRAJ_DERIVATIVE_CODES)}")
        self._check(self._lib.grape_set_running_cost_derivative(self._h, TRAJ_DERIVATIVE_CODES[mode]))
        self._rc_derivative = mode

    @property
    def running_cost_derivative(self):
        """the mode set_running_cost_derivative left in force: "first_order" or "exact" """
        return self._rc_derivative

    def risk_weights(self):
        """grape_get_risk_weights: p (E,) of the last evaluation under set_risk (array 0 of a batch); sum p = sum w."""
        p = np.empty(self.E)
        self._check(self._lib.grape_get_risk_weights(self._h, _p(p)))
        return p

    @property
    def _cols(self):
        """second dimension of the arrays the evaluation calls take and return: M in parameter mode, else N"""
        return self.n_params or self.N

    def controls(self, theta):
        """grape_get_controls: the physical pulse (K, N) of a parameter array (K, M), expanded on the device by the
        kernel the evaluations use.  Without a basis the parameters are the pulse -- saturated, if set_bounds is in force."""
        theta = np.asarray(theta, dtype=np.float64)
        if theta.shape != (self.K, self._cols):
            raise ValueError(f"theta must be ({self.K},{self._cols})")
        tf = np.ascontiguousarray(theta.T)
        x = np.empty((self.N, self.K))
        self._check(self._lib.grape_get_controls(self._h, _p(tf), _p(x)))
        return np.ascontiguousarray(x.T)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc:
            raise GrapeError(rc, self._lib.grape_last_error(self._h).decode())

    def close(self):
        if self._h is not None:
            self._lib.grape_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def info(self):
        inf = GrapeInfo()
        self._check(self._lib.grape_get_info(self._h, C.byref(inf)))
        return {f: (getattr(inf, f).decode() if f == "arch" else getattr(inf, f)) for f, _ in inf._fields_}

    # ------------------------------------------------------------------ one process per GPU
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL bootstrap token (rank 0 creates it, every rank passes it to comm_attach)."""
        lib = load_library()
        cid = GrapeCommId()
        rc = lib.grape_comm_unique_id(C.byref(cid))
        if rc:
            raise GrapeError(rc, lib.grape_last_error(None).decode())
        return bytes(bytearray(cid)[:128])

    def comm_attach(self, token, rank, n_ranks):
        """Join the communicator: from now on every eval()/eval_device() of this context (this rank's
        member shard) ends in the single all-reduce of [G, F] over the ranks, inside the library."""
        cid = GrapeCommId.from_buffer_copy(bytes(token))
        self._check(self._lib.grape_comm_attach(self._h, C.byref(cid), int(rank), int(n_ranks)))

    def ipc_export(self, n_ranks):
        """64 opaque bytes naming this rank's exchange mailbox (grape_ipc_export): all-gather them, then ipc_attach."""
        buf = C.create_string_buffer(64)
        self._check(self._lib.grape_ipc_export(self._h, int(n_ranks), buf))
        return buf.raw

    def ipc_attach(self, handles, rank, n_ranks):
        """handles: the n_ranks exported byte strings in rank order.  From now on every eval()/eval_device()/lbfgs() of this
        context ends in the mailbox all-reduce of [G, F] over the ranks (no RCCL)."""
        blob = b"".join(bytes(h) for h in handles)
        if len(blob) != 64 * int(n_ranks):
            raise ValueError("ipc_attach: need n_ranks handles of 64 bytes")
        self._check(self._lib.grape_ipc_attach(self._h, C.create_string_buffer(blob, len(blob)), int(rank), int(n_ranks)))

    # ------------------------------------------------------------------ evaluation
    def eval(self, x, want_F=True, want_G=True):
        """grape_eval: host x (K,N) -> (F, G); either may be skipped like Optim's only_fg!.  Parameter mode (set_basis):
        x is theta (K,M) and G its gradient (K,M) -- here and in eval_cm, bind_eval, eval_batch, fom and lbfgs."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        xf = np.ascontiguousarray(x.T)
        F = C.c_double()
        G = np.empty((self._cols, self.K)) if want_G else None
        self._check(self._lib.grape_eval(self._h, _p(xf), C.byref(F) if want_F else None, _p(G)))
        return (F.value if want_F else None), (np.ascontiguousarray(G.T) if want_G else None)

    def eval_cm(self, xf, G_out=None):
        """grape_eval on caller-owned buffers in the library's own layout, no copies: xf is x as (K,N) COLUMN-major
        memory, i.e. a C-contiguous float64 array of shape (N, K); G_out (same shape, or None to skip G) receives
        the gradient in that layout.  Returns F.  This is what a compiled caller (the Julia ccall) does per
        optimiser step; eval() is the convenience form with natural (K, N) arrays."""
        if xf.dtype != np.float64 or not xf.flags.c_contiguous or xf.shape != (self._cols, self.K):
            raise ValueError(f"xf must be a C-contiguous float64 array of shape ({self._cols},{self.K})")
        if G_out is not None and (G_out.dtype != np.float64 or not G_out.flags.c_contiguous or G_out.shape != xf.shape):
            raise ValueError("G_out must match xf")
        rc = self._lib.grape_eval(self._h, xf.ctypes.data, C.byref(self._F), G_out.ctypes.data if G_out is not None else None)
        if rc:
            self._check(rc)
        return self._F.value

    def bind_eval(self, xf, G_out):
        """Pre-bound grape_eval on fixed caller buffers (layout as eval_cm): returns a zero-argument callable that
        runs one evaluation and returns F.  The ctypes argument objects are built once, so a call costs what the
        foreign-function call itself costs -- the closest Python gets to the Julia `ccall` in julia/GrapeHIP.jl."""
        if xf.dtype != np.float64 or not xf.flags.c_contiguous or xf.shape != (self._cols, self.K):
            raise ValueError(f"xf must be a C-contiguous float64 array of shape ({self._cols},{self.K})")
        if G_out.dtype != np.float64 or not G_out.flags.c_contiguous or G_out.shape != xf.shape:
            raise ValueError("G_out must match xf")
        fn, h, px, pg, F = self._lib.grape_eval, self._h, C.c_void_p(xf.ctypes.data), C.c_void_p(G_out.ctypes.data), self._F
        pF = C.byref(F)
        check = self._check

        def call():
            self.calls += 1
            rc = fn(h, px, pF, pg)
            if rc:
                check(rc)
            return F.value
        call.buffers = (xf, G_out)              # keep them alive as long as the callable lives
        return call

    LBFGS_STATUS = {0: "g_tol reached", 1: "f_tol reached", 2: "max iterations", 3: "line search failed",
                    4: "zero step (Optim: x converged)"}

    LINE_SEARCH = {"hagerzhang": 0, "hz": 0, "optim": 1, "hagerzhang_strict": 1, "ladder": 2}

    def lbfgs(self, x0, memory=0, iterations=0, g_tol=-1.0, f_tol=0.0, max_linesearch=0, probes=0, line_search="hagerzhang"):
        """grape_lbfgs: device-resident L-BFGS from x0 (K,N) -> (x_min (K,N), result dict).  Optim LBFGS()
        defaults when the options are left at 0 / negative.  line_search: "hagerzhang" (Optim's line search, the
        initial step accepted when it satisfies the Wolfe conditions), "optim" (Hager-Zhang exactly as Optim runs it
        behind InitialStatic) or "ladder" (`probes` step lengths per batched launch; needs max_batch >= probes)."""
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.shape != (self.K, self._cols):
            raise ValueError(f"x0 must be ({self.K},{self._cols})")
        xf = np.ascontiguousarray(x0.T)
        out = np.empty_like(xf)
        opts = GrapeLbfgsOptions(int(memory), int(iterations), float(g_tol), float(f_tol), int(max_linesearch), int(probes),
                                 self.LINE_SEARCH[line_search] if isinstance(line_search, str) else int(line_search), 0)
        res = GrapeLbfgsResult()
        self._check(self._lib.grape_lbfgs(self._h, _p(xf), C.byref(opts), _p(out), C.byref(res)))
        info = {f: getattr(res, f) for f, _ in res._fields_}
        info["message"] = self.LBFGS_STATUS.get(res.status, "?")
        return np.ascontiguousarray(out.T), info

    def lbfgs_trace(self):
        """grape_lbfgs_get_trace: (alphas, evaluations) of the last lbfgs() run, one entry per iteration."""
        cnt = C.c_int32()
        self._check(self._lib.grape_lbfgs_get_trace(self._h, None, None, 0, C.byref(cnt)))
        al, ev = np.empty(cnt.value), np.empty(cnt.value, dtype=np.int32)
        self._check(self._lib.grape_lbfgs_get_trace(self._h, _p(al), _p(ev), cnt.value, C.byref(cnt)))
        return al, ev

    def eval_batch(self, X):
        """grape_eval_batch: X (n_x, K, N) control arrays -> (F (n_x,), G (n_x, K, N)); entry b equals
        eval(X[b]).  An extension for multi-start optimisation; needs max_batch >= n_x."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 3 or X.shape[1:] != (self.K, self._cols):
            raise ValueError(f"X must be (n_x, {self.K}, {self._cols})")
        n_x = X.shape[0]
        xf = np.ascontiguousarray(np.swapaxes(X, 1, 2))            # each (K,N) column-major
        F = np.empty(n_x)
        G = np.empty((n_x, self._cols, self.K))
        self._check(self._lib.grape_eval_batch(self._h, n_x, _p(xf), _p(F), _p(G)))
        return F, np.ascontiguousarray(np.swapaxes(G, 1, 2))

    def fom(self, x, members=False):
        """grape_eval_fom: the figure of merit WITHOUT the gradient (pw_evolve + fom_func / C1).  x (K,N) -> F, or
        (F, member_F (E,)) with members=True; x (B,K,N), B <= max_batch -> F (B,) and member_F (B,E).  F is what eval(x)
        returns as F (penalties included), member_F the members' unweighted F_k.  For n = 2..4 on one device a
        forward-only kernel does the work (no propagator is stored, no backward sweep); elsewhere the full evaluation
        runs and its F is returned bit for bit."""
        x = np.asarray(x, dtype=np.float64)
        single = x.ndim == 2
        if (x.shape if single else x.shape[1:]) != (self.K, self._cols) or x.ndim not in (2, 3):
            raise ValueError(f"x must be ({self.K},{self._cols}) or (n_x,{self.K},{self._cols})")
        n_x = 1 if single else x.shape[0]
        xf = np.ascontiguousarray(np.swapaxes(x, -1, -2))          # each (K,N) column-major
        F = np.empty(n_x)
        mF = np.empty((n_x, self.E)) if members else None
        self._check(self._lib.grape_eval_fom(self._h, n_x, _p(xf), _p(F), _p(mF)))
        if single:
            return (float(F[0]), mF[0]) if members else float(F[0])
        return (F, mF) if members else F

    def observe(self, x, ops, per_member=False, final=False, want_F=False):
        """grape_eval_observables: one evaluation of x (K,N) (theta / u with a basis / bounds in force) and, behind it, the
        expectation values y[k, j, s] = tr(O_kj' X_ks) of the probes along the trajectory, s = 0..N (X_k0 = Xi_k; the states
        of the physical pulse).  ops: (n_obs, n, m) probes shared by the members -- or one (n, m) matrix -- and with
        per_member=True (E, n_obs, n, m); at most 16 probes; None (with final=True) for the final states alone.
        Returns y (E, n_obs, N+1) complex128 -- then X_final (E, n, m) with final=True -- then F, bit for bit eval(x)'s,
        with want_F=True.  n = 2..4, single-device contexts (include/grape_hip.h)."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        n, m, E, N = self.n, self.m, self.E, self.N
        if ops is None:
            if not final:
                raise ValueError("observe: nothing asked for (ops=None needs final=True)")
            n_obs, Of, y = 0, None, None
        else:
            O = np.asarray(ops, dtype=np.complex128)
            if not per_member and O.ndim == 2:
                O = O[None]
            want = (E, O.shape[1] if O.ndim == 4 else 0, n, m) if per_member else (O.shape[0] if O.ndim == 3 else 0, n, m)
            if O.shape != want or not 1 <= O.shape[-3] <= 16:
                raise ValueError(f"observe: ops must be {'(E, n_obs, n, m)' if per_member else '(n_obs, n, m)'} with E = {E}, "
                                 f"n = {n}, m = {m} and 1 <= n_obs <= 16")
            n_obs = O.shape[-3]
            # column-major (n, m, [E,] n_obs): the probe index slowest, then the member
            Of = _cm(np.swapaxes(O, 0, 1) if per_member else O)
            y = np.empty((E, n_obs, N + 1), np.complex128)
        Xf = np.empty((E, m, n), np.complex128) if final else None
        F = C.c_double()
        xf = np.ascontiguousarray(x.T)
        self._check(self._lib.grape_eval_observables(self._h, _p(xf), n_obs, 1 if per_member else 0, _p(Of), _p(y), _p(Xf),
                                                     C.byref(F) if want_F else None))
        out = [y]
        if final:
            out.append(np.ascontiguousarray(np.swapaxes(Xf, -1, -2)))
        if want_F:
            out.append(F.value)
        return out[0] if len(out) == 1 else tuple(out)

    def observe_vjp(self, x, ops, ybar=None, xbar_final=None, per_member=False):
        """grape_eval_vjp: the vector-Jacobian product of observe() -- the gradient with respect to x (K,N) (theta / u with a
        basis / bounds in force) of any real loss l written on observe's returns, from its cotangents
        ybar (E, n_obs, N+1) = dl/dRe y + i dl/dIm y and xbar_final (E, n, m) likewise (what torch hands to backward); either
        may be None (zero), not both.  ops as in observe (None with xbar_final alone).  Returns G (K, cols), first order in
        dt like the running cost's gradient, without ensemble weights, penalties, running cost or risk: the gradient of the
        caller's loss alone, in the coordinates of x.  n = 2..4, UnitaryGate, single-device contexts (include/grape_hip.h)."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        n, m, E, N = self.n, self.m, self.E, self.N
        if ybar is None and xbar_final is None:
            raise ValueError("observe_vjp: nothing to pull back (ybar and xbar_final are both None)")
        if ops is None:
            if ybar is not None:
                raise ValueError("observe_vjp: ybar needs the probes it belongs to")
            n_obs, Of = 0, None
        else:
            O = np.asarray(ops, dtype=np.complex128)
            if not per_member and O.ndim == 2:
                O = O[None]
            want = (E, O.shape[1] if O.ndim == 4 else 0, n, m) if per_member else (O.shape[0] if O.ndim == 3 else 0, n, m)
            if O.shape != want or not 1 <= O.shape[-3] <= 16:
                raise ValueError(f"observe_vjp: ops must be {'(E, n_obs, n, m)' if per_member else '(n_obs, n, m)'} with "
                                 f"E = {E}, n = {n}, m = {m} and 1 <= n_obs <= 16")
            n_obs = O.shape[-3]
            Of = _cm(np.swapaxes(O, 0, 1) if per_member else O)
        yb = None
        if ybar is not None:
            yb = np.ascontiguousarray(ybar, dtype=np.complex128)
            if yb.shape != (E, n_obs, N + 1):
                raise ValueError(f"observe_vjp: ybar must be ({E},{n_obs},{N + 1})")
        else:
            n_obs, Of = 0, None                                   # (probes without cotangents: nothing of theirs to pull back)
        xb = None
        if xbar_final is not None:
            xb = np.asarray(xbar_final, dtype=np.complex128)
            if xb.shape != (E, n, m):
                raise ValueError(f"observe_vjp: xbar_final must be ({E},{n},{m})")
            xb = _cm(xb)
        G = np.empty((self._cols, self.K))
        xf = np.ascontiguousarray(x.T)
        self._check(self._lib.grape_eval_vjp(self._h, _p(xf), n_obs, 1 if per_member else 0, _p(Of), _p(yb), _p(xb), _p(G)))
        return np.ascontiguousarray(G.T)

    def observe_jvp(self, x, xdot, ops, per_member=False, final=False):
        """grape_eval_jvp: the Jacobian-vector product of observe() -- how its returns move to first order when x (K,N)
        (theta / u with a basis / bounds in force) moves along xdot, an array of x's shape and coordinates.  ops as in observe
        (None with final=True for the final states alone).  Returns ydot (E, n_obs, N+1) complex128 -- then Xdot_final
        (E, n, m) with final=True.  First order in dt, the exact transpose of observe_vjp: sum Re(conj(ybar) ydot) +
        sum Re(conj(xbar_final) Xdot_final) = sum(observe_vjp(x, ops, ybar, xbar_final) * xdot) to rounding.  n = 2..4,
        UnitaryGate, single-device contexts (include/grape_hip.h)."""
        x = np.asarray(x, dtype=np.float64)
        xd = np.asarray(xdot, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        if xd.shape != x.shape:
            raise ValueError(f"observe_jvp: xdot must be ({self.K},{self._cols}), the shape of x")
        n, m, E, N = self.n, self.m, self.E, self.N
        if ops is None:
            if not final:
                raise ValueError("observe_jvp: nothing asked for (ops=None needs final=True)")
            n_obs, Of, yd = 0, None, None
        else:
            O = np.asarray(ops, dtype=np.complex128)
            if not per_member and O.ndim == 2:
                O = O[None]
            want = (E, O.shape[1] if O.ndim == 4 else 0, n, m) if per_member else (O.shape[0] if O.ndim == 3 else 0, n, m)
            if O.shape != want or not 1 <= O.shape[-3] <= 16:
                raise ValueError(f"observe_jvp: ops must be {'(E, n_obs, n, m)' if per_member else '(n_obs, n, m)'} with "
                                 f"E = {E}, n = {n}, m = {m} and 1 <= n_obs <= 16")
            n_obs = O.shape[-3]
            Of = _cm(np.swapaxes(O, 0, 1) if per_member else O)
            yd = np.empty((E, n_obs, N + 1), np.complex128)
        Xf = np.empty((E, m, n), np.complex128) if final else None
        xf, xdf = np.ascontiguousarray(x.T), np.ascontiguousarray(xd.T)
        self._check(self._lib.grape_eval_jvp(self._h, _p(xf), _p(xdf), n_obs, 1 if per_member else 0, _p(Of), _p(yd), _p(Xf)))
        if final:
            return yd, np.ascontiguousarray(np.swapaxes(Xf, -1, -2))
        return yd

    def _mean_args(self, who, x, ops, per_member, v):
        """(xf, n_obs, Of, vf) of the *_mean forms: x column-major, the probes as the library reads them, the weights"""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        n_obs, O = self._jvp_probes(who, ops, per_member)
        Of = None if O is None else _cm(np.swapaxes(O, 0, 1) if per_member else O)
        vf = None
        if v is not None:
            vf = np.ascontiguousarray(v, dtype=np.float64)
            if vf.shape != (self.E,):
                raise ValueError(f"{who}: v must be ({self.E},)")
        return np.ascontiguousarray(x.T), n_obs, Of, vf

    def observe_mean(self, x, ops, v=None, per_member=False, final=False, want_F=False):
        """grape_eval_observables_mean: observe() with the member axis summed on the device, y_mean[j, s] = sum_k v_k y[k, j, s]
        and X_mean = sum_k v_k X_final[k].  v (E,): the weights of the sum; None: the ensemble weights wts (not the risk
        weights: pass risk_weights() for those).  x, ops, per_member, final, want_F as in observe.  Returns y_mean (n_obs, N+1)
        complex128 -- then X_mean (n, m) with final=True -- then F with want_F=True.  The summation order depends on E alone:
        equal bits call to call, chunked or not, and column j of a 16-probe call is the 1-probe call with probe j."""
        xf, n_obs, Of, vf = self._mean_args("observe_mean", x, ops, per_member, v)
        if Of is None and not final:
            raise ValueError("observe_mean: nothing asked for (ops=None needs final=True)")
        y = None if Of is None else np.empty((n_obs, self.N + 1), np.complex128)
        Xm = np.empty((self.m, self.n), np.complex128) if final else None
        F = C.c_double()
        self._check(self._lib.grape_eval_observables_mean(self._h, _p(xf), n_obs, 1 if per_member else 0, _p(Of), _p(vf), _p(y),
                                                          _p(Xm), C.byref(F) if want_F else None))
        out = [y]
        if final:
            out.append(np.ascontiguousarray(Xm.T))
        if want_F:
            out.append(F.value)
        return out[0] if len(out) == 1 else tuple(out)

    def observe_vjp_mean(self, x, ops, ybar_mean=None, xbar_mean=None, v=None, per_member=False):
        """grape_eval_vjp_mean: the vector-Jacobian product of observe_mean() -- the gradient with respect to x of any real loss
        written on its returns, from the cotangents ybar_mean (n_obs, N+1) and xbar_mean (n, m) (either may be None, not both).
        Bit for bit observe_vjp with ybar[k] = v_k * ybar_mean, xbar_final[k] = v_k * xbar_mean (component-wise products),
        which a kernel forms on the device.  Returns G (K, cols) in the coordinates of x."""
        xf, n_obs, Of, vf = self._mean_args("observe_vjp_mean", x, ops, per_member, v)
        if ybar_mean is None and xbar_mean is None:
            raise ValueError("observe_vjp_mean: nothing to pull back (ybar_mean and xbar_mean are both None)")
        yb = None
        if ybar_mean is not None:
            if Of is None:
                raise ValueError("observe_vjp_mean: ybar_mean needs the probes it belongs to")
            yb = np.ascontiguousarray(ybar_mean, dtype=np.complex128)
            if yb.shape != (n_obs, self.N + 1):
                raise ValueError(f"observe_vjp_mean: ybar_mean must be ({n_obs},{self.N + 1})")
        else:
            n_obs, Of = 0, None                                   # (probes without cotangents: nothing of theirs to pull back)
        xb = None
        if xbar_mean is not None:
            xb = np.asarray(xbar_mean, dtype=np.complex128)
            if xb.shape != (self.n, self.m):
                raise ValueError(f"observe_vjp_mean: xbar_mean must be ({self.n},{self.m})")
            xb = _cm(xb)
        G = np.empty((self._cols, self.K))
        self._check(self._lib.grape_eval_vjp_mean(self._h, _p(xf), n_obs, 1 if per_member else 0, _p(Of), _p(vf), _p(yb), _p(xb),
                                                  _p(G)))
        return np.ascontiguousarray(G.T)

    def observe_jvp_mean(self, x, xdot, ops, v=None, per_member=False, final=False):
        """grape_eval_jvp_mean: the Jacobian-vector product of observe_mean() along xdot (x's shape and coordinates): the sums
        sum_k v_k ydot[k] and sum_k v_k Xdot_final[k] of observe_jvp's returns, formed on the device in observe_mean's order.
        Returns ydot_mean (n_obs, N+1) -- then Xdot_mean (n, m) with final=True.  The transpose of observe_vjp_mean."""
        xf, n_obs, Of, vf = self._mean_args("observe_jvp_mean", x, ops, per_member, v)
        xd = np.asarray(xdot, dtype=np.float64)
        if xd.shape != (self.K, self._cols):
            raise ValueError(f"observe_jvp_mean: xdot must be ({self.K},{self._cols}), the shape of x")
        if Of is None and not final:
            raise ValueError("observe_jvp_mean: nothing asked for (ops=None needs final=True)")
        yd = None if Of is None else np.empty((n_obs, self.N + 1), np.complex128)
        Xm = np.empty((self.m, self.n), np.complex128) if final else None
        xdf = np.ascontiguousarray(xd.T)
        self._check(self._lib.grape_eval_jvp_mean(self._h, _p(xf), _p(xdf), n_obs, 1 if per_member else 0, _p(Of), _p(vf), _p(yd),
                                                  _p(Xm)))
        if final:
            return yd, np.ascontiguousarray(Xm.T)
        return yd

    def observe_hvp(self, x, xdot, ops, ybar=None, xbar_final=None, ybar_dot=None, xbar_final_dot=None, per_member=False):
        """grape_eval_hvp: the directional derivative of observe_vjp -- how G = observe_vjp(x, ops, ybar, xbar_final) moves to
        first order when x moves along xdot (x's shape and coordinates) and the cotangents move along ybar_dot (E, n_obs, N+1)
        / xbar_final_dot (E, n, m); either tangent may be None (zero).  With ybar = dl/dy of a loss l on observe's returns and
        ybar_dot = l'' applied to observe_jvp(x, xdot, ...) this is the Hessian-vector product of l.  Returns Gdot (K, cols),
        first order in dt under the rule of observe_vjp / observe_jvp, without ensemble weights, penalties, running cost or
        risk.  The contexts observe_vjp serves, without bounds and in the first-order trajectory derivative mode
        (include/grape_hip.h)."""
        x = np.asarray(x, dtype=np.float64)
        xd = np.asarray(xdot, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        if xd.shape != x.shape:
            raise ValueError(f"observe_hvp: xdot must be ({self.K},{self._cols}), the shape of x")
        n, m, E, N = self.n, self.m, self.E, self.N
        if ybar is None and xbar_final is None:
            raise ValueError("observe_hvp: nothing to pull back (ybar and xbar_final are both None)")
        if ops is None:
            if ybar is not None or ybar_dot is not None:
                raise ValueError("observe_hvp: ybar / ybar_dot need the probes they belong to")
        n_obs, O = self._jvp_probes("observe_hvp", ops, per_member)
        Of = None if O is None else _cm(np.swapaxes(O, 0, 1) if per_member else O)
        if ybar is None and ybar_dot is None:
            n_obs, Of = 0, None                                   # (probes without cotangents: nothing of theirs to pull back)

        def rows(a, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.complex128)
            if a.shape != (E, n_obs, N + 1):
                raise ValueError(f"observe_hvp: {name} must be ({E},{n_obs},{N + 1})")
            return a

        def finals(a, name):
            if a is None:
                return None
            a = np.asarray(a, dtype=np.complex128)
            if a.shape != (E, n, m):
                raise ValueError(f"observe_hvp: {name} must be ({E},{n},{m})")
            return _cm(a)

        yb, ybd = rows(ybar, "ybar"), rows(ybar_dot, "ybar_dot")
        xb, xbd = finals(xbar_final, "xbar_final"), finals(xbar_final_dot, "xbar_final_dot")
        Gd = np.empty((self._cols, self.K))
        xf, xdf = np.ascontiguousarray(x.T), np.ascontiguousarray(xd.T)
        self._check(self._lib.grape_eval_hvp(self._h, _p(xf), _p(xdf), n_obs, 1 if per_member else 0, _p(Of), _p(yb), _p(xb),
                                             _p(ybd), _p(xbd), _p(Gd)))
        return np.ascontiguousarray(Gd.T)

    def _gnvp_weights(self, who, w, n_obs, blocks):
        """(w_per_member, the three planes rr / ri / ii as the library reads them) of observe_gnvp's w"""
        E, N = self.E, self.N
        w = np.asarray(w, dtype=np.float64)
        shared, member = (n_obs, N + 1), (E, n_obs, N + 1)
        if blocks is not True and w.shape in (shared, member):    # scalar weights: rr = ii = w, ri = 0
            planes = np.stack([w, np.zeros_like(w), w])
        elif blocks is not False and w.shape in ((3,) + shared, (3,) + member):
            planes = w
        else:
            raise ValueError(f"{who}: w must be ({n_obs},{N + 1}) or ({E},{n_obs},{N + 1}), or the three planes rr, ri, ii of "
                             f"either behind a leading axis of 3")
        return (1 if planes.ndim == 4 else 0), np.ascontiguousarray(planes)

    def observe_gnvp(self, x, xdot, ops, w=None, wf=None, per_member=False, blocks=None):
        """grape_eval_gnvp: the weighted Gauss-Newton product J' W J xdot of observe() in one trajectory pass --
        observe_vjp(x, ops, ybar = W ydot, xbar_final = wf Xdot_final) of (ydot, Xdot_final) = observe_jvp(x, xdot, ops,
        final=True), without either array.  w: real weights of y's entries, (E, n_obs, N+1) or (n_obs, N+1) shared by the
        members; behind a leading axis of 3 the planes rr, ri, ii of a real symmetric 2x2 block per entry, acting on
        (Re ydot, Im ydot).  blocks=None infers which from the shape, and an array of y's own shape is scalar weights per member
        -- with E = 3 that is also the shape of shared planes: blocks=True reads the leading axis of 3 as the planes,
        blocks=False never does.  wf (E,): the weights of the final
        states, the Gauss-Newton term of 1/2 wf_k |X_N - T|^2.  Either may be None, not both.  Returns Gn (K, cols) in the
        coordinates of x (basis and bounds are served), first order in dt, without ensemble weights, penalties, running cost
        or risk.  The contexts observe_vjp serves, in the first-order trajectory derivative mode (include/grape_hip.h)."""
        x = np.asarray(x, dtype=np.float64)
        xd = np.asarray(xdot, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        if xd.shape != x.shape:
            raise ValueError(f"observe_gnvp: xdot must be ({self.K},{self._cols}), the shape of x")
        if w is None and wf is None:
            raise ValueError("observe_gnvp: nothing to weight (w and wf are both None)")
        if ops is None and w is not None:
            raise ValueError("observe_gnvp: w needs the probes it belongs to")
        n_obs, O = self._jvp_probes("observe_gnvp", ops, per_member)
        Of = None if O is None else _cm(np.swapaxes(O, 0, 1) if per_member else O)
        wpm, wy = 0, None
        if w is not None:
            wpm, wy = self._gnvp_weights("observe_gnvp", w, n_obs, blocks)
        else:
            n_obs, Of = 0, None                                   # (probes without weights: nothing of theirs enters)
        wff = None
        if wf is not None:
            wff = np.ascontiguousarray(wf, dtype=np.float64)
            if wff.shape != (self.E,):
                raise ValueError(f"observe_gnvp: wf must be ({self.E},)")
        Gn = np.empty((self._cols, self.K))
        xf, xdf = np.ascontiguousarray(x.T), np.ascontiguousarray(xd.T)
        self._check(self._lib.grape_eval_gnvp(self._h, _p(xf), _p(xdf), n_obs, 1 if per_member else 0, _p(Of), wpm, _p(wy), _p(wff),
                                              _p(Gn)))
        return np.ascontiguousarray(Gn.T)

    def gn_step(self, x, ops, y_target=None, w=None, xf_target=None, wf=None, lam=0.0, cg_iter=20, cg_rtol=1e-10, per_member=False,
                blocks=None):
        """grape_gn_step: one Levenberg-Marquardt step of L(x) = 1/2 sum r' W r + 1/2 sum_k wf_k |X_N - xf_target|^2
        (r = observe(x) - y_target) solved on the device -- one sweep, one upload, the CG iterations on
        (J' W J + lam 1) p = -g along the stored trajectory.  y_target (E, n_obs, N+1) complex with w (None: ones; shaped and
        inferred exactly as in observe_gnvp) and / or xf_target (E, n, m) with wf (None: ones).  cg_iter: operator
        applications at most (0: loss and gradient only, p = 0); cg_rtol: stop at |r| <= cg_rtol |g|.  Returns dict(p, g
        (K, cols) in the coordinates of x, loss, predicted (the model decrease -g'p - p'Hp/2), iterations, status (0 converged,
        1 iteration limit, 2 no positive curvature / NaN, 3 g = 0), residual, g_norm, g_inf, p_norm)."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        n, m, E, N = self.n, self.m, self.E, self.N
        if y_target is None and xf_target is None:
            raise ValueError("gn_step: nothing to fit (y_target and xf_target are both None)")
        if y_target is None and w is not None:
            raise ValueError("gn_step: w needs the y_target it weights")
        if xf_target is None and wf is not None:
            raise ValueError("gn_step: wf needs the xf_target it weights")
        if ops is None and y_target is not None:
            raise ValueError("gn_step: y_target needs the probes it belongs to")
        n_obs, O = self._jvp_probes("gn_step", ops, per_member)
        Of = None if O is None else _cm(np.swapaxes(O, 0, 1) if per_member else O)
        wpm, wy, yt = 0, None, None
        if y_target is not None:
            yt = np.ascontiguousarray(y_target, dtype=np.complex128)
            if yt.shape != (E, n_obs, N + 1):
                raise ValueError(f"gn_step: y_target must be ({E},{n_obs},{N + 1})")
            wpm, wy = self._gnvp_weights("gn_step", np.ones((n_obs, N + 1)) if w is None else w, n_obs, blocks)
        else:
            n_obs, Of = 0, None                                   # (probes without a target: nothing of theirs enters)
        wff, xt = None, None
        if xf_target is not None:
            xt = np.asarray(xf_target, dtype=np.complex128)
            if xt.shape != (E, n, m):
                raise ValueError(f"gn_step: xf_target must be ({E},{n},{m})")
            xt = _cm(xt)
            wff = np.ones(E) if wf is None else np.ascontiguousarray(wf, dtype=np.float64)
            if wff.shape != (E,):
                raise ValueError(f"gn_step: wf must be ({E},)")
        opts = GrapeGnOptions(float(lam), float(cg_rtol), int(cg_iter), 0)
        res = GrapeGnResult()
        p, g = np.empty((self._cols, self.K)), np.empty((self._cols, self.K))
        xf = np.ascontiguousarray(x.T)
        self._check(self._lib.grape_gn_step(self._h, _p(xf), n_obs, 1 if per_member else 0, _p(Of), _p(yt), wpm, _p(wy), _p(xt),
                                            _p(wff), C.byref(opts), _p(p), _p(g), C.byref(res)))
        return dict(p=np.ascontiguousarray(p.T), g=np.ascontiguousarray(g.T), loss=res.loss, predicted=res.predicted,
                    iterations=res.cg_iterations, status=res.status, residual=res.residual, g_norm=res.g_norm, g_inf=res.g_inf,
                    p_norm=res.p_norm)

    def observe_gnvp_device(self, d_x, d_xdot, n_obs, per_member, d_O, w_per_member, d_wy, d_wf, d_Gn, stream=0):
        """grape_eval_gnvp_device with raw device pointers, layouts as observe_jvp_device; d_wy f64 (N+1, n_obs, [E,] 3), planes
        rr, ri, ii slowest, d_wf f64 (E), 0 for zero (not both); d_Gn f64 (K, cols) column-major.  d_x=0: reuse -- along the
        trajectory the last device form left in the workspace, without a sweep (GrapeError NOT_READY when anything else has
        touched the context since, or under a member chunk); the other reuse forms may follow.  One call per CG iteration."""
        n_obs = self._traj_device_args("observe_gnvp_device", 1, n_obs, d_O, d_wy, d_wf, "d_wy and d_wf")
        if not d_xdot:
            raise ValueError("observe_gnvp_device: d_xdot is null")
        if not d_Gn:
            raise ValueError("observe_gnvp_device: d_Gn is null")
        self._check(self._lib.grape_eval_gnvp_device(self._h, C.c_void_p(d_x), C.c_void_p(d_xdot), n_obs, 1 if per_member else 0,
                                                     C.c_void_p(d_O), int(w_per_member), C.c_void_p(d_wy), C.c_void_p(d_wf),
                                                     C.c_void_p(d_Gn), C.c_void_p(stream)))

    def observe_device(self, d_x, n_obs, per_member, d_O, d_y, d_X_final, d_fg=0, stream=0):
        """grape_eval_observables_device with raw device pointers (e.g. torch tensor .data_ptr()), in the library's layouts:
        d_x f64 (K, cols) column-major, d_O c128 (n, m, [E,] n_obs), d_y c128 (N+1, n_obs, E), d_X_final c128 (n, m, E), d_fg
        f64 [K cols + 1]; 0 for an output that is not wanted (not d_y and d_X_final both).  Asynchronous on `stream`; the
        arrays stay alive until the stream has passed the call.  Non-finite device entries are not checked."""
        n_obs = self._traj_device_args("observe_device", d_x, n_obs, d_O, d_y, d_X_final, "d_y and d_X_final")
        self._check(self._lib.grape_eval_observables_device(self._h, C.c_void_p(d_x), n_obs, 1 if per_member else 0, C.c_void_p(d_O),
                                                            C.c_void_p(d_y), C.c_void_p(d_X_final), C.c_void_p(d_fg),
                                                            C.c_void_p(stream)))

    def observe_vjp_device(self, d_x, n_obs, per_member, d_O, d_ybar, d_Xbar_final, d_G, stream=0):
        """grape_eval_vjp_device with raw device pointers, layouts as observe_device; d_G f64 (K, cols) column-major.  d_x=0:
        reuse -- pull back along the trajectory the last observe_device / observe_vjp_device left in the workspace, without
        a sweep (GrapeError NOT_READY when anything else has touched the context since, or under a member chunk)."""
        n_obs = self._traj_device_args("observe_vjp_device", 1, n_obs, d_O, d_ybar, d_Xbar_final, "d_ybar and d_Xbar_final")
        if not d_G:
            raise ValueError("observe_vjp_device: d_G is null")
        self._check(self._lib.grape_eval_vjp_device(self._h, C.c_void_p(d_x), n_obs, 1 if per_member else 0, C.c_void_p(d_O),
                                                    C.c_void_p(d_ybar), C.c_void_p(d_Xbar_final), C.c_void_p(d_G),
                                                    C.c_void_p(stream)))

    def observe_jvp_device(self, d_x, d_xdot, n_obs, per_member, d_O, d_ydot, d_Xdot_final, stream=0):
        """grape_eval_jvp_device with raw device pointers, layouts as observe_device; d_xdot f64 (K, cols) column-major like
        d_x.  d_x=0: reuse -- push d_xdot forward along the trajectory the last device form left in the workspace, without a
        sweep (GrapeError NOT_READY when anything else has touched the context since, or under a member chunk); an
        observe_vjp_device(0, ...) may follow at the same point."""
        n_obs = self._traj_device_args("observe_jvp_device", 1, n_obs, d_O, d_ydot, d_Xdot_final, "d_ydot and d_Xdot_final")
        if not d_xdot:
            raise ValueError("observe_jvp_device: d_xdot is null")
        self._check(self._lib.grape_eval_jvp_device(self._h, C.c_void_p(d_x), C.c_void_p(d_xdot), n_obs, 1 if per_member else 0,
                                                    C.c_void_p(d_O), C.c_void_p(d_ydot), C.c_void_p(d_Xdot_final),
                                                    C.c_void_p(stream)))

    def observe_hvp_device(self, d_x, d_xdot, n_obs, per_member, d_O, d_ybar, d_Xbar_final, d_ybar_dot, d_Xbar_final_dot, d_Gdot,
                           stream=0):
        """grape_eval_hvp_device with raw device pointers, layouts as observe_vjp_device / observe_jvp_device; d_ybar_dot and
        d_Xbar_final_dot in the layouts of d_ybar / d_Xbar_final, 0 for zero; d_Gdot f64 (K, cols) column-major.  d_x=0: reuse
        -- along the trajectory the last device form left in the workspace, without a sweep (GrapeError NOT_READY when
        anything else has touched the context since, or under a member chunk); the other reuse forms may follow."""
        n_obs = self._traj_device_args("observe_hvp_device", 1, n_obs, d_O, d_ybar, d_Xbar_final, "d_ybar and d_Xbar_final")
        if not d_xdot:
            raise ValueError("observe_hvp_device: d_xdot is null")
        if not d_Gdot:
            raise ValueError("observe_hvp_device: d_Gdot is null")
        self.calls += 1
        self._check(self._lib.grape_eval_hvp_device(self._h, C.c_void_p(d_x), C.c_void_p(d_xdot), n_obs, 1 if per_member else 0,
                                                    C.c_void_p(d_O), C.c_void_p(d_ybar), C.c_void_p(d_Xbar_final),
                                                    C.c_void_p(d_ybar_dot), C.c_void_p(d_Xbar_final_dot), C.c_void_p(d_Gdot),
                                                    C.c_void_p(stream)))

    def _jvp_probes(self, who, ops, per_member):
        """(n_obs, O as (n_obs, n, m) / (E, n_obs, n, m) complex128) of the jvp forms; ops=None: (0, None)"""
        if ops is None:
            return 0, None
        n, m, E = self.n, self.m, self.E
        O = np.asarray(ops, dtype=np.complex128)
        if not per_member and O.ndim == 2:
            O = O[None]
        want = (E, O.shape[1] if O.ndim == 4 else 0, n, m) if per_member else (O.shape[0] if O.ndim == 3 else 0, n, m)
        if O.shape != want or not 1 <= O.shape[-3] <= 16:
            raise ValueError(f"{who}: ops must be {'(E, n_obs, n, m)' if per_member else '(n_obs, n, m)'} with "
                             f"E = {E}, n = {n}, m = {m} and 1 <= n_obs <= 16")
        return O.shape[-3], O

    def observe_jvp_multi(self, x, xdots, ops, per_member=False, final=False):
        """grape_eval_jvp_multi: observe_jvp for several directions behind ONE evaluation of x.  xdots (n_dir, K, cols), every
        direction of x's shape and coordinates.  Returns ydot (n_dir, E, n_obs, N+1) -- then Xdot_final (n_dir, E, n, m) with
        final=True; block d is bit for bit observe_jvp(x, xdots[d], ...).  More than MAX_JVP_DIRECTIONS = 8 directions are
        walked in blocks of 8 (one evaluation each)."""
        x = np.asarray(x, dtype=np.float64)
        xd = np.asarray(xdots, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        if xd.ndim != 3 or xd.shape[1:] != x.shape or xd.shape[0] < 1:
            raise ValueError(f"observe_jvp_multi: xdots must be (n_dir, {self.K}, {self._cols}) with n_dir >= 1")
        if ops is None and not final:
            raise ValueError("observe_jvp_multi: nothing asked for (ops=None needs final=True)")
        n, m, E, N = self.n, self.m, self.E, self.N
        n_obs, O = self._jvp_probes("observe_jvp_multi", ops, per_member)
        Of = None if O is None else _cm(np.swapaxes(O, 0, 1) if per_member else O)
        n_dir = xd.shape[0]
        yd = np.empty((n_dir, E, n_obs, N + 1), np.complex128) if n_obs else None
        Xf = np.empty((n_dir, E, m, n), np.complex128) if final else None
        xf = np.ascontiguousarray(x.T)
        for d0 in range(0, n_dir, MAX_JVP_DIRECTIONS):
            d1 = min(n_dir, d0 + MAX_JVP_DIRECTIONS)
            xdf = np.ascontiguousarray(np.swapaxes(xd[d0:d1], 1, 2))
            yb = None if yd is None else yd[d0:d1]
            Xb = None if Xf is None else Xf[d0:d1]
            self._check(self._lib.grape_eval_jvp_multi(self._h, _p(xf), d1 - d0, _p(xdf), n_obs, 1 if per_member else 0, _p(Of),
                                                       _p(yb), _p(Xb)))
        if final:
            return yd, np.ascontiguousarray(np.swapaxes(Xf, -1, -2))
        return yd

    def observe_jvp_multi_device(self, x, xdots, ops, per_member=False, final=False, stream=0):
        """grape_eval_jvp_multi_device on CUDA tensors of the context's GPU: x float64 (K, cols), or None for reuse -- along the
        trajectory the last device form left in the workspace, without a sweep (GrapeError NOT_READY when anything else has
        touched the context since, or under a member chunk); xdots float64 (n_dir, K, cols); ops complex128 as in observe_jvp
        (None with final=True).  Returns CUDA tensors ydot (n_dir, E, n_obs, N+1) -- then Xdot_final (n_dir, E, n, m) with
        final=True -- written asynchronously on `stream` (0: the default stream; the layout copies of the inputs run on torch's
        current stream, which must be the same or ordered in front of it).  More than 8 directions are walked in blocks of 8,
        the blocks behind the first one by reuse.  Non-finite device entries are not checked."""
        import torch

        K, cols, n, m, E, N = self.K, self._cols, self.n, self.m, self.E, self.N
        if x is not None and (not x.is_cuda or x.dtype != torch.float64 or tuple(x.shape) != (K, cols)):
            raise ValueError(f"observe_jvp_multi_device: x must be a CUDA float64 tensor ({K},{cols}) or None")
        if not xdots.is_cuda or xdots.dtype != torch.float64 or xdots.dim() != 3 or tuple(xdots.shape[1:]) != (K, cols) \
                or xdots.shape[0] < 1:
            raise ValueError(f"observe_jvp_multi_device: xdots must be a CUDA float64 tensor (n_dir, {K}, {cols}) with n_dir >= 1")
        if ops is None and not final:
            raise ValueError("observe_jvp_multi_device: nothing asked for (ops=None needs final=True)")
        n_obs, d_O = 0, None
        if ops is not None:
            if not ops.is_cuda or ops.dtype != torch.complex128:
                raise ValueError("observe_jvp_multi_device: ops must be a CUDA complex128 tensor")
            O = ops[None] if (not per_member and ops.dim() == 2) else ops
            want = (E, O.shape[1] if O.dim() == 4 else 0, n, m) if per_member else (O.shape[0] if O.dim() == 3 else 0, n, m)
            if tuple(O.shape) != want or not 1 <= O.shape[-3] <= 16:
                raise ValueError(f"observe_jvp_multi_device: ops must be {'(E, n_obs, n, m)' if per_member else '(n_obs, n, m)'} "
                                 f"with E = {E}, n = {n}, m = {m} and 1 <= n_obs <= 16")
            n_obs = O.shape[-3]
            # column-major (n, m, [E,] n_obs): the probe index slowest, then the member
            d_O = (O.transpose(0, 1) if per_member else O).transpose(-1, -2).contiguous()
        dev = xdots.device
        n_dir = xdots.shape[0]
        d_x = None if x is None else x.t().contiguous()
        d_xd = xdots.transpose(1, 2).contiguous()
        yd = torch.empty((n_dir, E, n_obs, N + 1), dtype=torch.complex128, device=dev) if n_obs else None
        Xf = torch.empty((n_dir, E, m, n), dtype=torch.complex128, device=dev) if final else None
        reuse_ok = n_dir <= MAX_JVP_DIRECTIONS or self._jacobian_reuse()      # (a member chunk: every block carries x)
        for d0 in range(0, n_dir, MAX_JVP_DIRECTIONS):
            d1 = min(n_dir, d0 + MAX_JVP_DIRECTIONS)
            ptr = lambda t: C.c_void_p(0 if t is None else t[d0:d1].data_ptr())
            first = d_x is not None and (d0 == 0 or not reuse_ok)
            self._check(self._lib.grape_eval_jvp_multi_device(self._h, C.c_void_p(d_x.data_ptr() if first else 0), d1 - d0,
                                                              ptr(d_xd), n_obs, 1 if per_member else 0,
                                                              C.c_void_p(0 if d_O is None else d_O.data_ptr()), ptr(yd), ptr(Xf),
                                                              C.c_void_p(stream)))
        self._jvp_multi_keep = (d_x, d_xd, d_O)              # (alive until the stream has passed the call)
        if final:
            return yd, Xf.transpose(-1, -2).contiguous()
        return yd

    def observe_vjp_multi(self, x, ops, ybars=None, xbars_final=None, per_member=False):
        """grape_eval_vjp_multi: observe_vjp for several cotangent sets behind ONE evaluation of x.  ybars (n_set, E, n_obs, N+1)
        and xbars_final (n_set, E, n, m), either None (zero) for all sets, not both; the probes are shared by the sets.
        Returns G (n_set, K, cols); block r is bit for bit observe_vjp(x, ops, ybars[r], xbars_final[r]).  More than
        MAX_VJP_COTANGENTS = 8 sets are walked in blocks of 8 (one evaluation each)."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        n, m, E, N = self.n, self.m, self.E, self.N
        if ybars is None and xbars_final is None:
            raise ValueError("observe_vjp_multi: nothing to pull back (ybars and xbars_final are both None)")
        if ops is None and ybars is not None:
            raise ValueError("observe_vjp_multi: ybars needs the probes it belongs to")
        n_obs, O = self._jvp_probes("observe_vjp_multi", ops if ybars is not None else None, per_member)
        Of = None if O is None else _cm(np.swapaxes(O, 0, 1) if per_member else O)
        yb = xb = None
        if ybars is not None:
            yb = np.ascontiguousarray(ybars, dtype=np.complex128)
            if yb.ndim != 4 or yb.shape[1:] != (E, n_obs, N + 1) or yb.shape[0] < 1:
                raise ValueError(f"observe_vjp_multi: ybars must be (n_set, {E},{n_obs},{N + 1}) with n_set >= 1")
        if xbars_final is not None:
            xb = np.asarray(xbars_final, dtype=np.complex128)
            if xb.ndim != 4 or xb.shape[1:] != (E, n, m) or xb.shape[0] < 1:
                raise ValueError(f"observe_vjp_multi: xbars_final must be (n_set, {E},{n},{m}) with n_set >= 1")
            xb = _cm(xb)
        if yb is not None and xb is not None and yb.shape[0] != xb.shape[0]:
            raise ValueError("observe_vjp_multi: ybars and xbars_final differ in n_set")
        n_set = (yb if yb is not None else xb).shape[0]
        G = np.empty((n_set, self._cols, self.K))
        xf = np.ascontiguousarray(x.T)
        for r0 in range(0, n_set, MAX_VJP_COTANGENTS):
            r1 = min(n_set, r0 + MAX_VJP_COTANGENTS)
            part = lambda a: None if a is None else a[r0:r1]
            self._check(self._lib.grape_eval_vjp_multi(self._h, _p(xf), r1 - r0, n_obs, 1 if per_member else 0, _p(Of),
                                                       _p(part(yb)), _p(part(xb)), _p(G[r0:r1])))
        return np.ascontiguousarray(np.swapaxes(G, 1, 2))

    def observe_vjp_multi_device(self, x, ops, ybars=None, xbars_final=None, per_member=False, stream=0):
        """grape_eval_vjp_multi_device on CUDA tensors of the context's GPU: x float64 (K, cols), or None for reuse -- along the
        trajectory the last device form left in the workspace, without a sweep (GrapeError NOT_READY when anything else has
        touched the context since, or under a member chunk); ops complex128 as in observe_vjp (None with xbars_final alone);
        ybars complex128 (n_set, E, n_obs, N+1) and xbars_final complex128 (n_set, E, n, m), either None, not both.  Returns
        the CUDA tensor G (n_set, K, cols), written asynchronously on `stream` (0: the default stream; the layout copies of
        the inputs run on torch's current stream, which must be the same or ordered in front of it).  More than 8 sets are
        walked in blocks of 8, the blocks behind the first one by reuse.  Non-finite device entries are not checked."""
        import torch

        K, cols, n, m, E, N = self.K, self._cols, self.n, self.m, self.E, self.N
        who = "observe_vjp_multi_device"
        if x is not None and (not x.is_cuda or x.dtype != torch.float64 or tuple(x.shape) != (K, cols)):
            raise ValueError(f"{who}: x must be a CUDA float64 tensor ({K},{cols}) or None")
        if ybars is None and xbars_final is None:
            raise ValueError(f"{who}: nothing to pull back (ybars and xbars_final are both None)")
        n_obs, d_O = 0, None
        if ybars is not None:
            if ops is None:
                raise ValueError(f"{who}: ybars needs the probes it belongs to")
            if not ops.is_cuda or ops.dtype != torch.complex128:
                raise ValueError(f"{who}: ops must be a CUDA complex128 tensor")
            O = ops[None] if (not per_member and ops.dim() == 2) else ops
            want = (E, O.shape[1] if O.dim() == 4 else 0, n, m) if per_member else (O.shape[0] if O.dim() == 3 else 0, n, m)
            if tuple(O.shape) != want or not 1 <= O.shape[-3] <= 16:
                raise ValueError(f"{who}: ops must be {'(E, n_obs, n, m)' if per_member else '(n_obs, n, m)'} "
                                 f"with E = {E}, n = {n}, m = {m} and 1 <= n_obs <= 16")
            n_obs = O.shape[-3]
            # column-major (n, m, [E,] n_obs): the probe index slowest, then the member
            d_O = (O.transpose(0, 1) if per_member else O).transpose(-1, -2).contiguous()
            if not ybars.is_cuda or ybars.dtype != torch.complex128 or ybars.dim() != 4 \
                    or tuple(ybars.shape[1:]) != (E, n_obs, N + 1) or ybars.shape[0] < 1:
                raise ValueError(f"{who}: ybars must be a CUDA complex128 tensor (n_set, {E},{n_obs},{N + 1}) with n_set >= 1")
        if xbars_final is not None and (not xbars_final.is_cuda or xbars_final.dtype != torch.complex128 or xbars_final.dim() != 4
                                        or tuple(xbars_final.shape[1:]) != (E, n, m) or xbars_final.shape[0] < 1):
            raise ValueError(f"{who}: xbars_final must be a CUDA complex128 tensor (n_set, {E},{n},{m}) with n_set >= 1")
        if ybars is not None and xbars_final is not None and ybars.shape[0] != xbars_final.shape[0]:
            raise ValueError(f"{who}: ybars and xbars_final differ in n_set")
        n_set = (ybars if ybars is not None else xbars_final).shape[0]
        d_x = None if x is None else x.t().contiguous()
        d_yb = None if ybars is None else ybars.contiguous()
        d_xb = None if xbars_final is None else xbars_final.transpose(-1, -2).contiguous()
        G = torch.empty((n_set, cols, K), dtype=torch.float64, device=(ybars if ybars is not None else xbars_final).device)
        reuse_ok = n_set <= MAX_VJP_COTANGENTS or self._jacobian_reuse()     # (a member chunk: every block carries x)
        for r0 in range(0, n_set, MAX_VJP_COTANGENTS):
            r1 = min(n_set, r0 + MAX_VJP_COTANGENTS)
            ptr = lambda t: C.c_void_p(0 if t is None else t[r0:r1].data_ptr())
            first = d_x is not None and (r0 == 0 or not reuse_ok)
            self._check(self._lib.grape_eval_vjp_multi_device(self._h, C.c_void_p(d_x.data_ptr() if first else 0), r1 - r0, n_obs,
                                                              1 if per_member else 0,
                                                              C.c_void_p(0 if d_O is None else d_O.data_ptr()), ptr(d_yb), ptr(d_xb),
                                                              ptr(G), C.c_void_p(stream)))
        self._vjp_multi_keep = (d_x, d_O, d_yb, d_xb)        # (alive until the stream has passed the call)
        return G.transpose(1, 2).contiguous()

    def trajectory_jacobian_rows(self, x, ops, rows, per_member=False):
        """Rows of the Jacobian of observe(x, ops) in reverse mode, the twin of trajectory_jacobian: `rows` is a list of
        (member, probe, slice) triples, the result J (n_rows, K, cols) is complex with J[r] = d y[member, probe, slice] / d x.
        Each row is two unit cotangents (1: the real part's gradient, i: the imaginary part's), so a block of 8 cotangent
        sets serves 4 rows; the first block carries x, the rest reuse its trajectory (member-chunked contexts: every block
        carries x).  It pays off where there are fewer residuals than controls.  In the derivative mode of
        set_trajectory_derivative."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        O = np.asarray(ops)
        n_obs = 1 if (not per_member and O.ndim == 2) else O.shape[-3]
        rows = [tuple(int(v) for v in r) for r in rows]
        if not rows:
            raise ValueError("trajectory_jacobian_rows: no rows")
        for r in rows:
            if len(r) != 3 or not (0 <= r[0] < self.E and 0 <= r[1] < n_obs and 0 <= r[2] <= self.N):
                raise ValueError(f"trajectory_jacobian_rows: row {r} is not a (member < {self.E}, probe < {n_obs}, "
                                 f"slice <= {self.N}) triple")
        reuse_ok = self._jacobian_reuse()
        per_block = MAX_VJP_COTANGENTS // 2
        out = []
        for b in range(0, len(rows), per_block):
            block = rows[b:b + per_block]
            ybars = np.zeros((2 * len(block), self.E, n_obs, self.N + 1), np.complex128)
            for i, (k, j, s) in enumerate(block):
                ybars[2 * i, k, j, s] = 1.0
                ybars[2 * i + 1, k, j, s] = 1.0j
            G = self._jacobian_rows_block(x, b == 0 or not reuse_ok, ybars, ops, per_member)
            out.append(G[0::2] + 1j * G[1::2])
        return np.concatenate(out, axis=0)

    def _jacobian_rows_block(self, x, carry_x, ybars, ops, per_member):
        """one block of trajectory_jacobian_rows through the device form: G (len(ybars), K, cols) as a NumPy array"""
        import torch

        dev = torch.device("cuda", self.info["device"])
        state = getattr(self, "_jacobian_rows_dev", None)
        if carry_x or state is None:                         # (x and the probes go up once per walk)
            state = self._jacobian_rows_dev = (torch.as_tensor(x, device=dev),
                                               torch.as_tensor(np.asarray(ops, np.complex128), device=dev))
        G = self.observe_vjp_multi_device(state[0] if carry_x else None, state[1], torch.as_tensor(ybars, device=dev),
                                          per_member=per_member)
        torch.cuda.synchronize(dev)
        return G.cpu().numpy()

    def trajectory_jacobian(self, x, ops, columns=None, per_member=False):
        """dy/dx of observe(x, ops) for the listed flat indices of x (row-major over (K, cols); all by default): an array
        (len(columns), E, n_obs, N+1) whose entry j is d y / d x.flat[columns[j]], built from unit directions in blocks of 8
        through the device form -- the first block carries x, the rest reuse its trajectory (member-chunked contexts: every
        block carries x).  In the derivative mode of set_trajectory_derivative."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.K, self._cols):
            raise ValueError(f"x must be ({self.K},{self._cols})")
        cols = jacobian_columns(x.size, columns)
        reuse_ok = self._jacobian_reuse()
        out = []
        for b, block in enumerate(jacobian_blocks(cols, MAX_JVP_DIRECTIONS)):
            dirs = np.zeros((len(block), x.size))
            dirs[np.arange(len(block)), block] = 1.0
            out.append(self._jacobian_block(x, b == 0 or not reuse_ok, dirs.reshape((len(block),) + x.shape), ops, per_member))
        return np.concatenate(out, axis=0)

    def _jacobian_reuse(self):
        """the blocks behind the first may reuse its trajectory: not under a member chunk"""
        return self.info["member_chunk"] >= self.E

    def _jacobian_block(self, x, carry_x, dirs, ops, per_member):
        """one block of trajectory_jacobian through the device form: ydot (len(dirs), E, n_obs, N+1) as a NumPy array"""
        import torch

        dev = torch.device("cuda", self.info["device"])
        state = getattr(self, "_jacobian_dev", None)
        if carry_x or state is None:                         # (x and the probes go up once per walk)
            state = self._jacobian_dev = (torch.as_tensor(x, device=dev), torch.as_tensor(np.asarray(ops, np.complex128), device=dev))
        yd = self.observe_jvp_multi_device(state[0] if carry_x else None, torch.as_tensor(dirs, device=dev), state[1],
                                           per_member=per_member)
        torch.cuda.synchronize(dev)
        return yd.cpu().numpy()

    @staticmethod
    def _traj_device_args(who, d_x, n_obs, d_O, d_a, d_b, names):
        n_obs = int(n_obs)
        if not 0 <= n_obs <= 16:
            raise ValueError(f"{who}: n_obs = {n_obs} (must be in 0..16)")
        if not d_x:
            raise ValueError(f"{who}: d_x is null")
        if not d_a and not d_b:
            raise ValueError(f"{who}: {names} are both null")
        if n_obs > 0 and not d_O:
            raise ValueError(f"{who}: n_obs > 0 with a null d_O")
        return n_obs

    def eval_device(self, d_x_ptr, d_fg_ptr, stream=0):
        """grape_eval_device with raw device pointers (e.g. torch tensor .data_ptr())."""
        self._check(self._lib.grape_eval_device(self._h, C.c_void_p(d_x_ptr), C.c_void_p(d_fg_ptr),
                                                C.c_void_p(stream)))

    def eval_batch_device(self, n_x, d_x_ptr, d_fg_ptr, stream=0):
        """grape_eval_batch_device with raw device pointers: d_x (K,N,n_x) f64, d_fg n_x blocks of (K*N+1) f64."""
        self._check(self._lib.grape_eval_batch_device(self._h, int(n_x), C.c_void_p(d_x_ptr), C.c_void_p(d_fg_ptr),
                                                      C.c_void_p(stream)))

    def member_results(self):
        foms = np.empty(self.E)
        grads = np.empty((self.E, self.N, self.K))
        self._check(self._lib.grape_get_member_results(self._h, _p(foms), _p(grads)))
        return foms, np.ascontiguousarray(np.swapaxes(grads, 1, 2))

    def trajectory(self, member, costates=False, states=True):
        n, N, m = self.n, self.N, self.m
        P = np.empty((N, n, n), np.complex128)
        X = np.empty((N + 1, m, n), np.complex128) if states else None       # column-major n x m each
        Lc = np.empty((N + 1, m, n), np.complex128) if costates else None
        self._check(self._lib.grape_get_trajectory(self._h, int(member), _p(P), _p(X), _p(Lc)))
        sw = lambda a: None if a is None else np.ascontiguousarray(np.swapaxes(a, -1, -2))
        return (sw(P), sw(X), sw(Lc)) if costates else (sw(P), sw(X))

    def phase_stamps(self):
        """(E*W, 10) uint64 stamps of the last evaluation (FLAG_PHASE_STAMPS): columns 0..4 shader clock at the phase
        boundaries, 5 and 6 the 100 MHz counter behind the prologue and at the end, 7 hardware ids, 8 and 9 the 100 MHz
        counter and the shader clock at kernel entry (lane-pair kernel; 0 from the lane kernel)."""
        cnt = C.c_int64()
        self._check(self._lib.grape_get_phase_stamps(self._h, None, 0, C.byref(cnt)))
        out = np.empty(cnt.value, dtype=np.uint64)
        self._check(self._lib.grape_get_phase_stamps(self._h, _p(out), cnt.value, C.byref(cnt)))
        return out.reshape(-1, 10)

    def group_timing(self, reset=False):
        """multi-device contexts: mean host-side microseconds per grape_eval since the last reset."""
        out = np.zeros(6)
        self._check(self._lib.grape_get_group_timing(self._h, _p(out), int(reset)))
        return dict(zip(("evaluations", "stage_x_us", "issue_skew_us", "sum_issue_us", "wait_us", "total_us"), out.tolist()))

    def kernel_samples(self, capacity=65536):
        """(total_ms, first_ms): per-evaluation kernel durations since the last kernel_time(reset=True) (FLAG_TIME_KERNELS);
        first_ms = the expm part of the n = 5..32 family (0 for n <= 4)."""
        cnt = C.c_int64()
        self._check(self._lib.grape_get_kernel_samples(self._h, None, None, 0, C.byref(cnt)))
        n = min(int(cnt.value), int(capacity))
        tot, first = np.empty(n), np.empty(n)
        if n:
            self._check(self._lib.grape_get_kernel_samples(self._h, _p(tot), _p(first), n, C.byref(cnt)))
        return tot, first

    def kernel_names(self):
        """The kernels the last evaluation launched, in launch order (grape_get_kernel_names): the names a rocprofv3
        kernel trace shows, without namespace and template arguments.  After lbfgs(): the run's last evaluation, then the
        optimiser's own kernels, each name once in order of first launch."""
        need = self._lib.grape_get_kernel_names(self._h, None, 0)
        if need < 0:
            self._check(need)
        buf = C.create_string_buffer(max(int(need), 1))
        self._check(min(self._lib.grape_get_kernel_names(self._h, buf, len(buf)), 0))
        return [k for k in buf.value.decode().split(";") if k]

    def kernel_time(self, reset=False):
        ms = C.c_double()
        cnt = C.c_int64()
        self._check(self._lib.grape_get_kernel_time(self._h, C.byref(ms), C.byref(cnt), int(reset)))
        return ms.value, cnt.value
