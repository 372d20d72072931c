# GrapeHIP.jl -- the reference-side binding a QuOptimalControl.jl maintainer would add to route
# the GRAPE hot path through libgrape_hip.so (include/grape_hip.h).
#
# NOT EXECUTED IN THIS REPOSITORY'S CI: the build container and the GPU box have no Julia.  The
# file is kept thin on purpose and mirrors, call for call, quoptimalcontrol.jl_amd/engine.py +
# api.py (which ARE tested, tests/test_gpu_golden_and_api.py), so that behaviour is pinned there.
#
# What it replaces in /root/reference:
#   * the body of the closure `topt` in  solve(::Problem, ::GRAPE)          src/solve.jl:75-100
#                                    and solve(::EnsembleProblem, ::GRAPE)  src/solve.jl:164-196
#     (i.e. the loop over _fom_and_gradient_GRAPE!, src/GRAPE.jl:25-96, and the weighted sums)
#   * init_GRAPE's workspace                                                src/grape_tools.jl:4-16
# What it keeps: Problem / EnsembleProblem / init_ensemble / Optim.LBFGS / the result structs.
#
# Usage:   include("GrapeHIP.jl"); using .GrapeHIP
#          sol = solve(ens_prob, GRAPE_HIP(n_slices = 500))
module GrapeHIP

using QuOptimalControl
using QuOptimalControl: Problem, EnsembleProblem, StateTransfer, UnitaryGate, CoherenceTransfer,
                        SolutionResult, EnsembleSolutionResult, init_ensemble
using Optim
import QuOptimalControl: solve

export GRAPE_HIP, ADGRAPE_HIP, GrapeContext

const libgrape = get(ENV, "LIBGRAPE_HIP", "libgrape_hip.so")

# struct grape_config (include/grape_hip.h) -- field order and types must match exactly
struct GrapeConfig
    sys_type::Int32
    variant::Int32
    n::Int32
    n_controls::Int32
    n_slices::Int32
    n_ensemble::Int32
    duration::Float64
    device::Int32
    flags::Int32
    slices_per_lane::Int32
    waves_per_member::Int32
    expm_squarings::Int32
    max_batch::Int32
    n_state_cols::Int32              # ABI v2: 0 = square states
    n_devices::Int32                 # ABI v2: 0/1 = one GPU; 2..8 = in-library sharding + RCCL all-reduce
    device_ids::NTuple{8,Int32}
    gradient::Int32                  # 0 = reference first-order gradient, 1 = exact (2 <= n <= 64)
    objective::Int32                 # 0 = fom_func, 1 = C1 functional of the ADGRAPE path
end

sys_code(::UnitaryGate) = Int32(0)
sys_code(::StateTransfer) = Int32(1)
sys_code(::CoherenceTransfer) = Int32(2)

"New algorithm tag next to `GRAPE` (src/solve.jl:33-42)."
Base.@kwdef struct GRAPE_HIP{OPTS}
    n_slices::Int
    isinplace::Bool = true           # selects the in-place / static formula variant (sign, sum order)
    device::Int = -1
    devices::Vector{Int} = Int[]     # 2..8 HIP ordinals: the ensemble is sharded over them inside the library
    peer_sum::Bool = false           # GRAPE_FLAG_GROUP_PEER_SUM: sum the shards on devices[1] by peer copies, no RCCL
    penalties::Any = nothing         # ABI v7: PenaltyFunctionals of C3 / C4 (src/cost_functions.jl:29-39, 66-69), on the device
    optim_options::OPTS = Optim.Options()
end

const GRAPE_FLAG_GROUP_PEER_SUM = Int32(1 << 7)
cfg_flags(alg::GRAPE_HIP) = alg.peer_sum ? GRAPE_FLAG_GROUP_PEER_SUM : Int32(0)
cfg_flags(alg) = Int32(0)

"""
Counterpart of `ADGRAPE` (src/solve.jl:44-52): the functional C1(Xt, U Xi [U']) of src/solve.jl:268-361 with its
EXACT gradient from the device (grape_config.gradient = 1, objective = 1) instead of a Zygote tape.
"""
Base.@kwdef struct ADGRAPE_HIP{OPTS}
    n_slices::Int
    device::Int = -1
    devices::Vector{Int} = Int[]
    penalties::Any = nothing
    optim_options::OPTS = Optim.Options()
end

# per-algorithm settings of grape_config: (variant, gradient, objective)
cfg_mode(alg::GRAPE_HIP) = (alg.isinplace ? Int32(0) : Int32(1), Int32(0), Int32(0))
cfg_mode(::ADGRAPE_HIP) = (Int32(1), Int32(1), Int32(1))      # pw_evolve adds A first (src/timeevolution.jl:32-35)

mutable struct GrapeContext
    handle::Ptr{Cvoid}
    K::Int
    N::Int
    E::Int                                 # members of the context: sizes the per-member outputs (observables)
    n::Int
    m::Int
    function GrapeContext(members::Vector{<:Problem}, wts::Vector{Float64}, alg)
        p1 = members[1]
        n = size(p1.A, 1)
        m = size(p1.Xi, 2)                 # n x m states (m < n: e.g. a vectorised density matrix, test/liou.jl)
        K, N, E = p1.n_controls, alg.n_slices, length(members)
        nd = length(alg.devices)
        ids = ntuple(i -> i <= nd ? Int32(alg.devices[i]) : Int32(0), 8)
        variant, gradient, objective = cfg_mode(alg)
        cfg = GrapeConfig(sys_code(p1.sys_type), variant, n, K, N, E, Float64(p1.T),
                          nd == 1 ? alg.devices[1] : alg.device, cfg_flags(alg), 0, 0, -1, 0, m == n ? 0 : m, nd > 1 ? nd : 0, ids,
                          gradient, objective)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:grape_create, libgrape), Cint, (Ref{GrapeConfig}, Ref{Ptr{Cvoid}}), cfg, h)
        rc == 0 || error("grape_create: ", unsafe_string(ccall((:grape_last_error, libgrape), Cstring, (Ptr{Cvoid},), C_NULL)))
        ctx = new(h[], K, N, E, n, m)
        finalizer(c -> ccall((:grape_destroy, libgrape), Cint, (Ptr{Cvoid},), c.handle), ctx)
        # pack what init_ensemble produced (src/tools.jl:42-53) into contiguous column-major arrays
        A  = Array{ComplexF64}(undef, n, n, E)
        B  = Array{ComplexF64}(undef, n, n, K, E)
        Xi = Array{ComplexF64}(undef, n, m, E)
        Xt = Array{ComplexF64}(undef, n, m, E)
        for (k, p) in enumerate(members)
            A[:, :, k] .= p.A
            for j in 1:K
                B[:, :, j, k] .= p.B[j]
            end
            Xi[:, :, k] .= p.Xi
            Xt[:, :, k] .= p.Xt
        end
        check(ctx, ccall((:grape_set_operators, libgrape), Cint,
                         (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{Float64}),
                         ctx.handle, A, B, Xi, Xt, wts))
        alg.penalties === nothing || set_penalties!(ctx, alg.penalties)
        ctx
    end
end

# grape_set_penalties (ABI v7): per-control weights of C3 (amplitude) and C4 (variation); a weight is a scalar or a K-vector
function set_penalties!(ctx::GrapeContext, pf)
    w = Dict{Any,Vector{Float64}}()
    for (wt, f) in zip(pf.weights, pf.functions)
        (f === QuOptimalControl.C3 || f === QuOptimalControl.C4) || error("set_penalties!: only C3 and C4 run on the device")
        w[f] = wt isa Number ? fill(Float64(wt), ctx.K) : Vector{Float64}(wt)
    end
    amp, var = get(w, QuOptimalControl.C3, nothing), get(w, QuOptimalControl.C4, nothing)
    check(ctx, ccall((:grape_set_penalties, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx.handle,
                     amp === nothing ? C_NULL : amp, var === nothing ? C_NULL : var))
end

# grape_set_running_cost: costs on the intermediate states (C5 / C6 / C7, src/cost_functions.jl:44-61) added to every evaluation:
#   J = sum_k w_k sum_j sum_s rho[s,j] |tr(R[:,:,k,j]' X_{k,s})|^2,  X_{k,s} the state after s slices, s = 1..N
# R (n, m, E, n_terms) ComplexF64, rho (N, n_terms) Float64 -- Julia's column-major arrays are the layout the library reads;
# n_terms <= 4.  C5: R = forbidden ket, rho = +lambda; C6: R = Xt, rho = -lambda / (N D^2); C7 (kets): R = psiT, rho = -lambda / N
# (the caller adds the constant lambda).  R = nothing switches the term off.  (Written, NOT executed: no Julia toolchain where
# this file was written; the Python binding makes the same call and is tested on the GPU.)
function set_running_cost!(ctx::GrapeContext, R::Union{Nothing,Array{ComplexF64,4}}, rho::Union{Nothing,Matrix{Float64}} = nothing)
    if R === nothing
        return check(ctx, ccall((:grape_set_running_cost, libgrape), Cint, (Ptr{Cvoid}, Int32, Ptr{ComplexF64}, Ptr{Float64}),
                                ctx.handle, Int32(0), C_NULL, C_NULL))
    end
    rho === nothing && throw(ArgumentError("set_running_cost!: rho is needed with R"))
    size(rho) == (ctx.N, size(R, 4)) || throw(DimensionMismatch("rho must be (n_slices, n_terms)"))
    1 <= size(R, 4) <= 4 || throw(ArgumentError("set_running_cost!: 1 to 4 terms"))
    GC.@preserve R rho check(ctx, ccall((:grape_set_running_cost, libgrape), Cint, (Ptr{Cvoid}, Int32, Ptr{ComplexF64}, Ptr{Float64}),
                                        ctx.handle, Int32(size(R, 4)), R, rho))
end

# grape_set_basis: from here on every x handed to this context is theta (K, M) and every gradient is with respect to theta:
#   x[c,t] = x0[c,t] + sum_m theta[c,m] phi[t,m];  phi (N, M) for every control or (N, M, K), one basis per control -- Julia's
# column-major arrays are the layout the library reads.  phi = nothing switches the basis off.  (Not executed where this
# file was written: no Julia toolchain there; the Python binding makes the same two calls and is tested on the GPU.)
function set_basis!(ctx::GrapeContext, phi::Union{Nothing,Array{Float64}}, x0::Union{Nothing,Matrix{Float64}} = nothing)
    if phi === nothing
        return check(ctx, ccall((:grape_set_basis, libgrape), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
                                ctx.handle, Int32(0), Int32(1), C_NULL, C_NULL))
    end
    size(phi, 1) == ctx.N && (ndims(phi) == 2 || (ndims(phi) == 3 && size(phi, 3) == ctx.K)) ||
        throw(DimensionMismatch("phi must be (n_slices, M) or (n_slices, M, n_controls)"))
    x0 === nothing || size(x0) == (ctx.K, ctx.N) || throw(DimensionMismatch("x0 must be (n_controls, n_slices)"))
    GC.@preserve phi x0 check(ctx, ccall((:grape_set_basis, libgrape), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
                                         ctx.handle, Int32(size(phi, 2)), Int32(ndims(phi) == 3 ? ctx.K : 1), phi,
                                         x0 === nothing ? C_NULL : x0))
end

# grape_set_bounds: smooth amplitude bounds.  lo, hi: one entry per control, finite lo < hi, or -Inf / Inf for a control that
# stays free; from here on every x handed to this context is the raw pulse u (theta with a basis), the evaluation runs on
# x = mid + half tanh((u - mid) / half) and every gradient is with respect to u.  lo = nothing switches the bounds off.
# (Not executed where this file was written: no Julia toolchain there; the Python binding makes the same call and is tested
# on the GPU.)
function set_bounds!(ctx::GrapeContext, lo::Union{Nothing,Vector{Float64}}, hi::Union{Nothing,Vector{Float64}} = nothing)
    if lo === nothing
        return check(ctx, ccall((:grape_set_bounds, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                                ctx.handle, C_NULL, C_NULL))
    end
    hi === nothing && throw(ArgumentError("set_bounds!: hi is needed with lo"))
    length(lo) == ctx.K && length(hi) == ctx.K || throw(DimensionMismatch("lo and hi must have n_controls entries"))
    GC.@preserve lo hi check(ctx, ccall((:grape_set_bounds, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                                        ctx.handle, lo, hi))
end

# grape_set_risk: the soft worst case over the ensemble in place of its weighted mean -- from here on every evaluation returns
# F_beta = (W / beta) log((1 / W) sum_k w_k exp(beta F_k)) and G_beta = sum_k p_k g_k.  beta = 0 switches it off.
# (Not executed where this file was written, like set_bounds!.)
set_risk!(ctx::GrapeContext, beta::Real) =
    check(ctx, ccall((:grape_set_risk, libgrape), Cint, (Ptr{Cvoid}, Float64), ctx.handle, Float64(beta)))

"grape_get_risk_weights: p_k of the last evaluation under set_risk! (array 0 of a batch); sum(p) == sum(wts)."
function risk_weights(ctx::GrapeContext)
    p = Vector{Float64}(undef, ctx.E)
    GC.@preserve p check(ctx, ccall((:grape_get_risk_weights, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.handle, p))
    p
end

"grape_get_controls: the physical pulse (K, N) of a parameter array theta (K, M), expanded (and, with bounds, saturated) on the device."
function controls(ctx::GrapeContext, theta::Matrix{Float64})
    x = Matrix{Float64}(undef, ctx.K, ctx.N)
    GC.@preserve theta x check(ctx, ccall((:grape_get_controls, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                                          ctx.handle, theta, x))
    x
end

check(ctx::GrapeContext, rc) =
    rc == 0 || error("libgrape_hip: ", unsafe_string(ccall((:grape_last_error, libgrape), Cstring, (Ptr{Cvoid},), ctx.handle)))

"One call of the reference's closure body: returns F, fills G in place (either may be `nothing`)."
function fom_and_gradient!(ctx::GrapeContext, G, x::Matrix{Float64}; want_F = true)
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    F = Ref{Float64}(NaN)
    GC.@preserve x G begin
        gptr = G === nothing ? Ptr{Float64}(C_NULL) : pointer(G)
        fptr = want_F ? Base.unsafe_convert(Ptr{Float64}, F) : Ptr{Float64}(C_NULL)
        check(ctx, ccall((:grape_eval, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         ctx.handle, x, fptr, gptr))
    end
    F[]
end

"grape_eval_fom (ABI v8): the figure of merit of `x` without its gradient -- what a gradient-free optimiser (src/dCRAB.jl) or a
robustness scan needs; for n = 2..4 on one device a forward-only kernel, elsewhere the full evaluation's F."
function grape_fom(ctx::GrapeContext, x::Matrix{Float64})
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    F = Ref{Float64}(NaN)
    GC.@preserve x check(ctx, ccall((:grape_eval_fom, libgrape), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ref{Float64}, Ptr{Float64}),
                                    ctx.handle, Int32(1), x, F, C_NULL))
    F[]
end

# grape_eval_observables: one evaluation of x and, behind it, the expectation values along the trajectory -- what test_pulse
# (src/tools.jl:32-36) and visualise_expt_vals (src/visualisation.jl:13-51) name:
#   y[s+1, j, k] = tr(O_kj' X_{k,s}),  s = 0..N,  X_{k,0} = Xi_k;   real.(y[:, j, k]) is what visualise_expt_vals plots
# O (n, m, n_obs): probes shared by the members; O (n, m, E, n_obs): one set per member -- Julia's column-major arrays are the
# layout the library reads; n_obs <= 16.  The library writes every member of the context: y and X_final are sized from the
# context's own E, n, m, and an O of another shape is rejected before the call.  Returns (y (N+1, n_obs, E), X_final (n, m, E), F)
# with F bit for bit fom_and_gradient!'s.  n = 2..4, single-device contexts.  (Written, NOT executed: no Julia toolchain where
# this file was written; the Python binding makes the same call and is tested on the GPU.)
function observables(ctx::GrapeContext, x::Matrix{Float64}, O::Array{ComplexF64})
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    n_obs = size(O, ndims(O))
    (ndims(O) == 3 && size(O) == (ctx.n, ctx.m, n_obs)) || (ndims(O) == 4 && size(O) == (ctx.n, ctx.m, ctx.E, n_obs)) ||
        throw(DimensionMismatch("O must be (n, m, n_obs) or (n, m, E, n_obs) with the context's n, m and E"))
    1 <= n_obs <= 16 || throw(ArgumentError("observables: 1 to 16 probes"))
    y = Array{ComplexF64}(undef, ctx.N + 1, n_obs, ctx.E)
    Xf = Array{ComplexF64}(undef, ctx.n, ctx.m, ctx.E)
    F = Ref{Float64}(NaN)
    GC.@preserve x O y Xf check(ctx, ccall((:grape_eval_observables, libgrape), Cint,
                                           (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ref{Float64}),
                                           ctx.handle, x, Int32(n_obs), Int32(ndims(O) == 4 ? 1 : 0), O, y, Xf, F))
    y, Xf, F[]
end

# grape_eval_jvp: the Jacobian-vector product of `observables` -- how y and X_final move to first order (in dt too) when x
# moves along xdot, an array of x's shape:  ydot[s+1, j, k] = tr(O_kj' Xdot_{k,s}),  Xdot_final = Xdot_{k,N}.  The exact transpose
# of grape_eval_vjp; what a Gauss-Newton step on a loss on y, or a linear-response read-out, needs.  O as in `observables`.
# Returns (ydot (N+1, n_obs, E), Xdot_final (n, m, E)).  n = 2..4, UnitaryGate, single-device contexts.  (Written, NOT executed,
# like `observables`; the Python binding makes the same call and is tested on the GPU.)
function observables_jvp(ctx::GrapeContext, x::Matrix{Float64}, xdot::Matrix{Float64}, O::Array{ComplexF64})
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    size(xdot) == size(x) || throw(DimensionMismatch("xdot must have the shape of x"))
    n_obs = size(O, ndims(O))
    (ndims(O) == 3 && size(O) == (ctx.n, ctx.m, n_obs)) || (ndims(O) == 4 && size(O) == (ctx.n, ctx.m, ctx.E, n_obs)) ||
        throw(DimensionMismatch("O must be (n, m, n_obs) or (n, m, E, n_obs) with the context's n, m and E"))
    1 <= n_obs <= 16 || throw(ArgumentError("observables_jvp: 1 to 16 probes"))
    ydot = Array{ComplexF64}(undef, ctx.N + 1, n_obs, ctx.E)
    Xdf = Array{ComplexF64}(undef, ctx.n, ctx.m, ctx.E)
    GC.@preserve x xdot O ydot Xdf check(ctx, ccall((:grape_eval_jvp, libgrape), Cint,
                                                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}),
                                                    ctx.handle, x, xdot, Int32(n_obs), Int32(ndims(O) == 4 ? 1 : 0), O, ydot, Xdf))
    ydot, Xdf
end

# The ensemble-averaged host forms (grape_eval_observables_mean / _vjp_mean / _jvp_mean): the member axis is summed (or, for the
# cotangent, broadcast) on the device, y_mean[s+1, j] = sum_k v[k] y[s+1, j, k], X_mean = sum_k v[k] X_final[:, :, k].
# v (E): the weights; `nothing`: the ensemble weights the context was given.  O as in `observables`.  The summation order depends
# on E alone (bitwise reproducible; column j of a 16-probe call is the 1-probe call with probe j).  (Written, NOT executed, like
# `observables`; the Python binding makes the same calls and is tested on the GPU.)
function _mean_probes(ctx::GrapeContext, who::String, O::Array{ComplexF64}, v::Union{Nothing,Vector{Float64}})
    n_obs = size(O, ndims(O))
    (ndims(O) == 3 && size(O) == (ctx.n, ctx.m, n_obs)) || (ndims(O) == 4 && size(O) == (ctx.n, ctx.m, ctx.E, n_obs)) ||
        throw(DimensionMismatch("O must be (n, m, n_obs) or (n, m, E, n_obs) with the context's n, m and E"))
    1 <= n_obs <= 16 || throw(ArgumentError("$who: 1 to 16 probes"))
    v === nothing || length(v) == ctx.E || throw(DimensionMismatch("v must have one entry per member"))
    n_obs, Int32(ndims(O) == 4 ? 1 : 0), (v === nothing ? Ptr{Float64}(C_NULL) : pointer(v))
end

"Returns (y_mean (N+1, n_obs), X_mean (n, m), F) with F bit for bit fom_and_gradient!'s."
function observables_mean(ctx::GrapeContext, x::Matrix{Float64}, O::Array{ComplexF64}; v::Union{Nothing,Vector{Float64}} = nothing)
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    n_obs, pm, p_v = _mean_probes(ctx, "observables_mean", O, v)
    y = Array{ComplexF64}(undef, ctx.N + 1, n_obs)
    Xm = Array{ComplexF64}(undef, ctx.n, ctx.m)
    F = Ref{Float64}(NaN)
    GC.@preserve x O v y Xm check(ctx, ccall((:grape_eval_observables_mean, libgrape), Cint,
                                             (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{ComplexF64}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ref{Float64}),
                                             ctx.handle, x, Int32(n_obs), pm, O, p_v, y, Xm, F))
    y, Xm, F[]
end

"The gradient (K, N) of a loss on `observables_mean`'s returns from its cotangents ybar_mean (N+1, n_obs) and Xbar_mean (n, m)
(either may be `nothing`, not both): bit for bit grape_eval_vjp with ybar[:, :, k] = v[k] ybar_mean, component by component."
function observables_vjp_mean(ctx::GrapeContext, x::Matrix{Float64}, O::Array{ComplexF64},
                              ybar_mean::Union{Nothing,Matrix{ComplexF64}}, Xbar_mean::Union{Nothing,Matrix{ComplexF64}};
                              v::Union{Nothing,Vector{Float64}} = nothing)
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    (ybar_mean === nothing && Xbar_mean === nothing) && throw(ArgumentError("observables_vjp_mean: both cotangents are nothing"))
    n_obs, pm, p_v = _mean_probes(ctx, "observables_vjp_mean", O, v)
    ybar_mean === nothing || size(ybar_mean) == (ctx.N + 1, n_obs) || throw(DimensionMismatch("ybar_mean must be (N+1, n_obs)"))
    Xbar_mean === nothing || size(Xbar_mean) == (ctx.n, ctx.m) || throw(DimensionMismatch("Xbar_mean must be (n, m)"))
    p_y = ybar_mean === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(ybar_mean)
    p_X = Xbar_mean === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(Xbar_mean)
    G = Matrix{Float64}(undef, ctx.K, ctx.N)
    GC.@preserve x O v ybar_mean Xbar_mean G check(ctx, ccall((:grape_eval_vjp_mean, libgrape), Cint,
                                                              (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{ComplexF64}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{Float64}),
                                                              ctx.handle, x, Int32(ybar_mean === nothing ? 0 : n_obs), pm,
                                                              ybar_mean === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(O), p_v, p_y, p_X, G))
    G
end

"Returns (ydot_mean (N+1, n_obs), Xdot_mean (n, m)): `observables_jvp`'s tangents summed over the members with v."
function observables_jvp_mean(ctx::GrapeContext, x::Matrix{Float64}, xdot::Matrix{Float64}, O::Array{ComplexF64};
                              v::Union{Nothing,Vector{Float64}} = nothing)
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    size(xdot) == size(x) || throw(DimensionMismatch("xdot must have the shape of x"))
    n_obs, pm, p_v = _mean_probes(ctx, "observables_jvp_mean", O, v)
    ydot = Array{ComplexF64}(undef, ctx.N + 1, n_obs)
    Xdm = Array{ComplexF64}(undef, ctx.n, ctx.m)
    GC.@preserve x xdot O v ydot Xdm check(ctx, ccall((:grape_eval_jvp_mean, libgrape), Cint,
                                                      (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{ComplexF64}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}),
                                                      ctx.handle, x, xdot, Int32(n_obs), pm, O, p_v, ydot, Xdm))
    ydot, Xdm
end

# grape_eval_jvp_device: the same on device memory of the context's GPU (raw device pointers, e.g. of AMDGPU.jl arrays in the
# layouts above; C_NULL for an output that is not wanted, not both), asynchronous on `stream`.  d_x = C_NULL pushes d_xdot forward
# along the trajectory the last device form left in the workspace, without a sweep.
function observables_jvp_device(ctx::GrapeContext, d_x::Ptr{Cvoid}, d_xdot::Ptr{Cvoid}, n_obs::Integer, per_member::Bool,
                                d_O::Ptr{Cvoid}, d_ydot::Ptr{Cvoid}, d_Xdot_final::Ptr{Cvoid}; stream::Ptr{Cvoid} = C_NULL)
    check(ctx, ccall((:grape_eval_jvp_device, libgrape), Cint,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     ctx.handle, d_x, d_xdot, Int32(n_obs), Int32(per_member ? 1 : 0), d_O, d_ydot, d_Xdot_final, stream))
    ctx
end

# grape_eval_gnvp: the weighted Gauss-Newton product J' W J xdot of `observables` in one trajectory pass -- what
# `observables_vjp` returns for ybar = W ydot, Xbar_final = wf Xdot_final of `observables_jvp`, without either array.
# wy: (N+1, n_obs, 3) shared by the members or (N+1, n_obs, E, 3), the last axis the planes rr, ri, ii of a real symmetric 2x2
# block per entry of y (scalar weights: rr = ii = w, ri = 0); wf (E): the weights of the final states; either may be `nothing`,
# not both.  Returns Gn (K, N).  Bounds and a basis are served.  (Written, NOT executed, like `observables_jvp`; the Python
# binding makes the same call and is tested on the GPU.)
function observables_gnvp(ctx::GrapeContext, x::Matrix{Float64}, xdot::Matrix{Float64}, O::Union{Nothing,Array{ComplexF64}},
                          wy::Union{Nothing,Array{Float64}}, wf::Union{Nothing,Vector{Float64}})
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    size(xdot) == size(x) || throw(DimensionMismatch("xdot must have the shape of x"))
    (wy === nothing && wf === nothing) && throw(ArgumentError("observables_gnvp: both weights are nothing"))
    n_obs, pm, wpm = 0, Int32(0), Int32(0)
    if wy !== nothing
        O === nothing && throw(ArgumentError("observables_gnvp: wy needs the probes it belongs to"))
        n_obs = size(O, ndims(O))
        (ndims(O) == 3 && size(O) == (ctx.n, ctx.m, n_obs)) || (ndims(O) == 4 && size(O) == (ctx.n, ctx.m, ctx.E, n_obs)) ||
            throw(DimensionMismatch("O must be (n, m, n_obs) or (n, m, E, n_obs) with the context's n, m and E"))
        1 <= n_obs <= 16 || throw(ArgumentError("observables_gnvp: 1 to 16 probes"))
        size(wy) == (ctx.N + 1, n_obs, 3) || size(wy) == (ctx.N + 1, n_obs, ctx.E, 3) ||
            throw(DimensionMismatch("wy must be (N+1, n_obs, 3) or (N+1, n_obs, E, 3)"))
        pm, wpm = Int32(ndims(O) == 4 ? 1 : 0), Int32(ndims(wy) == 4 ? 1 : 0)
    end
    wf === nothing || length(wf) == ctx.E || throw(DimensionMismatch("wf must have one entry per member"))
    p_O = wy === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(O)
    p_wy = wy === nothing ? Ptr{Float64}(C_NULL) : pointer(wy)
    p_wf = wf === nothing ? Ptr{Float64}(C_NULL) : pointer(wf)
    Gn = Matrix{Float64}(undef, ctx.K, ctx.N)
    GC.@preserve x xdot O wy wf Gn check(ctx, ccall((:grape_eval_gnvp, libgrape), Cint,
                                                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ptr{ComplexF64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                                    ctx.handle, x, xdot, Int32(n_obs), pm, p_O, wpm, p_wy, p_wf, Gn))
    Gn
end

# grape_eval_gnvp_device: the same on device memory of the context's GPU (raw device pointers in the layouts above; C_NULL for
# a weight array that is zero, not both), asynchronous on `stream`.  d_x = C_NULL runs along the trajectory the last device form
# left in the workspace, without a sweep: one call per CG iteration of a Gauss-Newton step.
function observables_gnvp_device(ctx::GrapeContext, d_x::Ptr{Cvoid}, d_xdot::Ptr{Cvoid}, n_obs::Integer, per_member::Bool,
                                 d_O::Ptr{Cvoid}, w_per_member::Bool, d_wy::Ptr{Cvoid}, d_wf::Ptr{Cvoid}, d_Gn::Ptr{Cvoid};
                                 stream::Ptr{Cvoid} = C_NULL)
    check(ctx, ccall((:grape_eval_gnvp_device, libgrape), Cint,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     ctx.handle, d_x, d_xdot, Int32(n_obs), Int32(per_member ? 1 : 0), d_O, Int32(w_per_member ? 1 : 0), d_wy, d_wf,
                     d_Gn, stream))
    ctx
end

# struct grape_gn_options / grape_gn_result (include/grape_hip.h) -- field order and types must match exactly
struct GrapeGnOptions
    lambda::Float64
    cg_rtol::Float64
    cg_max_iter::Int32
    reserved::Int32
end

struct GrapeGnResult
    loss::Float64
    g_norm::Float64
    g_inf::Float64
    residual::Float64
    p_norm::Float64
    predicted::Float64
    cg_iterations::Int32
    status::Int32
end

# grape_gn_step: one Levenberg-Marquardt step of L = 1/2 sum r' W r + 1/2 sum_k wf_k |X_N - Xf_target|^2, r = y - y_target,
# solved on the device: one sweep, one upload, the CG iterations on (J' W J + lambda 1) p = -g along the stored trajectory.
# O, wy, wf as in `observables_gnvp`; y_target (N+1, n_obs, E) comes with wy, Xf_target (n, m, E) with wf, one pair at least.
# Returns (p, g, result::GrapeGnResult) with p, g (K, N).  (Written, NOT executed, like `observables_gnvp`; the Python binding
# makes the same call and is tested on the GPU.)
function gn_step(ctx::GrapeContext, x::Matrix{Float64}, O::Union{Nothing,Array{ComplexF64}},
                 y_target::Union{Nothing,Array{ComplexF64,3}}, wy::Union{Nothing,Array{Float64}},
                 Xf_target::Union{Nothing,Array{ComplexF64,3}}, wf::Union{Nothing,Vector{Float64}};
                 lambda::Float64 = 0.0, cg_iter::Integer = 20, cg_rtol::Float64 = 1e-10)
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    (wy === nothing) == (y_target === nothing) || throw(ArgumentError("gn_step: wy and y_target come together or not at all"))
    (wf === nothing) == (Xf_target === nothing) || throw(ArgumentError("gn_step: wf and Xf_target come together or not at all"))
    (wy === nothing && wf === nothing) && throw(ArgumentError("gn_step: nothing to fit"))
    n_obs, pm, wpm = 0, Int32(0), Int32(0)
    if wy !== nothing
        O === nothing && throw(ArgumentError("gn_step: y_target needs the probes it belongs to"))
        n_obs = size(O, ndims(O))
        (ndims(O) == 3 && size(O) == (ctx.n, ctx.m, n_obs)) || (ndims(O) == 4 && size(O) == (ctx.n, ctx.m, ctx.E, n_obs)) ||
            throw(DimensionMismatch("O must be (n, m, n_obs) or (n, m, E, n_obs) with the context's n, m and E"))
        1 <= n_obs <= 16 || throw(ArgumentError("gn_step: 1 to 16 probes"))
        size(wy) == (ctx.N + 1, n_obs, 3) || size(wy) == (ctx.N + 1, n_obs, ctx.E, 3) ||
            throw(DimensionMismatch("wy must be (N+1, n_obs, 3) or (N+1, n_obs, E, 3)"))
        size(y_target) == (ctx.N + 1, n_obs, ctx.E) || throw(DimensionMismatch("y_target must be (N+1, n_obs, E)"))
        pm, wpm = Int32(ndims(O) == 4 ? 1 : 0), Int32(ndims(wy) == 4 ? 1 : 0)
    end
    if wf !== nothing
        length(wf) == ctx.E || throw(DimensionMismatch("wf must have one entry per member"))
        size(Xf_target) == (ctx.n, ctx.m, ctx.E) || throw(DimensionMismatch("Xf_target must be (n, m, E)"))
    end
    p_O = wy === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(O)
    p_yt = wy === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(y_target)
    p_wy = wy === nothing ? Ptr{Float64}(C_NULL) : pointer(wy)
    p_xt = wf === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(Xf_target)
    p_wf = wf === nothing ? Ptr{Float64}(C_NULL) : pointer(wf)
    opts = Ref(GrapeGnOptions(lambda, cg_rtol, Int32(cg_iter), Int32(0)))
    res = Ref(GrapeGnResult(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, Int32(0), Int32(0)))
    p = Matrix{Float64}(undef, ctx.K, ctx.N)
    g = Matrix{Float64}(undef, ctx.K, ctx.N)
    GC.@preserve x O y_target wy Xf_target wf p g check(ctx, ccall((:grape_gn_step, libgrape), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{ComplexF64}, Ptr{ComplexF64}, Int32, Ptr{Float64}, Ptr{ComplexF64}, Ptr{Float64},
         Ref{GrapeGnOptions}, Ptr{Float64}, Ptr{Float64}, Ref{GrapeGnResult}),
        ctx.handle, x, Int32(n_obs), pm, p_O, p_yt, wpm, p_wy, p_xt, p_wf, opts, p, g, res))
    p, g, res[]
end

# grape_eval_jvp_multi: `observables_jvp` for a block of directions behind ONE evaluation of x.  xdot is (K, N, n_dir) (the
# direction index slowest, 1 <= n_dir <= 8); ydot (N+1, n_obs, E, n_dir) and Xdf (n, m, E, n_dir) are written in place and
# returned.  Slice [:, :, :, d] of either is bit for bit what `observables_jvp` returns for xdot[:, :, d].  (Written, NOT
# executed, like `observables_jvp`; the Python binding makes the same call and is tested on the GPU.)
function eval_jvp_multi!(ydot::Array{ComplexF64,4}, Xdf::Array{ComplexF64,4}, ctx::GrapeContext, x::Matrix{Float64},
                         xdot::Array{Float64,3}, O::Array{ComplexF64})
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    n_dir = size(xdot, 3)
    size(xdot) == (ctx.K, ctx.N, n_dir) || throw(DimensionMismatch("xdot must be (n_controls, n_slices, n_dir)"))
    1 <= n_dir <= 8 || throw(ArgumentError("eval_jvp_multi!: 1 to 8 directions (GRAPE_MAX_JVP_DIRECTIONS)"))
    n_obs = size(O, ndims(O))
    (ndims(O) == 3 && size(O) == (ctx.n, ctx.m, n_obs)) || (ndims(O) == 4 && size(O) == (ctx.n, ctx.m, ctx.E, n_obs)) ||
        throw(DimensionMismatch("O must be (n, m, n_obs) or (n, m, E, n_obs) with the context's n, m and E"))
    1 <= n_obs <= 16 || throw(ArgumentError("eval_jvp_multi!: 1 to 16 probes"))
    size(ydot) == (ctx.N + 1, n_obs, ctx.E, n_dir) || throw(DimensionMismatch("ydot must be (N+1, n_obs, E, n_dir)"))
    size(Xdf) == (ctx.n, ctx.m, ctx.E, n_dir) || throw(DimensionMismatch("Xdf must be (n, m, E, n_dir)"))
    GC.@preserve x xdot O ydot Xdf check(ctx, ccall((:grape_eval_jvp_multi, libgrape), Cint,
                                                    (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Int32, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}),
                                                    ctx.handle, x, Int32(n_dir), xdot, Int32(n_obs), Int32(ndims(O) == 4 ? 1 : 0), O, ydot, Xdf))
    ydot, Xdf
end

# grape_eval_jvp_multi_device: the same on device memory (raw device pointers in the layouts above), asynchronous on `stream`;
# d_x = C_NULL runs along the stored trajectory without a sweep.
function eval_jvp_multi_device!(ctx::GrapeContext, d_x::Ptr{Cvoid}, n_dir::Integer, d_xdot::Ptr{Cvoid}, n_obs::Integer,
                                per_member::Bool, d_O::Ptr{Cvoid}, d_ydot::Ptr{Cvoid}, d_Xdot_final::Ptr{Cvoid};
                                stream::Ptr{Cvoid} = C_NULL)
    check(ctx, ccall((:grape_eval_jvp_multi_device, libgrape), Cint,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     ctx.handle, d_x, Int32(n_dir), d_xdot, Int32(n_obs), Int32(per_member ? 1 : 0), d_O, d_ydot, d_Xdot_final, stream))
    ctx
end

# grape_eval_vjp_multi: the pull-back of `observables` for a block of cotangent sets behind ONE evaluation of x.  ybar is
# (N+1, n_obs, E, n_set) and Xbar (n, m, E, n_set) (the set index slowest, 1 <= n_set <= 8; either may be `nothing` = zero, not
# both); G (K, N, n_set) is written in place and returned.  Slice [:, :, r] is bit for bit what grape_eval_vjp returns for
# set r alone.  (Written, NOT executed, like `eval_jvp_multi!`; the Python binding makes the same call and is tested on the GPU.)
function eval_vjp_multi!(G::Array{Float64,3}, ctx::GrapeContext, x::Matrix{Float64}, O::Union{Nothing,Array{ComplexF64}},
                         ybar::Union{Nothing,Array{ComplexF64,4}}, Xbar::Union{Nothing,Array{ComplexF64,4}})
    size(x) == (ctx.K, ctx.N) || throw(DimensionMismatch("x must be (n_controls, n_slices)"))
    (ybar === nothing && Xbar === nothing) && throw(ArgumentError("eval_vjp_multi!: ybar and Xbar are both nothing"))
    n_set = ybar === nothing ? size(Xbar, 4) : size(ybar, 4)
    1 <= n_set <= 8 || throw(ArgumentError("eval_vjp_multi!: 1 to 8 cotangent sets (GRAPE_MAX_VJP_COTANGENTS)"))
    n_obs = 0
    if ybar !== nothing
        O === nothing && throw(ArgumentError("eval_vjp_multi!: ybar needs the probes it belongs to"))
        n_obs = size(O, ndims(O))
        (ndims(O) == 3 && size(O) == (ctx.n, ctx.m, n_obs)) || (ndims(O) == 4 && size(O) == (ctx.n, ctx.m, ctx.E, n_obs)) ||
            throw(DimensionMismatch("O must be (n, m, n_obs) or (n, m, E, n_obs) with the context's n, m and E"))
        1 <= n_obs <= 16 || throw(ArgumentError("eval_vjp_multi!: 1 to 16 probes"))
        size(ybar) == (ctx.N + 1, n_obs, ctx.E, n_set) || throw(DimensionMismatch("ybar must be (N+1, n_obs, E, n_set)"))
    end
    Xbar === nothing || size(Xbar) == (ctx.n, ctx.m, ctx.E, n_set) || throw(DimensionMismatch("Xbar must be (n, m, E, n_set)"))
    size(G) == (ctx.K, ctx.N, n_set) || throw(DimensionMismatch("G must be (n_controls, n_slices, n_set)"))
    per_member = (n_obs > 0 && ndims(O) == 4) ? 1 : 0
    p_O = n_obs > 0 ? pointer(O) : Ptr{ComplexF64}(C_NULL)
    p_y = ybar === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(ybar)
    p_X = Xbar === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(Xbar)
    GC.@preserve x O ybar Xbar G check(ctx, ccall((:grape_eval_vjp_multi, libgrape), Cint,
                                                  (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Int32, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{Float64}),
                                                  ctx.handle, x, Int32(n_set), Int32(n_obs), Int32(per_member), p_O, p_y, p_X, G))
    G
end

# grape_eval_vjp_multi_device: the same on device memory (raw device pointers in the layouts above), asynchronous on `stream`;
# d_x = C_NULL pulls back along the stored trajectory without a sweep.
function eval_vjp_multi_device!(ctx::GrapeContext, d_x::Ptr{Cvoid}, n_set::Integer, n_obs::Integer, per_member::Bool,
                                d_O::Ptr{Cvoid}, d_ybar::Ptr{Cvoid}, d_Xbar_final::Ptr{Cvoid}, d_G::Ptr{Cvoid};
                                stream::Ptr{Cvoid} = C_NULL)
    check(ctx, ccall((:grape_eval_vjp_multi_device, libgrape), Cint,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     ctx.handle, d_x, Int32(n_set), Int32(n_obs), Int32(per_member ? 1 : 0), d_O, d_ybar, d_Xbar_final, d_G, stream))
    ctx
end

# grape_set_trajectory_derivative: :first_order (default) or :exact -- observables_vjp / observables_jvp, their device forms and
# the reuse forms then use the Frechet derivative of the sweep's own expm evaluation per slice instead of (-i dt B) P
function set_trajectory_derivative!(ctx::GrapeContext, mode::Symbol)
    mode in (:first_order, :exact) || throw(ArgumentError("mode must be :first_order or :exact"))
    check(ctx, ccall((:grape_set_trajectory_derivative, libgrape), Cint, (Ptr{Cvoid}, Int32), ctx.handle, Int32(mode == :exact ? 1 : 0)))
    ctx
end

# grape_set_running_cost_derivative: :first_order (default) or :exact -- the J part of every gradient then uses the Frechet
# derivative of the sweep's own expm evaluation per slice; contexts created with gradient = exact take a running cost in the
# exact mode only (set it before set_running_cost!)
function set_running_cost_derivative!(ctx::GrapeContext, mode::Symbol)
    mode in (:first_order, :exact) || throw(ArgumentError("mode must be :first_order or :exact"))
    check(ctx, ccall((:grape_set_running_cost_derivative, libgrape), Cint, (Ptr{Cvoid}, Int32), ctx.handle, Int32(mode == :exact ? 1 : 0)))
    ctx
end

"The kernels the last evaluation launched, in launch order (grape_get_kernel_names, ABI v4)."
function kernel_names(ctx::GrapeContext)
    need = ccall((:grape_get_kernel_names, libgrape), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint), ctx.handle, C_NULL, 0)
    need > 0 || return String[]
    buf = Vector{UInt8}(undef, need)
    ccall((:grape_get_kernel_names, libgrape), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint), ctx.handle, buf, need)
    filter(!isempty, split(unsafe_string(pointer(buf)), ';'))
end

"Accepted step length and cumulative evaluation count of every iteration of the last `grape_lbfgs` run (ABI v5)."
function lbfgs_trace(ctx::GrapeContext)
    n = Ref{Int32}(0)
    check(ctx, ccall((:grape_lbfgs_get_trace, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Int32}),
                     ctx.handle, C_NULL, C_NULL, 0, n))
    alphas, evals = Vector{Float64}(undef, n[]), Vector{Int32}(undef, n[])
    check(ctx, ccall((:grape_lbfgs_get_trace, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Int32}),
                     ctx.handle, alphas, evals, n[], n))
    alphas, evals
end

"""
One process per GPU without librccl (ABI v4): `allgather` is any function that returns every rank's 64 bytes in rank
order as one `Vector{UInt8}` (e.g. `h -> MPI.Allgather(h, comm)`).  Afterwards `fom_and_gradient!` on every rank returns
the full-ensemble F and G: the ranks' rows meet in mailboxes in device memory (src/solve.jl:171-191's sum).
"""
function attach_ipc!(ctx::GrapeContext, rank::Integer, nranks::Integer, allgather)
    h = Vector{UInt8}(undef, 64)
    check(ctx, ccall((:grape_ipc_export, libgrape), Cint, (Ptr{Cvoid}, Cint, Ptr{UInt8}), ctx.handle, nranks, h))
    all = allgather(h)
    length(all) == 64 * nranks || error("attach_ipc!: allgather must return 64 * nranks bytes")
    check(ctx, ccall((:grape_ipc_attach, libgrape), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint), ctx.handle, all, rank, nranks))
    ctx
end

# the (F, G, x) protocol of Optim.only_fg!, as in src/solve.jl:94-99 and :189-195
function make_topt(ctx::GrapeContext)
    (F, G, x) -> begin
        fom = fom_and_gradient!(ctx, G, x; want_F = F !== nothing)
        F !== nothing ? fom : nothing
    end
end

function solve(prob::Problem, alg::Union{GRAPE_HIP,ADGRAPE_HIP})
    ctx = GrapeContext([prob], [1.0], alg)
    res = Optim.optimize(Optim.only_fg!(make_topt(ctx)), prob.guess, Optim.LBFGS(), alg.optim_options)   # src/solve.jl:138
    SolutionResult(res, res.minimum, res.minimizer, prob, alg)                                            # src/solve.jl:139
end

function solve(ens::EnsembleProblem, alg::Union{GRAPE_HIP,ADGRAPE_HIP})
    members = init_ensemble(ens)                                                                          # src/solve.jl:150
    ctx = GrapeContext(members, Vector{Float64}(ens.wts), alg)
    res = Optim.optimize(Optim.only_fg!(make_topt(ctx)), members[1].guess, Optim.LBFGS(), alg.optim_options)  # :244
    EnsembleSolutionResult(res, res.minimum, res.minimizer, ens, alg)                                     # :245
end

end # module
