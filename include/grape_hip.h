/*
 * grape_hip.h -- C ABI of libgrape_hip.so, the MI355X (gfx950) GRAPE propagator/gradient
 * engine that replaces the body of the (F, G, x) closure QuOptimalControl.jl hands to Optim.
 *
 * The reference has no FFI of its own (pure Julia); the seam is the closure `topt` built in
 *   solve(::Problem, ::GRAPE)          /root/reference/src/solve.jl:63-143  (closure :75-100)
 *   solve(::EnsembleProblem, ::GRAPE)  /root/reference/src/solve.jl:145-250 (closure :164-196)
 * whose body is  _fom_and_gradient_GRAPE!  (src/GRAPE.jl:25-96)  looped over the ensemble.
 * Each entry point below names the reference code it stands in for.  INTEGRATION.md shows the
 * Julia `ccall` glue (julia/GrapeHIP.jl) and the Python ctypes binding that mirror it.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types.  Every function returns a grape_status
 *     (0 = OK, negative = error); grape_last_error() gives the message.  No exceptions cross.
 *   - complex numbers are interleaved {re, im} doubles == Julia ComplexF64 == double _Complex.
 *   - matrices are column-major (Julia): element (i,j) of an n x n matrix at i + j*n.
 *   - x and G are (K, N) column-major Float64: x[j,i] at j + i*K  (what Optim hands in/out).
 *   - host-pointer arguments are only read/written during the call; the library keeps no
 *     caller pointer after return (Julia: GC.@preserve for the duration of the ccall).
 *   - every entry point selects the device(s) of its context and restores the calling thread's current HIP device before
 *     it returns (a host framework in the same thread keeps allocating and launching where it was).
 *   - one evaluation in flight per context (like the reference's closure, which shares one
 *     evolve_store, src/solve.jl:162); distinct contexts are independent.
 */
#ifndef GRAPE_HIP_H
#define GRAPE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRAPE_ABI_VERSION 8

typedef enum grape_status {
    GRAPE_OK = 0,
    GRAPE_ERR_INVALID_ARG = -1,   /* null pointer, non-positive size, bad enum           */
    GRAPE_ERR_UNSUPPORTED = -2,   /* operator dimension / option this build has no kernel for */
    GRAPE_ERR_NO_DEVICE = -3,     /* no HIP device / wrong architecture                 */
    GRAPE_ERR_HIP = -4,           /* a HIP runtime call failed (message has the detail) */
    GRAPE_ERR_NOT_READY = -5,     /* grape_eval before grape_set_operators              */
    GRAPE_ERR_ALLOC = -6,         /* host or device allocation failed                   */
    GRAPE_ERR_TIMEOUT = -7,       /* the device did not finish an evaluation within the time limit
                                     (GRAPE_EVAL_TIMEOUT_S, default 600 s): device presumed hung */
    GRAPE_ERR_COMM = -8           /* RCCL could not be loaded / a collective call failed */
} grape_status;

/* src/problems.jl:8-10.  CoherenceTransfer dispatches exactly like StateTransfer
 * (src/GRAPE.jl:197,236,276,294; src/cost_functions.jl:104). */
typedef enum grape_sys_type {
    GRAPE_UNITARY_GATE = 0,
    GRAPE_STATE_TRANSFER = 1,
    GRAPE_COHERENCE_TRANSFER = 2
} grape_sys_type;

/* GRAPE(isinplace=true)  -> _fom_and_gradient_GRAPE!  (src/GRAPE.jl:25-96):   H = (sum_j B_j x_j) + A,
 *                           UnitaryGate gradient sign +i (src/GRAPE.jl:272)
 * GRAPE(isinplace=false) -> _fom_and_gradient_sGRAPE  (src/GRAPE.jl:103-166): H = A + sum_j B_j x_j,
 *                           UnitaryGate gradient sign -i (src/GRAPE.jl:290) */
typedef enum grape_variant {
    GRAPE_VARIANT_INPLACE = 0,
    GRAPE_VARIANT_STATIC = 1
} grape_variant;

enum {
    GRAPE_FLAG_KEEP_COSTATES = 1 << 0,  /* debug: also store every costate L_t so that
                                           grape_get_trajectory can return them         */
    GRAPE_FLAG_TIME_KERNELS = 1 << 1,   /* record HIP events around the sweep kernel of every
                                           evaluation (see grape_get_kernel_time)       */
    GRAPE_FLAG_PHASE_STAMPS = 1 << 2,   /* diagnostic build of the sweep: every wave stamps the
                                           shader clock at its phase boundaries
                                           (see grape_get_phase_stamps); never for timing runs */
    GRAPE_FLAG_MEMBER_RESULTS = 1 << 4, /* also leave every member's unweighted (F_k, g_k) in HBM for
                                           grape_get_member_results (the reference's
                                           gradient[k,:,:] intermediate); off by default: F and G
                                           do not need it and it costs E*(K*N+1) doubles of writes */
    GRAPE_FLAG_FORCE_GENERAL = 1 << 3,  /* always use the general data flow (forward states stored
                                           in HBM, as the reference does), even when every
                                           generator is Hermitian and the cheaper unitary flow
                                           applies.  KEEP_COSTATES implies it.          */
    GRAPE_FLAG_TIME_SAMPLED = 1 << 6,   /* with TIME_KERNELS: record the event pair on every 8th evaluation only
                                           (an event pair costs ~5 us of a ~90 us host->host call)  */
    GRAPE_FLAG_GROUP_PEER_SUM = 1 << 7, /* multi-device contexts (n_devices >= 2): sum the shards' [G, F] on the first device
                                           through peer copies and one reduction kernel (fixed shard order) instead of the
                                           RCCL all-reduce; librccl is not loaded, and device_ids may repeat a device
                                           (several shards on one GPU: the way the sharding logic is tested on a one-GPU
                                           machine)                                                                    */
    GRAPE_FLAG_FORCE_COLLECTIVE = 1 << 5 /* create the RCCL communicator and run the all-reduce of
                                           [G, F] even when the context spans ONE device (a
                                           1-rank collective: exercises the multi-GPU code path
                                           on a single-GPU machine; testing/diagnostics)  */
};

#define GRAPE_MAX_DEVICES 8

/* Mirrors what solve() unpacks: Problem fields (src/problems.jl:19-28: sys_type, T,
 * n_controls), the integrator's n_slices (src/timeevolution.jl:11-14), EnsembleProblem.n_ens
 * (src/problems.jl:33-41) -- the members this context owns: the whole ensemble for a
 * single-process caller (the library shards it over `n_devices` GPUs itself), or this rank's
 * shard when one process per GPU is used with grape_comm_attach. */
typedef struct grape_config {
    int32_t sys_type;          /* grape_sys_type                                     */
    int32_t variant;           /* grape_variant                                      */
    int32_t n;                 /* operator dimension (d, or d*d for Liouvillians): any n >= 1 (ABI v5; src/GRAPE.jl:25-96 is
                                  size-generic).  n = 2..4 run in registers, 5..32 and 33..64 on the FP64 matrix cores, n = 1 and
                                  n > 64 (up to 2048) through a plain size-generic kernel: correct, not fast */
    int32_t n_controls;        /* K                                                  */
    int32_t n_slices;          /* N                                                  */
    int32_t n_ensemble;        /* E owned by this context (1 for a plain Problem)    */
    double  duration;          /* T                                                  */
    int32_t device;            /* HIP device ordinal, -1 = current device            */
    int32_t flags;             /* GRAPE_FLAG_*                                       */
    /* tuning; 0 = choose automatically */
    int32_t slices_per_lane;   /* S: consecutive time slices one lane owns           */
    int32_t waves_per_member;  /* W: wavefronts that share one member's time axis    */
    int32_t expm_squarings;    /* <0 = per slice from the generator norm; >=0 forces s */
    int32_t max_batch;         /* control arrays one grape_eval_batch call may carry; 0 or 1 = no batching */
    /* ---- ABI v2 ---- */
    int32_t n_state_cols;      /* m: Xi, Xt are n x m (src/problems.jl:23-24 puts no constraint on the
                                  shape); 0 = n (square, every reference test).  m < n (e.g. m = 1,
                                  vectorised density matrices as in test/liou.jl:38-48) needs UnitaryGate */
    int32_t n_devices;         /* 0 or 1: one GPU (`device`).  2..8: the ensemble axis is sharded inside the
                                  library over device_ids[0..n_devices) in contiguous blocks of ceil(E/G)
                                  members (src/solve.jl:166-187 is the loop being split) and every
                                  evaluation ends in ONE RCCL all-reduce of the K*N+1 doubles [G, F]
                                  (src/solve.jl:171-186, :191) */
    int32_t device_ids[GRAPE_MAX_DEVICES];   /* HIP ordinals, used when n_devices >= 2 */
    int32_t gradient;          /* grape_gradient: 0 = the reference's first-order grad_func! (src/GRAPE.jl:261-303),
                                  1 = exact derivative of the objective (what ADGRAPE gets from Zygote,
                                  src/GRAPE.jl:12-20; cf. expm_exact_gradient, src/grape_tools.jl:26-57); 2 <= n <= 64.  Runs behind the
                                  debug flow (every X_t, L_t stored: grape_get_trajectory returns them), except for
                                  UnitaryGate problems with Hermitian generators at n = 2 or 4 (the lane-pair kernel),
                                  which take the unitary flow (grape_info.unitary_flow = 1, states_stored = 0:
                                  grape_get_trajectory serves propagators only) unless GRAPE_FLAG_KEEP_COSTATES is set */
    int32_t objective;         /* grape_objective: 0 = fom_func (src/cost_functions.jl:99-111),
                                  1 = the ADGRAPE functional C1(Xt, U Xi [U']) for every system type
                                  (src/solve.jl:268-291, :317-361); needs gradient = 1 */
} grape_config;

typedef enum grape_gradient { GRAPE_GRADIENT_REFERENCE = 0, GRAPE_GRADIENT_EXACT = 1 } grape_gradient;
typedef enum grape_objective { GRAPE_OBJECTIVE_FOM = 0, GRAPE_OBJECTIVE_C1 = 1 } grape_objective;

typedef struct grape_info {
    int32_t abi_version;
    int32_t device;
    int32_t compute_units;
    int32_t slices_per_lane;       /* S in use                                          */
    int32_t waves_per_member;      /* W in use                                          */
    int32_t expm_squarings;        /* forced s, or -1 = per slice from the generator norm */
    int32_t kernel_family;         /* 0 = register-resident small-n, 1 = LDS/MFMA tile (n = 5..64), 2 = size-generic (n = 1, n > 64) */
    int32_t unitary_flow;          /* 1 after grape_set_operators found every A_k, B_jk Hermitian
                                      (propagators unitary): no forward-state round trip  */
    double  expm_theta;            /* norm threshold below which no scaling/squaring is done */
    uint64_t workspace_bytes;      /* device bytes owned by the context                 */
    char    arch[32];              /* gcnArchName of the device                         */
    /* ---- ABI v2 ---- */
    int32_t n_devices;             /* GPUs this context spans (in-library sharding)      */
    int32_t comm_size;             /* ranks of the RCCL communicator the all-reduce runs on (1 = none) */
    int32_t comm_rank;
    int32_t members_first_device;  /* members owned by device_ids[0] (the largest shard)  */
    int32_t lane_pair;             /* 1: the lane-pair small-n kernel (two lanes per time chunk, two waves per SIMD) */
    int32_t states_stored;         /* 1: grape_get_trajectory can return the forward states (after set_operators);
                                      0: the flow in use rebuilds them on the fly -- ask for GRAPE_FLAG_KEEP_COSTATES */
    int32_t rank_one_chain;        /* 1 after grape_set_operators found rank-one states (Xi = v v', Xt = w w' under the
                                      sandwich, or n x 1 states) where a vector flow exists: n = 9..16; n = 5..8 and 17..32
                                      with member-invariant controls on large ensembles; n = 33..64 with sparse control
                                      operators: the sweeps run on vectors; GRAPE_FLAG_FORCE_GENERAL keeps the dense chain */
    int32_t sparse_controls;       /* 1: every control operator has at most 64 non-zeros (Pauli-type controls; up to 256 --
                                      sums of a few Pauli strings, global drives -- where the longer lists pay) and the
                                      kernels that support it read (coefficient, position) lists instead of dense
                                      operators for the gradient traces */
    int32_t fused_forward;         /* rank-one chain, single evaluations: 1 when the forward vector pass runs inside the
                                      expm kernel (ensembles of at least 2 x compute_units members), so every propagator is
                                      read from HBM once instead of twice */
    int32_t time_chunks;           /* n = 5..32, fewer members than wavefront slots: the time axis
                                      of every member is cut into this many chunks evaluated in parallel (0 = one
                                      wavefront walks all slices) */
    /* ---- ABI v3 ---- */
    int32_t hoisted_controls;      /* 1 after grape_set_operators found the control operators B_c identical for every
                                      member (B_gens = k -> [Sx, Sy], test/setup_tests.jl:32) in the n = 5..32 family:
                                      the control sum sum_c x[c,t] B_c of src/timeevolution.jl:105-107 is formed once per
                                      slice and evaluation instead of once per (member, slice) */
    int32_t expm_action;           /* 1: rank-one states (rank_one_chain) on an ensemble that fills the device, with control
                                      operators shared by the members (n = 5..32) or up to six of the members' own
                                      (n <= 16): exp(G_t) is applied to the two chains' vectors by its
                                      Taylor series (matrix-vector products only); no propagator is formed, so
                                      grape_get_trajectory has none to return -- GRAPE_FLAG_KEEP_COSTATES keeps the dense flow */
    int32_t prop_chain;            /* 1: rank-one states (rank_one_chain), 9 <= n <= 16, ensembles below expm_action's threshold
                                      (down to one problem): the expm kernel stores P_t and P_t^T and both vector chains run on
                                      them with one matrix-vector product per slice (chain_prop_kernel); with time_chunks >= 2
                                      on a chunked time axis (a workgroup per member and chunk) */
    /* ---- ABI v5 ---- */
    int32_t member_chunk;          /* members the workspace arrays (P_t, X_t, L_t) hold at a time: n_ensemble when everything
                                      fits, fewer when the ensemble's workspace exceeds 0.9 x the free device memory (or
                                      GRAPE_MAX_WORKSPACE_BYTES): an evaluation then walks the ensemble in blocks of this
                                      many members (src/solve.jl:166-187 is a serial loop with no such limit) -- same
                                      results bit for bit; grape_get_trajectory is not available on such a context */
    int32_t pair_antiherm;         /* (the slot ABI v5 reserved; 0 before) 1: lane_pair, unitary_flow, n = 4, UnitaryGate, first-order
                                      gradient -- the backward sweep carries only the anti-Hermitian part of z M_t, all that the
                                      gradient traces see of it (GRAPE_PAIR_AH=0 in the environment at grape_create: the full M_t) */
    /* ---- ABI v6 ---- */
    uint64_t workspace_budget_bytes; /* what the workspace arrays may take: 0.9 x the device memory free at grape_create minus the
                                      other buffers, or GRAPE_MAX_WORKSPACE_BYTES -- with member_chunk, what makes a run's
                                      chunk plan reproducible on another device / another day */
    int32_t scaled_controls;       /* 1 after grape_set_operators found the members' control operators to be member 0's times one
                                      real factor per member, B_{k,c} = s_k B_{0,c} (EnsembleProblem.B_g with amplitude
                                      inhomogeneity, src/problems.jl:33-41): the flows built on the per-slice control sum keep
                                      it (hoisted_controls = 1) and every member scales it by its s_k */
    int32_t propagator_blocks;     /* kernel_family 2, n >= 17: workgroups per member of the propagator launch (1: one launch
                                      forms the propagators and walks the chain) */
} grape_info;

/* Opaque RCCL bootstrap token (ncclUniqueId), see grape_comm_unique_id / grape_comm_attach. */
typedef struct grape_comm_id {
    char bytes[128];
} grape_comm_id;

/* Opaque handle of a rank's exchange mailbox (hipIpcMemHandle_t), see grape_ipc_export / grape_ipc_attach. */
typedef struct grape_ipc_handle {
    char bytes[64];
} grape_ipc_handle;

typedef struct grape_ctx grape_ctx;

/* ABI version of the loaded library (== GRAPE_ABI_VERSION of the header it was built from). */
int grape_abi_version(void);

/* Replaces init_GRAPE (src/grape_tools.jl:4-16) + init_ensemble's allocation
 * (src/tools.jl:42-53): creates the device workspace (propagators, forward states,
 * per-member gradients) for the given shape.  *out is NULL on failure. */
int grape_create(const grape_config *cfg, grape_ctx **out);

/* Frees everything the context owns (Julia: finalizer). NULL is accepted. */
int grape_destroy(grape_ctx *ctx);

/* One process per GPU (the layout torch.distributed / MPI launchers produce): every rank creates a
 * context for ITS contiguous member shard, rank 0 calls grape_comm_unique_id and ships the 128
 * bytes to the other ranks by any means, then every rank calls grape_comm_attach.  From then on
 * each grape_eval / grape_eval_device on that context ends in the one all-reduce(sum) of
 * [G, F] over the ranks (RCCL over xGMI, enqueued on the evaluation's own stream) that completes
 * src/solve.jl:171-191, so every rank returns the full-ensemble F and G.  Collective: all ranks
 * must call grape_comm_attach, and later the evaluations, in the same order.
 * librccl is loaded lazily (dlopen) by these two calls and by multi-device contexts only. */
int grape_comm_unique_id(grape_comm_id *out);
int grape_comm_attach(grape_ctx *ctx, const grape_comm_id *id, int32_t rank, int32_t n_ranks);

/* ABI v4.  The same one-process-per-GPU layout WITHOUT librccl: the K*N+1 doubles of src/solve.jl:171-191's sum travel
 * through mailboxes in device memory that the ranks open in each other through HIP IPC.  Every rank calls
 * grape_ipc_export(ctx, n_ranks, &h) (allocates its mailbox, returns 64 opaque bytes), the ranks exchange the handles by any
 * means (all-gather over the launcher's control plane), then every rank calls grape_ipc_attach(ctx, handles[n_ranks], rank,
 * n_ranks).  From then on grape_eval / grape_eval_device / grape_lbfgs on that context end in ipc_allreduce_kernel: each rank
 * stores its row into its slot of every rank's mailbox (one hop over xGMI), waits -- bounded -- until its own mailbox holds
 * all n_ranks rows, sums them in rank order (bitwise the sum every other rank, and an in-process group with the same
 * shards, gets) and publishes to its host as a single-GPU evaluation does.  A rank that never shows up turns into
 * GRAPE_ERR_COMM on the others after GRAPE_EVAL_TIMEOUT_S (5 s at least, 120 s at most), never into a hang.  The blocking
 * entry points return that code themselves; the device-pointer entry points (grape_eval_device, grape_eval_batch_device, the
 * evaluations inside grape_lbfgs) cannot -- for them an exchange that gave up writes NaN over [G, F] (never a partial sum)
 * and sets a host-visible word: grape_lbfgs stops with GRAPE_ERR_COMM at its next wait, and every later call on the context
 * returns GRAPE_ERR_COMM (the peers are out of step: the context is retired).  Ranks may share
 * a GPU (tests).  n_ranks <= 8; mutually exclusive with grape_comm_attach; collective like it. */
int grape_ipc_export(grape_ctx *ctx, int32_t n_ranks, grape_ipc_handle *out);
int grape_ipc_attach(grape_ctx *ctx, const grape_ipc_handle *handles, int32_t rank, int32_t n_ranks);

/* Uploads the per-member operators once -- what init_ensemble (src/tools.jl:42-53) produces by
 * calling A_g(k), B_g(k), XiG(k), XtG(k), packed contiguously by the glue:
 *   A  c128 (n,n,E)     B  c128 (n,n,K,E)     Xi, Xt  c128 (n,m,E)     wts  f64 (E)
 * (wts: EnsembleProblem.wts, src/problems.jl:40; pass {1.0} for a plain Problem). */
int grape_set_operators(grape_ctx *ctx, const double *A, const double *B, const double *Xi,
                        const double *Xt, const double *wts);

/* ABI v7.  Control penalties of the reference's cost library, src/cost_functions.jl:29-39 (C3, C4) combined as
 * PenaltyFunctionals does (:66-69), added to the objective of every evaluation on this context:
 *   F_tot = F + sum_c amp_w[c] sum_t x[c,t]^2 + sum_c var_w[c] sum_{t<N-1} (x[c,t+1] - x[c,t])^2
 *   G_tot[c,t] = G[c,t] + 2 amp_w[c] x[c,t] + 2 var_w[c] ([t>0](x[c,t] - x[c,t-1]) - [t<N-1](x[c,t+1] - x[c,t]))
 * amp_w, var_w: host f64[K] (K = n_controls), each nullable (NULL: that term off; both NULL or all weights 0: no penalty,
 * and the evaluation is exactly the one without this call).  The penalty belongs to the pulse, not to a member: it is not
 * scaled by the ensemble weights, it is added ONCE per control array (grape_eval_batch: every array its own), and it
 * does not enter grape_get_member_results.  grape_eval, grape_eval_device, the batched forms and grape_lbfgs (whose
 * minimum and g_norm are then those of F_tot) all return the penalised [G, F].
 * Weights must be finite and >= 0; otherwise GRAPE_ERR_INVALID_ARG and the previous weights stay in force.  Valid any
 * time after grape_create, before or after grape_set_operators (the weights persist across it); ordered behind an
 * in-flight grape_eval_device as grape_set_operators is.  Multi-device contexts add the penalty once, on the first
 * device.  With grape_comm_attach / grape_ipc_attach only rank 0 adds it to its row before the exchange: every rank calls
 * grape_set_penalties with the same weights, just as every rank passes the same x. */
int grape_set_penalties(grape_ctx *ctx, const double *amp_w, const double *var_w);

/* Running costs on the intermediate states: the trajectory functionals of the reference's cost library,
 * src/cost_functions.jl:44-61 -- C5 (occupation of forbidden states), C6 (evolution time, target gate), C7 (evolution time,
 * target state) -- in one shared form.  Additive to ABI v8.
 *   R    host c128 (n, m, E, n_terms) column-major   probe matrices, one per member and term
 *   rho  host f64  (N, n_terms)                      slice weights; entry [s-1, j] weights the state AFTER s slices
 *   n_terms = 0 or R == NULL: off.  1 <= n_terms <= 4.
 * With X_{k,s} member k's state after s slices (X_{k,0} = Xi_k) and y_{k,j,s} = tr(R_{k,j}' X_{k,s}):
 *   J(x)        = sum_k w_k sum_j sum_{s=1..N} rho[s-1,j] |y_{k,j,s}|^2
 *   F_tot       = F + J                      (then the penalties, then the basis projection, as without it)
 *   G_tot[c,t]  = G[c,t] + sum_k w_k sum_j 2 Re tr( Lam_{k,j,t+1}' (-i dt B_{k,c}) X_{k,t+1} ),   t = 0..N-1
 *   Lam_{k,j,N} = rho[N-1,j] y_{k,j,N} R_{k,j}
 *   Lam_{k,j,s} = P_{k,s}' Lam_{k,j,s+1} + rho[s-1,j] y_{k,j,s} R_{k,j}      (P_{k,s}: the propagator taking X_s to X_{s+1})
 * This is the derivative of J with dP_t/dx[c,t] replaced by (-i dt) B_c P_t: FIRST ORDER in dt, the same order as the
 * reference's grad_func! (src/GRAPE.jl:261-303) that G itself follows.  The EXACT gradient of J is a setting of the context:
 * grape_set_running_cost_derivative(ctx, GRAPE_TRAJ_EXACT), below -- with it a running cost is also served on contexts
 * created with gradient = exact (either objective), which refuse it otherwise.
 * Instances (lambda: the caller's weight):  C5 with forbidden kets psiF_j: R_j = psiF_j (n x 1 states), rho = +lambda;
 * C6: R = Xt, rho = -lambda / (N D^2), the constant +lambda added by the caller;  C7 for pure states held as n x 1 kets
 * under UnitaryGate: R = psiT (|psiT' psi|^2 = tr(rhoT rho)), rho = -lambda / N, plus the constant.
 * Served: kernel family 0 (n = 2, 3, 4), GRAPE_UNITARY_GATE (any m, n x 1 kets included), gradient = 0, objective = 0,
 * Hermitian and non-Hermitian generators, both variants, single-device contexts (member-chunked ones and max_batch > 1
 * included).  Everything else -- other n, StateTransfer / CoherenceTransfer (the sandwich needs a second term), gradient =
 * exact, objective = c1, multi-device contexts, attached communicators or mailboxes (the
 * one-rank communicator of GRAPE_FLAG_FORCE_COLLECTIVE is one) -- is refused with
 * GRAPE_ERR_UNSUPPORTED and a message naming the reason; grape_comm_attach / grape_ipc_attach are refused in the same way
 * while a running cost is set.  Non-finite R or rho, n_terms outside 0..4: GRAPE_ERR_INVALID_ARG.  After any failure the
 * previous setting stays in force.  Valid any time after grape_create, before or after grape_set_operators (it persists
 * across it); ordered behind an in-flight grape_eval_device as grape_set_penalties is.
 * grape_eval, grape_eval_device, the batched forms (every array its own J) and grape_lbfgs return the augmented [G, F];
 * grape_eval_fom takes its fallback (the forward-only kernel stores no propagators) and returns grape_eval's F bit for
 * bit.  grape_get_member_results and the member_F of grape_eval_fom stay WITHOUT J, as they stay without penalties.
 * running_cost_kernel runs behind the sweep of every member block, on its stream, reads the propagators the sweep stored
 * (in the general flow it also stores the forward states: N n m 16 B per member and control array of extra workspace,
 * allocated by the first evaluation), and the members' rows join the ensemble sum in a fixed order: results are bitwise
 * reproducible call to call.  A context that never calls this, or switches it off again, launches exactly the kernels it
 * always did. */
int grape_set_running_cost(grape_ctx *ctx, int32_t n_terms, const double *R, const double *rho);

/* Pulses restricted to a basis (Fourier / CRAB series, splines, Slepians, the impulse response of an AWG filter), with the
 * gradient with respect to the coefficients -- "parameter mode".  Additive to ABI v8.
 *   x[c,t] = x0[c,t] + sum_{m<M} theta[c,m] * phi_b[t,m],   b = (n_bases == 1 ? 0 : c)
 *   phi  host f64 (N, M, n_bases) column-major, phi[t + N*(m + M*b)];  n_bases is 1 (one basis for every control) or K
 *   x0   host f64 (K, N), nullable (NULL = 0);  M = n_params, 1 <= M <= N.  phi == NULL or n_params == 0: basis off.
 * With a basis in force every `x` argument of grape_eval, grape_eval_device, grape_eval_batch, grape_eval_batch_device,
 * grape_eval_fom and grape_lbfgs (x0 and x_min; its vectors are K*M long) is theta, (K, M) column-major theta[c + K*m]
 * (batches (K, M, n_x)), every returned G is (K, M), and d_fg is f64[K*M + 1] per control array:
 *   F(theta) is the F of the physical pulse, the penalties of grape_set_penalties evaluated on the physical x;
 *   G_theta[c,m] = sum_t G_tot[c,t] * phi_b[t,m], G_tot including the penalty gradient.
 * The expansion runs on the device in front of the evaluation (basis_expand_kernel: m ascending, one FMA per term), the
 * projection behind the complete summed row -- after the cross-device sum or exchange, after the penalty -- in a fixed tree
 * over t (basis_project_kernel): results are bitwise reproducible call to call, and F is bit for bit what a context
 * without a basis returns through the device-pointer entry points for the expanded pulse.  grape_get_member_results,
 * grape_get_trajectory and the member_F of grape_eval_fom stay in physical slice space ((K, N) rows, per-slice data).
 * Valid any time after grape_create, before or after grape_set_operators (the basis persists across it); ordered behind an
 * in-flight grape_eval_device as grape_set_operators is.  Non-finite phi or x0, n_params outside 1..N, n_bases other than
 * 1 or K: GRAPE_ERR_INVALID_ARG, and the previous basis stays in force (as after any other failure).  Switching the basis
 * off restores the slice-mode behaviour exactly; a context that never calls this launches the kernels it always did.
 * Multi-device contexts expand once on the first device, in front of the fan-out of x.  With grape_comm_attach /
 * grape_ipc_attach every rank sets the same basis and expands its own copy; every rank projects the exchanged row. */
int grape_set_basis(grape_ctx *ctx, int32_t n_params, int32_t n_bases, const double *phi, const double *x0);

/* The physical pulse of a parameter array, expanded ON THE DEVICE by the kernel the evaluations use:
 *   theta host f64 (K, M)      x host f64 (K, N)
 * Blocking; ordered behind an in-flight grape_eval_device.  Without a basis x = theta ((K, N) both).  With
 * grape_set_bounds in force x is the saturated pulse (of theta's expansion, or of the raw (K, N) array without a basis). */
int grape_get_controls(grape_ctx *ctx, const double *theta, double *x);

/* Smooth amplitude bounds: a pointwise, differentiable map from a raw pulse u to the physical pulse, so that
 * lo_c < x[c,t] < hi_c holds for every finite u and every optimiser of the library works unchanged.  Additive to ABI v8.
 *   lo, hi  host f64[K] each (K = n_controls); both NULL: bounds off
 * For a control with finite lo_c < hi_c, mid = (lo + hi) / 2 and half = (hi - lo) / 2:
 *   x[c,t]   = mid_c + half_c * tanh((u[c,t] - mid_c) / half_c)
 *   s[c,t]   = 1 - tanh^2(...)          (dx/du: 1 at u = mid, so pulses small against half are unchanged to first order)
 *   G_u[c,t] = G_tot[c,t] * s[c,t]
 * A control with lo = -inf and hi = +inf is the identity (s = 1).  Everything else -- a one-sided pair, lo >= hi, NaN, one
 * pointer NULL -- is GRAPE_ERR_INVALID_ARG.  When EVERY control is (-inf, +inf) the call is the same as switching the bounds
 * off: the context behaves exactly like one that never called this (same kernels, same bits).
 * With bounds in force every `x` argument of grape_eval, grape_eval_device, grape_eval_batch, grape_eval_batch_device,
 * grape_eval_fom and grape_lbfgs (x0 and x_min) is the raw u, every returned G is G_u, and F is the F of the physical pulse.
 * The penalties of grape_set_penalties and the running costs of grape_set_running_cost are evaluated on the physical x;
 * their gradients are part of G_tot, in front of the slope.
 * With a basis: expand, saturate, evaluate, ..., slope, project --
 *   x = sat(x0 + theta phi^T),   G_theta[c,m] = sum_t G_tot[c,t] s[c,t] phi_b[t,m]
 * (a bounded Fourier / CRAB pulse; the entry points take theta as grape_set_basis describes).  The saturation is fused into
 * basis_expand_kernel, the slope into basis_project_kernel's multiply-add, whose order does not change; without a basis
 * bounds_saturate_kernel stands in for the upload of x and bounds_slope_kernel is the evaluation's last kernel.  Results
 * are bitwise reproducible call to call, and F is bit for bit what a context without bounds returns through the
 * device-pointer entry points for the pulse grape_get_controls returns.  grape_lbfgs probes as it does in parameter mode
 * (the evaluation does not end in a reduce kernel).  grape_get_controls returns the physical (saturated) pulse;
 * grape_get_member_results, grape_get_trajectory and the member_F of grape_eval_fom stay in physical slice space, without
 * the slope.  The fast path of grape_eval_fom saturates in place of its upload and needs no slope.
 * The slope vanishes in saturation: where tanh has rounded to +-1 (|u - mid| above ~19 half) x is held at the last double
 * inside the interval, s = 0 and the gradient entry is exactly 0 -- a gradient method started there does not move that
 * entry.  Start inside (the Python layer clips a guess to mid +- 0.999 half before it inverts the map).
 * Valid any time after grape_create, before or after grape_set_operators (the bounds persist across it); ordered behind an
 * in-flight grape_eval_device as grape_set_operators is.  After any failure the previous setting stays in force.  Switching
 * the bounds off restores the previous behaviour exactly; a context that never calls this launches the kernels it always
 * did.  Multi-device contexts saturate once on the first device, in front of the fan-out of x.  With grape_comm_attach /
 * grape_ipc_attach every rank sets the same bounds and saturates its own copy; every rank applies the slope to the
 * exchanged row. */
int grape_set_bounds(grape_ctx *ctx, const double *lo, const double *hi);

/* Soft worst case over the ensemble in place of its weighted mean.  Additive to ABI v8.
 *   beta   finite; 0: off (the weighted mean, as ever)
 * With W = sum_k w_k and F_k, g_k the members' unweighted results (what grape_get_member_results returns):
 *   F_beta = (W / beta) log( (1 / W) sum_k w_k exp(beta F_k) )
 *   p_k    = W w_k exp(beta F_k) / sum_j w_j exp(beta F_j)          (sum_k p_k = W)
 *   G_beta = sum_k p_k g_k
 * beta -> 0 gives the mean the library returns without a risk; beta -> +inf gives W max_k F_k, beta -> -inf W min_k F_k.
 * F is whatever the optimisers minimise: for the C1-type objectives (an infidelity) beta > 0 is the soft worst case.  Both
 * signs are accepted.  G_beta is the chain rule applied to the gradient convention of the context: with gradient = exact it
 * is the derivative of F_beta; with the reference's first-order grad_func! it is as exact as G is without a risk.
 * Composition: the penalties of grape_set_penalties are added behind F_beta and G_beta, once, as ever; a basis and bounds sit
 * in front and behind unchanged -- expand / saturate, evaluate, risk-weighted sum, penalty, slope / projection.  grape_eval,
 * grape_eval_device, both batched forms (every array gets its own p), grape_lbfgs (its minimum and g_norm are then those
 * of F_beta) and the F of grape_eval_observables return the risk-weighted [G, F].  grape_eval_fom takes its fallback while a
 * risk is set, as it does under a running cost, and returns grape_eval's F bit for bit; its member_F stays the unweighted
 * F_k and is available on every context while a risk is set.  grape_get_member_results, grape_get_trajectory, y and
 * X_final of grape_eval_observables do not change (a context of n <= 4 without GRAPE_FLAG_MEMBER_RESULTS still answers
 * GRAPE_ERR_NOT_READY to grape_get_member_results: the rows this feature keeps there are private to it).
 * On the device: every kernel family leaves the members' unweighted rows in HBM; risk_weights_kernel (one workgroup per
 * control array) forms M = max beta F_k over the members of positive weight and S = sum_k w_k exp(beta F_k - M) in a
 * fixed tree, writes p and F_beta = (W / beta)(M + log(S / W)); the final reduction sums the rows with p in place of w and
 * puts F_beta in front of the penalty.  No atomics: results are bitwise reproducible call to call, and a member-chunked
 * context returns the unchunked context's bits.  A non-finite F_k makes F and G NaN; a member with w_k = 0 gets p_k = 0.
 * Served: every operator dimension, system type, variant, gradient and objective, max_batch > 1, member-chunked contexts,
 * GRAPE_FLAG_KEEP_COSTATES -- on single-device contexts.  GRAPE_ERR_UNSUPPORTED with the reason in grape_last_error:
 * multi-device contexts; an attached communicator or mailbox (grape_comm_attach / grape_ipc_attach are refused while a risk
 * is set); a running cost in force (grape_set_running_cost with n_terms > 0 is refused while a risk is set: the members'
 * J_k are not in the member rows).  GRAPE_ERR_INVALID_ARG: beta NaN or +-inf; with beta != 0, a negative ensemble weight or
 * W = 0 -- checked here once operators are set, and by grape_set_operators while a risk is in force.
 * Valid any time after grape_create; persists across grape_set_operators; ordered behind an in-flight grape_eval_device
 * like the other settings.  After any failure the previous setting stays.  beta = 0, and a context that never calls this,
 * launch exactly the kernels they always did and return the same bits. */
int grape_set_risk(grape_ctx *ctx, double beta);
/* p: host f64[E], the p_k of the last evaluation (array 0 of a batch).  GRAPE_ERR_NOT_READY before an evaluation with a
 * risk in force. */
int grape_get_risk_weights(grape_ctx *ctx, double *p);

/* The closure body, src/solve.jl:164-196 (E>1) / :75-100 (E=1):
 *   F = sum_k w_k F_k ,  G[c,t] = sum_k w_k g_k[c,t]   with (F_k, g_k) = _fom_and_gradient_GRAPE!.
 * x: host (K,N) f64.  F (nullable): host f64.  G (nullable): host (K,N) f64 -- Optim passes
 * `nothing` for the one it does not need (src/solve.jl:189-195).  Blocks until F/G are written.
 * Non-finite x propagates NaN like the reference (no trapping). */
int grape_eval(grape_ctx *ctx, const double *x, double *F, double *G);

/* Same evaluation with device-resident input/output, asynchronous on `stream`
 * (a hipStream_t; NULL = the default stream):
 *   d_x   device (K,N) f64            d_fg  device f64[K*N + 1] = { G (K,N col-major), F }
 * This is the entry point the multi-GPU host layer uses: each rank evaluates its member shard
 * and a single all-reduce(sum) of d_fg over ranks completes src/solve.jl:171-191.
 * Nothing is synchronised; errors detectable at enqueue time are returned.
 * Stream ordering: the context has ONE workspace.  The library orders a later grape_eval /
 * grape_set_operators behind the last grape_eval_device (event wait), but two grape_eval_device
 * calls on DIFFERENT streams must be ordered by the caller.  Multi-device contexts: d_x and d_fg
 * live on device_ids[0]; the library fans x out to the other devices (peer copies). */
int grape_eval_device(grape_ctx *ctx, const double *d_x, double *d_fg, void *stream);

/* Extension beyond the reference (multi-start optimisation / line-search batches):
 * n_x <= max_batch independent control arrays evaluated against the same ensemble in ONE launch.
 *   x  host f64 (K,N,n_x)      F  host f64[n_x] (nullable)      G  host f64 (K,N,n_x) (nullable)
 * Entry b is exactly what grape_eval(ctx, x[:,:,b]) returns; with n_x = 1 the two calls are the same.
 * Needs grape_config.max_batch >= n_x (the workspace is sized for max_batch control arrays).  ABI v4: multi-device contexts
 * and attached communicators batch too -- every shard evaluates the n_x arrays, their rows cross the devices as one sum.
 * gradient = GRAPE_GRADIENT_EXACT batches as well: the stored trajectory is one control array's, so the arrays run one behind
 * the other on the stream (same results, one call, one completion). */
int grape_eval_batch(grape_ctx *ctx, int32_t n_x, const double *x, double *F, double *G);

/* Device-pointer form: d_x (K,N,n_x), d_fg f64[(K*N + 1) * n_x] = n_x blocks of { G, F }. */
int grape_eval_batch_device(grape_ctx *ctx, int32_t n_x, const double *d_x, double *d_fg, void *stream);

/* ABI v8.  The figure of merit WITHOUT the gradient: src/timeevolution.jl:28-39 (pw_evolve) followed by fom_func
 * (src/cost_functions.jl:99-111, objective = 0) or C1(Xt, U Xi [U']) (src/solve.jl:268-361, objective = 1), summed
 * over the ensemble as src/solve.jl:166-187 does -- for callers that rank pulses by their value: dCRAB / Nelder-Mead
 * (src/dCRAB.jl:13-89), robustness landscapes over a grid of members, multi-start screening.
 *   x         host f64 (K,N,n_x), 1 <= n_x <= max(1, grape_config.max_batch)
 *   F         host f64[n_x]          the value grape_eval / grape_eval_batch return as F (penalties of
 *                                    grape_set_penalties included)
 *   member_F  host f64 (E,n_x), nullable: every member's unweighted F_k (no penalty), member index fastest
 * Valid on EVERY context grape_eval serves (any n, system type, variant, gradient / objective setting, n x m states;
 * member-chunked, multi-device and communicator / mailbox contexts), blocking like grape_eval and ordered behind an
 * in-flight grape_eval_device in the same way.  Collective contexts: all ranks call it together, like grape_eval.
 * Fast path -- single-device contexts without communicator or mailbox in kernel family 0 (n = 2, 3, 4): a forward-only
 *   kernel (fom_lane_kernel / fom_pair_kernel) forms the propagators in registers and multiplies them up; nothing is written
 *   to the propagator / state / costate workspace or to the member-result rows, so grape_get_trajectory,
 *   grape_get_member_results, grape_get_kernel_time and an eval -> fom -> eval sequence behave as if the call had not
 *   happened; grape_get_kernel_names reports the kernels of this call.  It needs no P_t storage: a member-chunked context
 *   is evaluated in one launch, a batch in one launch whatever the workspace holds.  member_F is always available.  The
 *   value agrees with grape_eval's F to rounding (the two flows multiply in different orders), not bit for bit.
 * Fallback -- everywhere else: the full evaluation runs and its F is returned, BITWISE what grape_eval (grape_eval_batch,
 *   entry b) returns for the same x.  member_F then follows grape_get_member_results: available where the rows exist
 *   (n >= 5, or GRAPE_FLAG_MEMBER_RESULTS), otherwise GRAPE_ERR_NOT_READY (the message names GRAPE_FLAG_MEMBER_RESULTS)
 *   before anything runs; with n_x > 1 it is served by running the arrays one after another.
 * Errors as grape_eval: null x or F, n_x out of range -> GRAPE_ERR_INVALID_ARG; before grape_set_operators ->
 * GRAPE_ERR_NOT_READY.  Non-finite x propagates NaN.  Results are bitwise reproducible call to call: the chunk products
 * of a member combine in a tree fixed by the decomposition, the member sum has a fixed order. */
int grape_eval_fom(grape_ctx *ctx, int32_t n_x, const double *x, double *F, double *member_F);

/* ABI v8 (additive).  Expectation values along the trajectory and the final states of every member: what the reference names
 * and leaves undone -- test_pulse, src/tools.jl:32-36 ("simulate the pulse again returning the output so you can check the
 * gate is correct"; its body is `@show "not implemented"`), and visualise_expt_val / visualise_expt_vals,
 * src/visualisation.jl:13-51 (real(tr(op * X_s)) for every slice; commented out).
 *   y[s + (N+1) (j + n_obs k)] = tr(O_kj' X_{k,s}) ,  s = 0..N ,  X_{k,0} = Xi_k
 *   UnitaryGate (n x m states, kets included):   X_{k,s+1} = P_{k,s} X_{k,s}
 *   StateTransfer / CoherenceTransfer:           X_{k,s+1} = P_{k,s} X_{k,s} P_{k,s}'
 *   x          host f64 (K,N): what grape_eval takes -- theta / u with grape_set_basis / grape_set_bounds in force; the
 *              observables are those of the physical pulse
 *   n_obs      0..16 probes (the matrix units of a 4 x 4 state, or the 16 Pauli strings of two qubits, in one call)
 *   O          host c128, column-major: per_member = 0: (n, m, n_obs), shared by the members; per_member = 1:
 *              (n, m, E, n_obs), the layout of R in grape_set_running_cost.  Needed when n_obs > 0
 *   y          host c128 (N+1, n_obs, E), column-major; nullable
 *   X_final    host c128 (n, m, E): X_{k,N}, test_pulse's output; nullable
 *   F          host f64, nullable
 * The call runs ONE evaluation of x, exactly the one grape_eval runs (same kernels, same flow): F is bit for bit grape_eval's
 * F, penalties and running cost included.  Behind the sweep of every member block (and behind the running-cost kernels, if a
 * running cost is set) observe_kernel reads the propagators that sweep stored, walks the states and stores the traces.  It is
 * an evaluation in every other respect too: blocking, ordered behind an in-flight grape_eval_device like grape_eval;
 * afterwards grape_get_member_results, grape_get_trajectory and grape_get_kernel_names refer to it (the names include
 * observe_kernel).  y and X_final do not depend on penalties, running cost or ensemble weights.  Results are bitwise
 * reproducible call to call, and a member-chunked context returns the unchunked context's bits.  A context that never calls
 * this launches the kernels it always did; an eval -> observables -> eval sequence returns the first evaluation's [G, F] bit
 * for bit.
 * Served: kernel family 0 (n = 2, 3, 4), all three system types, both variants, Hermitian and non-Hermitian generators,
 * any m under UnitaryGate, gradient = 0 and objective = 0, single-device contexts without communicator or mailbox --
 * member-chunked contexts, max_batch > 1 (the call takes one array), GRAPE_FLAG_KEEP_COSTATES and forced slices_per_lane /
 * waves_per_member included.
 * Refused before anything runs, GRAPE_ERR_UNSUPPORTED with the reason in the message: n = 1 and n >= 5 ("dimension": those
 * workspaces hold P_t in other layouts or not at all), gradient = exact, objective = c1, multi-device contexts, an attached
 * communicator or mailbox.  GRAPE_ERR_INVALID_ARG: null x; y and X_final both NULL; n_obs outside 0..16; n_obs = 0 with a
 * non-NULL y; n_obs > 0 with a NULL O; per_member other than 0 or 1; a non-finite entry of O ("not finite"; with n_obs > 0 O
 * is read and checked even when y is NULL and the probes go unused).  The context's refusals are checked first.  Before
 * grape_set_operators: GRAPE_ERR_NOT_READY.  After any refusal the context evaluates exactly as before.  Non-finite x
 * propagates NaN. */
int grape_eval_observables(grape_ctx *ctx, const double *x, int32_t n_obs, int32_t per_member, const double *O, double *y,
                           double *X_final, double *F);

/* ABI v8 (additive).  The vector-Jacobian product of the trajectory read-out: the backward of grape_eval_observables.  Any
 * real loss l written on y[s,j,k] = tr(O_kj' X_{k,s}) and on X_final gets its gradient with respect to the controls from
 * the cotangents the caller (or an autograd framework) computes on the host -- no new kernel, no new setting per loss.
 *   x, n_obs, per_member, O   exactly as in grape_eval_observables (x is theta / u with a basis / bounds in force; up to
 *              16 probes; O is (n, m, n_obs), or (n, m, E, n_obs) with per_member = 1)
 *   ybar       host c128 (N+1, n_obs, E), the layout of y; nullable (NULL means zero)
 *   Xbar_final host c128 (n, m, E), the layout of X_final; nullable
 *   G          host f64 (K, N), or (K, M) in parameter mode; required
 * Cotangent convention: ybar = dl/dRe y + i dl/dIm y, Xbar_final likewise entry by entry -- what torch hands to backward for
 * a complex output of a real loss.
 * With the states and propagators of the physical pulse, X_{k,s+1} = P_{k,s} X_{k,s}:
 *   Lam_{k,N} = Xbar_k + sum_j ybar[N,j,k] O_kj
 *   Lam_{k,s} = P_{k,s}' Lam_{k,s+1} + sum_j ybar[s,j,k] O_kj          s = N-1 .. 1
 *   G[c,t]    = sum_k Re tr( Lam_{k,t+1}' (-i dt B_kc) X_{k,t+1} )     t = 0 .. N-1
 * ybar[0,.,.] is read and validated but contributes nothing (X_0 = Xi).  G holds no ensemble weight, penalty, running cost
 * or risk: it is the gradient of the caller's loss alone (the caller puts w_k into l).  The gradient is FIRST ORDER in dt,
 * like the reference's grad_func! and like grape_set_running_cost (the derivative of exp(-i dt H) is taken as -i dt B P);
 * against central differences of a smooth loss on a smooth pulse the deviation falls by ~4 per 4x in N.  The exact
 * derivative is a setting of the context: grape_set_trajectory_derivative(ctx, GRAPE_TRAJ_EXACT), below.
 * With grape_set_bounds and / or grape_set_basis in force G is returned in the coordinates of x: the summed physical row
 * goes through bounds_slope_kernel / basis_project_kernel (the slope of this very evaluation), without the penalty and F
 * that an evaluation's own tail carries -- so grape_eval_observables and this call agree on coordinates.
 * The call runs ONE evaluation of x exactly as the context is configured, as grape_eval_observables does, and discards its
 * [G, F]; behind the sweep of every member block (the running-cost kernels, if any) trajectory_vjp_kernel reads the stored
 * propagators -- one workgroup per member, one lane per time chunk, one pair of backward walks whatever n_obs is -- and
 * vjp_sum_kernel adds the members' rows in a tree fixed by the members' ensemble indices (groups of 32 consecutive members
 * in member order, then the groups in order).  Blocking, ordered behind an in-flight grape_eval_device;
 * afterwards grape_get_kernel_names includes the two kernels.  An eval -> vjp -> eval sequence returns the first
 * evaluation's bits; results are bitwise reproducible call to call; a member-chunked context returns the unchunked
 * context's bits; a standing running cost, penalties or risk do not change G.  The whole ybar is uploaded per call.
 * Served: kernel family 0 (n = 2, 3, 4), GRAPE_UNITARY_GATE with any m (kets included), Hermitian and non-Hermitian
 * generators, both variants, gradient = 0 and objective = 0, single-device contexts without communicator or mailbox --
 * member-chunked contexts, max_batch > 1 (the call takes one array) and forced slices_per_lane / waves_per_member included.
 * Refused before anything runs, GRAPE_ERR_UNSUPPORTED with the reason in the message: n = 1 and n >= 5 ("dimension"),
 * StateTransfer / CoherenceTransfer ("StateTransfer": the sandwich needs a second term), gradient = exact or objective = c1
 * ("exact"), multi-device contexts ("multi-device"), an attached communicator or mailbox ("communicator").
 * GRAPE_ERR_INVALID_ARG: null x or G; ybar and Xbar_final both NULL; n_obs outside 0..16; n_obs = 0 with a non-NULL ybar;
 * n_obs > 0 with a NULL O; per_member other than 0 or 1; a non-finite entry of O, ybar or Xbar_final ("not finite").  The
 * context's refusals are checked first.  Before grape_set_operators: GRAPE_ERR_NOT_READY.  After any refusal the context
 * evaluates exactly as before.  Non-finite x propagates NaN. */
int grape_eval_vjp(grape_ctx *ctx, const double *x, int32_t n_obs, int32_t per_member, const double *O, const double *ybar,
                   const double *Xbar_final, double *G);

/* ABI v8 (additive).  The device forms of the pair above: every array lives in device memory of the context's GPU, nothing
 * crosses to the host, nothing is synchronised -- the read-out and the pull-back for a loss that lives on the GPU (a torch
 * CUDA graph of y, say).  Layouts, the cotangent convention, scope, refusals and argument checks are those of the host forms,
 * word for word (the messages carry the device forms' names):
 *   d_x          what grape_eval_device takes: theta / u with a basis / bounds in force
 *   d_O          c128 (n, m, n_obs), or (n, m, E, n_obs) with per_member = 1
 *   d_y, d_ybar  c128 (N+1, n_obs, E)            d_X_final, d_Xbar_final  c128 (n, m, E)
 *   d_G          f64 (K, N), or (K, M) in parameter mode; required
 *   d_fg         f64 [K cols + 1], nullable: the evaluation's own [G, F], exactly what grape_eval_device writes for d_x -- a
 *                by-product of the read-out (cols = N, or M in parameter mode)
 * Both calls are asynchronous on `stream`, like grape_eval_device, under the same rules: one workspace per context; later
 * blocking calls are ordered behind the call; two device calls on different streams are ordered by the caller; the caller
 * keeps every device array alive until the stream has passed the call.  The kernels write straight into d_y, d_X_final and
 * d_G and read d_O, d_ybar and d_Xbar_final in place: no staging copy is made.  The context's own scratch (the members' rows,
 * the groups' sums, the summed row under a pulse map) grows only behind a pending device call.
 * NON-FINITE ENTRIES OF THE DEVICE ARRAYS ARE NOT CHECKED -- that would take a synchronisation.  A NaN in d_O, d_ybar or
 * d_Xbar_final propagates into y / G, the status stays GRAPE_OK, and the context evaluates as before afterwards.  Everything
 * else the host forms validate is validated the same way, the context's refusals first.
 * Results are bit for bit those of the host forms on the same values.  Two instances of each kernel serve the device forms:
 * the host forms' (observe_kernel, trajectory_vjp_kernel), and a staged one (observe_staged_kernel,
 * trajectory_vjp_staged_kernel) that passes a member's contiguous y / ybar block through LDS so that the global accesses are
 * lane-contiguous; same arithmetic, same order, same bits.  The library picks by the probe count where the block fits the
 * workgroup's LDS; GRAPE_TRAJ_STAGED=0 / 1 forces the choice, grape_get_kernel_names tells which ran.
 * Reuse: grape_eval_vjp_device with d_x = NULL pulls back along "the trajectory of the last grape_eval_observables_device or
 * grape_eval_vjp_device call on this context": no sweep is launched, only trajectory_vjp_kernel, vjp_sum_kernel and the slope /
 * projection tail run, on the propagators and the slope array that evaluation left in the workspace.  The result is bit for
 * bit that of the same call with d_x given.  The context keeps a "trajectory valid" flag: set at the end of a successful call
 * of either device form with a non-NULL d_x on a context that is not member-chunked; cleared by every other entry point that
 * evaluates or changes a setting (grape_eval*, grape_eval_fom, grape_lbfgs, the host forms, grape_get_controls, every
 * grape_set_*, grape_comm_attach / grape_ipc_attach) and by any failed call of the device forms.  d_x = NULL with the flag
 * clear: GRAPE_ERR_NOT_READY, the message names the reason; a member-chunked context always answers GRAPE_ERR_NOT_READY
 * ("member_chunk": its workspace holds one block of members only). */
int grape_eval_observables_device(grape_ctx *ctx, const double *d_x, int32_t n_obs, int32_t per_member, const double *d_O,
                                  double *d_y, double *d_X_final, double *d_fg, void *stream);
int grape_eval_vjp_device(grape_ctx *ctx, const double *d_x, int32_t n_obs, int32_t per_member, const double *d_O,
                          const double *d_ybar, const double *d_Xbar_final, double *d_G, void *stream);

/* ABI v8 (additive).  grape_eval_vjp for several cotangent sets behind ONE evaluation of x: one gradient per loss or constraint
 * of a multi-objective / constrained optimiser, Jacobian ROWS of the read-out in reverse mode (the twin of the columns
 * grape_eval_jvp_multi gives), per-probe sensitivities.  The set index is slowest everywhere:
 *   ybar        c128 (N+1, n_obs, E, n_set)   nullable for the whole block (zero)
 *   Xbar_final  c128 (n, m, E, n_set)         nullable for the whole block (zero); not both
 *   G           f64  (K, cols, n_set)         cols = N, or M in parameter mode
 * The probes O are shared by the sets.  1 <= n_set <= GRAPE_MAX_VJP_COTANGENTS, anything else GRAPE_ERR_INVALID_ARG with the
 * value in the message.  Every other argument check, refusal (checked first) and GRAPE_ERR_NOT_READY is grape_eval_vjp's; the
 * not-finite check of the host arrays runs over all sets.
 * DEFINING PROPERTY: block r of G is bit for bit what grape_eval_vjp returns for set r alone on the same context -- in both
 * modes of grape_set_trajectory_derivative, under a basis and / or bounds, on member-chunked contexts (the unchunked bits),
 * with forced slices_per_lane / waves_per_member and under a standing running cost, penalties or risk (none of which enter).
 * Exact linearity in the cotangents and the transpose identity with grape_eval_jvp_multi follow from it.
 * trajectory_vjp_multi_kernel carries a block of sets (2 to 8, by operator dimension and state columns) next to one chunk
 * product, one prefix scan, one walk of the states and one load of every propagator per pass; vjp_sum_kernel adds every
 * set's rows in grape_eval_vjp's fixed tree.  A decomposition with more than 256 time chunks per member, the exact mode
 * (trajectory_vjp_exact_kernel + traj_frechet_rows_kernel once per set behind the ONE sweep) and GRAPE_VJP_MULTI=0 run the
 * single call's kernels per set: the same bits; grape_get_kernel_names tells which ran.  The scratch of the block (the
 * members' rows, the groups' sums, the summed and projected rows of every set) is counted in grape_info.workspace_bytes.
 * An eval -> vjp_multi -> eval sequence returns the first evaluation's bits. */
#define GRAPE_MAX_VJP_COTANGENTS 8
int grape_eval_vjp_multi(grape_ctx *ctx, const double *x, int32_t n_set, int32_t n_obs, int32_t per_member,
                         const double *O, const double *ybar, const double *Xbar_final, double *G);

/* ABI v8 (additive).  The device form of grape_eval_vjp_multi under the rules of grape_eval_vjp_device: device arrays in the
 * layouts above, asynchronous on `stream`, not checked for non-finite values, no staging copy; the "trajectory valid" flag is
 * set under the same conditions.  d_x = NULL pulls back along the stored trajectory with no sweep, keeps the flag set and
 * returns the bits of the call with d_x; with the flag clear, or on a member-chunked context, GRAPE_ERR_NOT_READY with
 * grape_eval_vjp_device's messages.  The multi instance reads ybar directly (no staged instance). */
int grape_eval_vjp_multi_device(grape_ctx *ctx, const double *d_x, int32_t n_set, int32_t n_obs, int32_t per_member,
                                const double *d_O, const double *d_ybar, const double *d_Xbar_final, double *d_G,
                                void *stream);

/* ABI v8 (additive).  The Jacobian-vector product of the trajectory read-out: the forward-mode twin of grape_eval_vjp.  Given
 * a direction xdot in control space it returns how every expectation value along the trajectory, and the final state of every
 * member, move to first order -- what a Gauss-Newton / Levenberg-Marquardt step on a loss on y needs next to the pull-back,
 * a linear-response read-out, and the jvp of a forward-mode autograd framework.
 *   x, n_obs, per_member, O   exactly as in grape_eval_observables / grape_eval_vjp
 *   xdot       host f64, the shape and coordinates of x: (K, N), or (K, M) in parameter mode; the raw u-direction under bounds
 *   ydot       host c128 (N+1, n_obs, E), the layout of y; nullable
 *   Xdot_final host c128 (n, m, E), the layout of X_final; nullable (but not both)
 * With the states and propagators of the physical pulse and the physical direction xdot_phys:
 *   Xdot_{k,0}   = 0
 *   Xdot_{k,s+1} = P_{k,s} Xdot_{k,s} + ( sum_c xdot_phys[c,s] (-i dt B_kc) ) X_{k,s+1}        s = 0 .. N-1
 *   ydot[s,j,k]  = tr(O_kj' Xdot_{k,s})         (ydot[0,.,.] = 0, written)
 *   Xdot_final_k = Xdot_{k,N}
 * FIRST ORDER in dt: the linearisation of grape_eval_vjp, whose exact transpose this is -- for any cotangents, with
 * G = grape_eval_vjp(ybar, Xbar_final) on the same context,
 *   sum Re(conj(ybar) ydot) + sum_k Re tr(Xbar_k' Xdot_final_k) = sum_{c,t} G[c,t] xdot[c,t]
 * holds to rounding, in the coordinates of x.  Against central differences of grape_eval_observables on a smooth pulse the
 * deviation falls by ~4 per 4x in N.  The exact tangent: grape_set_trajectory_derivative(ctx, GRAPE_TRAJ_EXACT), below.
 * With grape_set_bounds and / or grape_set_basis in force xdot_phys = s * (xdot phi^T): the expansion without x0 (phi is the
 * identity without a basis) times the slope array s of this very evaluation (1 without bounds) -- the transpose of what the
 * pull-back's tail does (basis_expand_kernel / bounds_tangent_kernel in tangent mode).  No ensemble weight, penalty, running
 * cost or risk enters.
 * The call runs ONE evaluation of x exactly as the context is configured and discards its [G, F]; behind the sweep of every
 * member block (the running-cost kernels, if any) trajectory_jvp_kernel reads the stored propagators -- one workgroup per
 * member, one lane per time chunk, two forward walks whatever n_obs is.  Members are independent: there is no sum over
 * members.  Blocking, ordered behind an in-flight grape_eval_device; afterwards grape_get_kernel_names includes the kernel.
 * An eval -> jvp -> eval sequence returns the first evaluation's bits; results are bitwise reproducible call to call; a
 * member-chunked context returns the unchunked context's bits; a standing running cost, penalties or risk do not change a bit.
 * Every operation is linear in xdot: 2 xdot returns twice the bits, -xdot the negated bits, 0 returns 0.
 * Served: the contexts grape_eval_vjp serves -- kernel family 0 (n = 2, 3, 4), GRAPE_UNITARY_GATE with any m, Hermitian and
 * non-Hermitian generators, both variants, gradient = 0 and objective = 0, single-device contexts without communicator or
 * mailbox, member-chunked contexts, max_batch > 1 (the call takes one array) and forced slices_per_lane / waves_per_member
 * included.  Refused before anything runs, GRAPE_ERR_UNSUPPORTED with grape_eval_vjp's reasons ("dimension", "StateTransfer",
 * "exact", "multi-device", "communicator").
 * GRAPE_ERR_INVALID_ARG: null x or xdot; ydot and Xdot_final both NULL; n_obs outside 0..16; n_obs = 0 with a non-NULL ydot;
 * n_obs > 0 with a NULL O; per_member other than 0 or 1; a non-finite entry of O or xdot ("not finite").  The context's
 * refusals are checked first.  Before grape_set_operators: GRAPE_ERR_NOT_READY.  After any refusal the context evaluates
 * exactly as before.  Non-finite x propagates NaN. */
int grape_eval_jvp(grape_ctx *ctx, const double *x, const double *xdot, int32_t n_obs, int32_t per_member, const double *O,
                   double *ydot, double *Xdot_final);

/* ABI v8 (additive).  The device form of grape_eval_jvp, under the rules of grape_eval_observables_device /
 * grape_eval_vjp_device: every array lives in device memory of the context's GPU (d_xdot f64 in the layout of d_x, d_ydot c128
 * (N+1, n_obs, E), d_Xdot_final c128 (n, m, E)), the call is asynchronous on `stream`, nothing is synchronised, nothing is
 * staged (without a pulse map the kernel reads d_xdot in place; with one, the tangent map writes the physical direction into
 * scratch of the context, which grows only behind a pending device call).  Device arrays are NOT checked for non-finite
 * entries; everything else is validated as in the host form, the context's refusals first.  Results are bit for bit the host
 * form's.  There is one instance of the kernel (no staged one).
 * With a non-NULL d_x on a context that is not member-chunked the call sets the "trajectory valid" flag, exactly as the other
 * two device forms do.  d_x = NULL pushes xdot forward along the stored trajectory of the last device form: only the tangent
 * map and trajectory_jvp_kernel run, no sweep, and the bits are those of the call with d_x given; with the flag clear, or on a
 * member-chunked context, GRAPE_ERR_NOT_READY with grape_eval_vjp_device's messages.  A reuse call keeps the flag set, so
 * grape_eval_vjp_device(d_x = NULL) may follow it: the Gauss-Newton inner loop (one J v, one J' w per CG iteration at one
 * linearisation point). */
int grape_eval_jvp_device(grape_ctx *ctx, const double *d_x, const double *d_xdot, int32_t n_obs, int32_t per_member,
                          const double *d_O, double *d_ydot, double *d_Xdot_final, void *stream);

/* ABI v8 (additive).  Several tangent directions per call: a block of Jacobian columns (Gauss-Newton / Levenberg-Marquardt on
 * a least-squares trajectory loss, sensitivity and Fisher-type analyses) without repeating what does not depend on the
 * direction -- the sweep, the chunk products, the prefix scan of the propagators, the walk of the states and the passes over
 * the stored propagators.
 *   xdot        f64  (K, cols, n_dir)   cols = N, or M in parameter mode; the direction index is slowest and every direction
 *                                       has the shape and the coordinates grape_eval_jvp takes
 *   ydot        c128 (N+1, n_obs, E, n_dir), Xdot_final c128 (n, m, E, n_dir): direction-slowest too; either may be NULL
 * 1 <= n_dir <= GRAPE_MAX_JVP_DIRECTIONS, anything else GRAPE_ERR_INVALID_ARG with the value in the message.  Every other
 * argument check, the refusals (the context's first), GRAPE_ERR_NOT_READY before grape_set_operators and the not-finite check
 * of O and xdot are grape_eval_jvp's.
 * DEFINING PROPERTY: block d of ydot / Xdot_final is bit for bit what grape_eval_jvp returns for direction d alone on the same
 * context -- in both modes of grape_set_trajectory_derivative, under a basis and / or bounds, on member-chunked contexts (the
 * unchunked bits), with forced slices_per_lane / waves_per_member and under a standing running cost, penalties or risk (none
 * of which enter).  Exact linearity in xdot and the transpose identity with grape_eval_vjp follow from it.
 * trajectory_jvp_multi_kernel carries a block of directions (2 to 8, by operator dimension and state columns) next to one
 * state walk; per direction its operations and their order are trajectory_jvp_kernel's.  Where it did not measure faster per
 * direction than the single kernel, and for decompositions of more than 256 time chunks per member, the library runs
 * trajectory_jvp_kernel once per direction behind the ONE sweep: the same bits, and grape_get_kernel_names tells which ran
 * (environment GRAPE_JVP_MULTI=0 / 1 forces the choice).  In the exact mode every direction of a block has its own E_t image
 * in the context's scratch (shared with the exact pull-back and the exact running cost; stream order separates the users).
 * An eval -> jvp_multi -> eval sequence returns the first evaluation's bits. */
#define GRAPE_MAX_JVP_DIRECTIONS 8
int grape_eval_jvp_multi(grape_ctx *ctx, const double *x, int32_t n_dir, const double *xdot, int32_t n_obs, int32_t per_member,
                         const double *O, double *ydot, double *Xdot_final);

/* ABI v8 (additive).  The device form of grape_eval_jvp_multi under the rules of grape_eval_jvp_device: device arrays in the
 * layouts above, asynchronous on `stream`, no staging beyond the single device form's (under a pulse map the physical
 * directions go into scratch of the context, which grows only behind a pending device call and is counted in
 * grape_info.workspace_bytes, as are the further E_t images of the exact mode), device arrays not checked for non-finite
 * entries, results bit for bit the host form's.  The "trajectory valid" flag is set under grape_eval_jvp_device's conditions;
 * d_x = NULL runs along the stored trajectory with no sweep, keeps the flag set and returns the bits of the call with d_x;
 * with the flag clear or on a member-chunked context GRAPE_ERR_NOT_READY with the existing messages. */
int grape_eval_jvp_multi_device(grape_ctx *ctx, const double *d_x, int32_t n_dir, const double *d_xdot, int32_t n_obs,
                                int32_t per_member, const double *d_O, double *d_ydot, double *d_Xdot_final, void *stream);

/* ABI v8 (additive).  Second-order products along the trajectory: the directional derivative of grape_eval_vjp's program.
 * Given a direction xdot in control space and the tangent (ybar_dot, Xbar_final_dot) of the cotangents it returns how the
 * pull-back G = grape_eval_vjp(ybar, Xbar_final) moves to first order -- for a loss l(y(x), X_N(x)) with ybar = dl/dy,
 * ybar_dot = l'' (ydot, Xdot_N) and (ydot, Xdot_N) from grape_eval_jvp this is the Hessian-vector product H_l xdot, what a
 * Newton-CG or trust-region step on a custom loss and a curvature analysis need.
 *   x, n_obs, per_member, O, ybar, Xbar_final   exactly as in grape_eval_vjp (same layouts, same cotangent convention)
 *   xdot            host f64, the shape and coordinates of x, as in grape_eval_jvp
 *   ybar_dot        host c128 (N+1, n_obs, E), the layout of ybar; NULL: zero
 *   Xbar_final_dot  host c128 (n, m, E), the layout of Xbar_final; NULL: zero (each alone or both)
 *   Gdot            host f64 (K, N), or (K, M) in parameter mode
 * With B'_kc = -i dt B_kc, V_ks = sum_c xdot_phys[c,s] B'_kc, the propagators P and states X of the physical pulse and the
 * costate Lam of grape_eval_vjp for (ybar, Xbar_final):
 *   Xdot_0  = 0 ,    Xdot_{s+1} = P_s Xdot_s + V_s X_{s+1}                                          (grape_eval_jvp's tangent)
 *   Lamd_N  = Xbar_final_dot + sum_j ybar_dot[N,j] O_j
 *   Lamd_s  = P_s' ( Lamd_{s+1} + V_s' Lam_{s+1} ) + sum_j ybar_dot[s,j] O_j                       s = N-1 .. 1
 *   Gdot[c,t] = sum_k Re tr( Lamd_{k,t+1}' B'_kc X_{k,t+1} ) + Re tr( Lam_{k,t+1}' B'_kc Xdot_{k,t+1} )      t = 0 .. N-1
 * FIRST ORDER in dt like the pair it joins: Gdot is exactly the derivative of grape_eval_vjp's G under the rule that pair uses,
 * Pdot_s = V_s P_s (central differences of the VJP recurrence over P_s(eps) = expm(eps V_s) P_s agree to the difference
 * quotient's own error); against the true directional derivative of G the deviation falls by ~4 per 4x in N.  With xdot = 0
 * the result is grape_eval_vjp(ybar_dot, Xbar_final_dot).  The same-slice block of this operator is NOT symmetric: it holds
 * B_c B_d, not the symmetrised product (the rule differentiates P_s once more on the left only).  That changes the rate of a
 * Newton iteration, not its fixed point.
 * Gdot carries no ensemble weight, penalty, running cost or risk.  Under grape_set_basis xdot_phys is the tangent expansion
 * grape_eval_jvp uses and Gdot goes through the projection grape_eval_vjp uses (basis_project_kernel).
 * The call runs ONE evaluation of x exactly as the context is configured and discards its [G, F]; behind the sweep of every
 * member block trajectory_hvp_kernel reads the stored propagators -- one workgroup per member, one lane per time chunk -- and
 * vjp_sum_kernel adds the members' rows in grape_eval_vjp's fixed tree.  Blocking, ordered behind an in-flight
 * grape_eval_device; afterwards grape_get_kernel_names includes trajectory_hvp_kernel.  An eval -> hvp -> eval sequence returns
 * the first evaluation's bits; results are bitwise reproducible call to call; a member-chunked context returns the unchunked
 * context's bits; a standing running cost, penalties or risk do not change a bit.  Every operation is linear in the triple
 * (xdot, ybar_dot, Xbar_final_dot): twice the triple returns twice the bits, the negated triple the negated bits.
 * Served: the contexts grape_eval_vjp serves, refused with its reasons first.  Two refusals of this call alone follow them,
 * GRAPE_ERR_UNSUPPORTED: grape_set_bounds in force ("bounds": the saturation's second derivative and the first-order G would
 * enter) and grape_set_trajectory_derivative(GRAPE_TRAJ_EXACT) in force ("trajectory_derivative": a second Frechet derivative
 * would be needed).  They are checked in this order ("bounds" first where both stand), in front of the argument checks and of
 * the GRAPE_ERR_NOT_READY of a reuse; a device-form call refused by either clears the "trajectory valid" flag like any failed
 * call of the device forms.
 * GRAPE_ERR_INVALID_ARG: null x, xdot or Gdot; ybar and Xbar_final both NULL; n_obs outside 0..16; n_obs = 0 with a non-NULL
 * ybar or ybar_dot; n_obs > 0 with a NULL O; per_member other than 0 or 1; a non-finite entry of a host array ("not finite").
 * Before grape_set_operators: GRAPE_ERR_NOT_READY.  After any refusal the context evaluates exactly as before. */
int grape_eval_hvp(grape_ctx *ctx, const double *x, const double *xdot, int32_t n_obs, int32_t per_member, const double *O,
                   const double *ybar, const double *Xbar_final, const double *ybar_dot, const double *Xbar_final_dot,
                   double *Gdot);

/* ABI v8 (additive).  The device form of grape_eval_hvp under the rules of grape_eval_vjp_device / grape_eval_jvp_device: every
 * array lives in device memory of the context's GPU, the call is asynchronous on `stream`, nothing is synchronised; device
 * arrays are NOT checked for non-finite entries, everything else is validated as in the host form.  Results are bit for bit
 * the host form's.  With a non-NULL d_x on a context that is not member-chunked the call sets the "trajectory valid" flag;
 * d_x = NULL runs along the stored trajectory of the last device form with no sweep and the same bits, and keeps the flag set,
 * so the other reuse calls may follow (a Newton-CG inner loop: one grape_eval_jvp_device(NULL) and one grape_eval_hvp_device(NULL)
 * per iteration at one linearisation point).  With the flag clear, or on a member-chunked context, GRAPE_ERR_NOT_READY with
 * grape_eval_vjp_device's messages. */
int grape_eval_hvp_device(grape_ctx *ctx, const double *d_x, const double *d_xdot, int32_t n_obs, int32_t per_member,
                          const double *d_O, const double *d_ybar, const double *d_Xbar_final, const double *d_ybar_dot,
                          const double *d_Xbar_final_dot, double *d_Gdot, void *stream);

/* ABI v8 (additive).  Gauss-Newton products along the trajectory in ONE pass: the push-forward of grape_eval_jvp, weighted entry
 * by entry, into the pull-back of grape_eval_vjp -- Gn = J' W J xdot, the operator a Gauss-Newton or Levenberg-Marquardt step on
 * a least-squares trajectory loss (tracking a population curve, fitting a measured transient, holding a state on a path) applies
 * once per CG iteration.  Neither ydot nor a ybar array exists anywhere.
 *   x, xdot, n_obs, per_member, O   exactly as in grape_eval_jvp (x is theta / u under grape_set_basis / grape_set_bounds)
 *   w_per_member    0: wy is shared by the members; 1: one block per member
 *   wy              host f64 (N+1, n_obs, 3) (w_per_member = 0) or (N+1, n_obs, E, 3) (w_per_member = 1), column-major, the
 *                   PLANES rr, ri, ii slowest: a real symmetric 2x2 block per entry of y, acting on (Re ydot, Im ydot).  Scalar
 *                   weights are rr = ii = w, ri = 0.  Row s = 0 is read by nobody (ydot[0] = 0).  NULL: zero
 *   wf              host f64 [E], the weights of the final states; NULL: zero (each alone or both)
 *   Gn              host f64 (K, N), or (K, M) in parameter mode: the shape and coordinates of grape_eval_vjp's G
 * With B'_kc = -i dt B_kc, V_ks = sum_c xdot_phys[c,s] B'_kc and the propagators P and states X of the physical pulse:
 *   D_0    = 0 ,    D_{s+1} = P_s D_s + V_s X_{s+1}                                                  (grape_eval_jvp's tangent)
 *   ydot[s,j,k] = tr( O_kj' D_{k,s} )
 *   c[s,j,k]    = ( w_rr Re ydot + w_ri Im ydot ) + i ( w_ri Re ydot + w_ii Im ydot )
 *   Lam_N  = wf_k D_N + sum_j c[N,j,k] O_kj ,    Lam_s = P_s' Lam_{s+1} + sum_j c[s,j,k] O_kj         s = N-1 .. 1
 *   Gn[c,t] = sum_k Re tr( Lam_{k,t+1}' B'_kc X_{k,t+1} )                                             t = 0 .. N-1
 * that is grape_eval_vjp(ybar = W ydot, Xbar_final = wf Xdot_final) of (ydot, Xdot_final) = grape_eval_jvp(xdot), FIRST ORDER in
 * dt under the rule of that pair.  With these weights it is the generalised Gauss-Newton matrix of any loss that is separable
 * over the entries of y (the block is l'' of the entry's loss in (Re y, Im y): (|y|^2 - p)^2 and log-barriers on populations
 * have an off-diagonal part) plus 1/2 wf_k |X_N - T|^2.  The operator is symmetric to rounding, and positive semi-definite for
 * PSD blocks and wf >= 0; the library does NOT check definiteness -- indefinite weights are the caller's business.
 * Gn carries no ensemble weight, penalty, running cost or risk.  Under grape_set_basis and / or grape_set_bounds xdot_phys is
 * the tangent map grape_eval_jvp uses and Gn goes through the slope and projection grape_eval_vjp uses: Phi' s J' W J s Phi.
 * Bounds ARE served (no second derivative of the pulse map enters), unlike grape_eval_hvp.
 * The call runs ONE evaluation of x exactly as the context is configured and discards its [G, F]; behind the sweep of every
 * member block trajectory_gnvp_kernel reads the stored propagators -- one workgroup per member, one lane per time chunk -- and
 * vjp_sum_kernel adds the members' rows in grape_eval_vjp's fixed tree.  The kernel's scratch (one n x m block per slice and
 * member of a workspace block: the costate's source) is allocated on first use, grows only behind a pending device call and is
 * counted in grape_info.workspace_bytes.  Blocking, ordered behind an in-flight grape_eval_device; afterwards
 * grape_get_kernel_names includes trajectory_gnvp_kernel.  An eval -> gnvp -> eval sequence returns the first evaluation's
 * bits; results are bitwise reproducible call to call; a member-chunked context returns the unchunked context's bits; a
 * standing running cost, penalties or risk do not change a bit.  Every operation is linear in xdot, and in (wy, wf): twice the
 * direction returns twice the bits, the negated direction the negated bits, xdot = 0 exact zeros; shared weights return the
 * bits of the same block repeated per member.
 * Served: the contexts grape_eval_vjp serves, refused with its reasons first.  One refusal of this call alone follows them,
 * GRAPE_ERR_UNSUPPORTED: grape_set_trajectory_derivative(GRAPE_TRAJ_EXACT) in force ("trajectory_derivative": the fused kernel
 * carries the first-order pair only).
 * GRAPE_ERR_INVALID_ARG: null x, xdot or Gn; wy and wf both NULL; n_obs outside 0..16; n_obs = 0 with a non-NULL wy; n_obs > 0
 * with a NULL O; per_member or w_per_member other than 0 or 1; a non-finite entry of a host array ("not finite").
 * Before grape_set_operators: GRAPE_ERR_NOT_READY.  After any refusal the context evaluates exactly as before. */
int grape_eval_gnvp(grape_ctx *ctx, const double *x, const double *xdot, int32_t n_obs, int32_t per_member, const double *O,
                    int32_t w_per_member, const double *wy, const double *wf, double *Gn);

/* ABI v8 (additive).  The device form of grape_eval_gnvp under the rules of grape_eval_vjp_device / grape_eval_jvp_device: every
 * array lives in device memory of the context's GPU, the call is asynchronous on `stream`, nothing is synchronised; device
 * arrays are NOT checked for non-finite entries, everything else is validated as in the host form.  Results are bit for bit
 * the host form's.  With a non-NULL d_x on a context that is not member-chunked the call sets the "trajectory valid" flag;
 * d_x = NULL runs along the stored trajectory of the last device form with no sweep and the same bits, and keeps the flag set,
 * so the other reuse calls may follow (a Gauss-Newton-CG inner loop: ONE grape_eval_gnvp_device(NULL) per iteration at one
 * linearisation point).  With the flag clear, or on a member-chunked context, GRAPE_ERR_NOT_READY with
 * grape_eval_vjp_device's messages. */
int grape_eval_gnvp_device(grape_ctx *ctx, const double *d_x, const double *d_xdot, int32_t n_obs, int32_t per_member,
                           const double *d_O, int32_t w_per_member, const double *d_wy, const double *d_wf, double *d_Gn,
                           void *stream);

/* ABI v8 (additive).  grape_gn_step: one Levenberg-Marquardt step of the least-squares trajectory loss
 *   L(x) = 1/2 sum_{s,j,k} r' W r + 1/2 sum_k wf_k |X_{k,N} - T_k|^2 ,   r = y - y_target split into (Re, Im)
 * solved on the device: its loss, its gradient g and the damped Gauss-Newton step p of (J' W J + lambda 1) p = -g from ONE
 * sweep and ONE upload of everything; the CG iterations run along the stored trajectory with their vectors and scalars in
 * device memory. */
typedef struct grape_gn_options {
    double  lambda;        /* damping, finite and >= 0: the system is (J' W J + lambda 1) p = -g in the coordinates of x */
    double  cg_rtol;       /* stop when |r|_2 <= cg_rtol |g|_2 (CG's own recurrence residual); < 0 = 1e-10; 0 = never */
    int32_t cg_max_iter;   /* operator applications at most; 0 = loss and gradient only (p = 0); < 0 invalid */
    int32_t reserved;      /* must be 0 */
} grape_gn_options;

typedef struct grape_gn_result {
    double  loss;          /* L(x) */
    double  g_norm;        /* |g|_2 */
    double  g_inf;         /* |g|_inf */
    double  residual;      /* |r|_2 of the recurrence at exit */
    double  p_norm;        /* |p|_2 */
    double  predicted;     /* -g'p - p'Hp/2 with Hp = Ap - lambda p, Ap accumulated from CG's own products */
    int32_t cg_iterations; /* operator applications that updated the state */
    int32_t status;        /* 0 converged, 1 iteration limit, 2 direction without positive curvature (also: NaN), 3 g = 0 */
} grape_gn_result;

/*   x, n_obs, per_member, O, w_per_member, wy, wf   exactly as in grape_eval_gnvp, the planes rr, ri, ii of wy included
 *   y_target        host c128 (N+1, n_obs, E) column-major, y's layout; it comes with wy or not at all
 *   Xf_target       host c128 (n, m, E) column-major, X_final's layout; it comes with wf or not at all.  One pair at least
 *   p, g            host f64 (K, N), or (K, M) in parameter mode: the shape and coordinates of grape_eval_vjp's G; g may be NULL
 * g is what grape_eval_vjp(ybar = W r, Xbar_final = wf (X_N - T)) returns, the cotangent
 * c = (w_rr Re r + w_ri Im r) + i (w_ri Re r + w_ii Im r) as in grape_eval_gnvp; with unit weights bit for bit.  The operator is
 * grape_eval_gnvp's, first order in dt; bounds and a basis are served as they are there.  The iteration is conjugate gradients
 * from p = 0 with apply(v) = J' W J v + lambda v: the test r.r <= (cg_rtol |g|)^2 stands in front of every application, a
 * direction d with !(d' apply(d) > 0) ends the solve (status 2) with the state it found.
 * One call: every check, the host arrays' entries included; one upload; ONE evaluation of x as the context is configured, its
 * [G, F] discarded; gn_residual_kernel (the read-out with the residual and the weights formed on the device: only the
 * cotangents and L leave it, y never exists); the pull-back along the stored trajectory; per CG iteration one reuse launch of
 * trajectory_gnvp_kernel + vjp_sum_kernel and one gn_cg_step_kernel, enqueued in blocks of 4 (GRAPE_GN_CG_BLOCK = 1..64)
 * between which the host reads the scalars through the bounded wait of every blocking call (GRAPE_EVAL_TIMEOUT_S); launches
 * behind convergence are no-ops, so p, g and result do not depend on the block size, bit for bit.  Every sum has one fixed
 * tree: results are bitwise reproducible; a standing running cost, penalties or risk do not change a bit; an eval -> gn_step
 * -> eval sequence returns the first evaluation's bits.  The scratch (the targets, the cotangents, the CG vectors, the record)
 * is allocated on first use and counted in grape_info.workspace_bytes.  Blocking; the "trajectory valid" flag of the device
 * forms is left clear.
 * Refused with grape_eval_gnvp's refusals first, in its order and words ("trajectory_derivative" under GRAPE_TRAJ_EXACT
 * included); then GRAPE_ERR_UNSUPPORTED on a member-chunked context ("member_chunk": the iterations run along ONE stored
 * trajectory).  GRAPE_ERR_INVALID_ARG: null x, p, result or opts; wy without y_target or the reverse, wf without Xf_target or
 * the reverse, neither pair; lambda negative or not finite; cg_rtol not finite; cg_max_iter < 0; reserved != 0; n_obs,
 * per_member, w_per_member out of range as in grape_eval_gnvp; a non-finite entry of a host array other than x ("not
 * finite").  Before grape_set_operators: GRAPE_ERR_NOT_READY.  After any refusal the context evaluates exactly as before.  A
 * non-finite x is not refused: the call returns GRAPE_OK with status = 2, loss = NaN and p = 0.
 * Not served (refused as above): a device-pointer form, member-chunked contexts, the exact trajectory derivative, n >= 5, the
 * sandwich types. */
int grape_gn_step(grape_ctx *ctx, const double *x, int32_t n_obs, int32_t per_member, const double *O,
                  const double *y_target, int32_t w_per_member, const double *wy,
                  const double *Xf_target, const double *wf,
                  const grape_gn_options *opts, double *p, double *g, grape_gn_result *result);

/* ABI v8 (additive).  The ensemble-averaged host forms of the trajectory read-out, its pull-back and its push-forward: the
 * member axis of y / ybar / ydot never crosses the bus.  What an experiment on an inhomogeneously broadened ensemble measures
 * is sum_k v_k y[k]; a loss on it has the cotangent ybar[k] = v_k ybar_mean, ONE block broadcast over the members.
 *   x, xdot, n_obs, per_member, O, F, G   exactly as in grape_eval_observables / grape_eval_vjp / grape_eval_jvp (x is theta / u
 *                   under grape_set_basis / grape_set_bounds and G is in x's coordinates; both trajectory-derivative modes)
 *   v               host f64 [E], the weights of the sum; NULL: the ensemble weights w_k as grape_set_operators received them
 *                   (their device copy is read).  grape_set_risk does not enter: a caller who wants the risk weights passes
 *                   grape_get_risk_weights' output.  Zero and negative entries are accepted
 *   y_mean, ybar_mean, ydot_mean   host c128 (N+1, n_obs) column-major; ybar_mean in grape_eval_vjp's cotangent convention
 *                   (dl/dRe + i dl/dIm of the AVERAGED value)
 *   X_mean, Xbar_mean, Xdot_mean   host c128 (n, m) column-major
 * Nullability follows the call each form sits on: at least one of the pair; n_obs = 0 with a non-NULL y-type array is invalid.
 *   y_mean[s + (N+1) j] = sum_k v_k y[s + (N+1)(j + n_obs k)],   X_mean = sum_k v_k X_{k,N}
 * and the same sums of grape_eval_jvp's ydot / Xdot_final.  F of the read-out is grape_eval's F bit for bit.
 * grape_eval_vjp_mean returns, BIT FOR BIT, the G grape_eval_vjp returns for the explicit cotangents
 *   ybar[s,j,k] = (v_k Re ybar_mean[s,j], v_k Im ybar_mean[s,j]),   Xbar_k = (v_k Re Xbar_mean, v_k Im Xbar_mean)
 * -- each component one rounded product: traj_mean_broadcast_kernel writes exactly those arrays into the buffers the
 * pull-back kernels read, in front of the evaluation, and everything behind it is grape_eval_vjp.
 * The sums: traj_mean_reduce_kernel cuts the member axis into segments of 16 consecutive members and sums each in member
 * order (the first term a product, every further one an FMA), one lane per complex entry; with more than one segment
 * traj_mean_combine_kernel adds the segments' sums in segment order.  No atomics.  The tree depends on E alone -- not on N,
 * n_obs, the probe index, the member chunk or the sweep's workgroup layout -- so results are bitwise reproducible, a
 * member-chunked context returns the unchunked context's bits, and column j of a 16-probe call is the 1-probe call with
 * probe j.  E = 1 with v = {1.0} returns y[0].  Each component differs from the exact sum by at most
 * E 2^-53 sum_k |v_k| |component_k| to first order.  The reduction runs once, behind the read-out (push-forward) of the last
 * member block; afterwards grape_get_kernel_names includes the kernels named here.
 * Host forms ONLY: there is no _device form, no multi form and no HVP form.  A caller with device tensors already holds y on
 * the GPU and averages it there.
 * Served and refused exactly where the underlying call is, with its words behind this call's name: the context's refusals
 * first (GRAPE_ERR_UNSUPPORTED), then the arguments.  GRAPE_ERR_INVALID_ARG: what the underlying call refuses, a non-finite
 * entry of v, ybar_mean or Xbar_mean ("not finite"), and for grape_eval_vjp_mean a product v_k ybar_mean / v_k Xbar_mean that
 * overflows ("not finite").  Before grape_set_operators: GRAPE_ERR_NOT_READY.  After any refusal the context evaluates exactly
 * as before; a context that never calls these launches the kernels it always did; eval -> *_mean -> eval returns the first
 * evaluation's bits.  Blocking, ordered behind an in-flight grape_eval_device. */
int grape_eval_observables_mean(grape_ctx *ctx, const double *x, int32_t n_obs, int32_t per_member, const double *O,
                                const double *v, double *y_mean, double *X_mean, double *F);
int grape_eval_vjp_mean(grape_ctx *ctx, const double *x, int32_t n_obs, int32_t per_member, const double *O,
                        const double *v, const double *ybar_mean, const double *Xbar_mean, double *G);
int grape_eval_jvp_mean(grape_ctx *ctx, const double *x, const double *xdot, int32_t n_obs, int32_t per_member,
                        const double *O, const double *v, double *ydot_mean, double *Xdot_mean);

/* ABI v8 (additive).  The derivative rule of the pull-back and the push-forward along the trajectory: all six entry points --
 * grape_eval_vjp, grape_eval_vjp_device, grape_eval_jvp, grape_eval_jvp_device and the d_x = NULL reuse forms of both device
 * calls.  GRAPE_TRAJ_FIRST_ORDER (the default) takes dP_t/dx[c,t] as (-i dt B_c) P_t, as documented above.  GRAPE_TRAJ_EXACT
 * takes the Frechet derivative DF_t[E] at G_t = -i dt H_t of the map the sweep itself evaluated (the degree-8 Taylor
 * polynomial at G_t / 2^s squared s times, with the sweep's own s per slice, a forced expm_squarings included), operation by
 * operation -- exact to the rounding of P_t, the code path of gradient = exact (exact_grad.hip):
 *   VJP:  G[c,t]       = sum_k Re tr( Lam_{k,t+1}' DF_t[B'_kc] X_{k,t} ) = sum_k Re tr( DF_t[W_{k,t}] B'_kc ),
 *                        W_{k,t} = X_{k,t} Lam_{k,t+1}' ,  B' = -i dt B     (ONE derivative per slice serves all K controls)
 *   JVP:  Xdot_{k,t+1} = P_{k,t} Xdot_{k,t} + DF_t[V_t] X_{k,t} ,   V_t = sum_c xdot_phys[c,t] B'_kc
 * X_{k,t} is the state BEFORE slice t (the first-order rule uses X_{k,t+1}).  Everything else is unchanged: the layouts and
 * the cotangent convention, the Lam recurrence and ybar[0] contributing nothing, no weight / penalty / running cost / risk in
 * the result, the slope / projection tail and the tangent map under bounds / basis, member-chunked contexts, max_batch > 1,
 * the argument checks and the refusals.  The pair stays an exact transpose pair, now of the true derivative:
 * torch.autograd.gradcheck on the read-out passes, and against central differences the deviation is that of the differences.
 * The running cost's own gradient (grape_set_running_cost) follows its own setting, grape_set_running_cost_derivative
 * below (first order by default), and the main objective's stays first order unless the context was created with
 * gradient = exact.
 * Kernels (grape_get_kernel_names tells which ran): the exact instance of trajectory_vjp_kernel
 * (trajectory_vjp_exact_kernel) stores W_t per slice, traj_frechet_rows_kernel -- one lane (n = 3) or lane pair (n = 2, 4)
 * per (member, slice) -- rebuilds G_t from the physical pulse the evaluation left on the device and writes the row entries
 * that vjp_sum_kernel sums as ever; traj_frechet_dir_kernel stores E_t = DF_t[V_t] per slice and the exact instance of
 * trajectory_jvp_kernel (trajectory_jvp_exact_kernel) consumes it.  In front of them copy_kernel keeps the physical pulse
 * for the reuse forms, which stay bit for bit equal to the calls with d_x given.  The staged VJP instance is not used in
 * this mode (GRAPE_TRAJ_STAGED is ignored for the pull-back).  Scratch: one n x n c128 block per slice and member of a
 * workspace block -- the size of one control array's propagators -- shared by W_t and E_t, allocated by the first exact
 * call, counted in grape_info.workspace_bytes, growing only behind a pending device call.  No atomics: results are
 * bitwise reproducible call to call, member-chunked = unchunked, host form = device form, and the JVP is exactly linear in
 * xdot.
 * A setting like the other grape_set_*: valid any time after grape_create, persists across grape_set_operators, ordered
 * behind an in-flight grape_eval_device, clears the "trajectory valid" flag.  GRAPE_ERR_INVALID_ARG: mode outside {0, 1}.
 * mode = GRAPE_TRAJ_EXACT on a context that grape_eval_vjp refuses is refused with GRAPE_ERR_UNSUPPORTED and that call's
 * reason ("dimension", "StateTransfer", "exact", "multi-device", "communicator"); while the mode is exact,
 * grape_comm_attach / grape_ipc_attach are refused.  After a failure the previous setting stays in force.  With mode = 0,
 * and on a context that never calls this, every entry point launches the kernels it always did and returns the same bits. */
typedef enum grape_traj_derivative { GRAPE_TRAJ_FIRST_ORDER = 0, GRAPE_TRAJ_EXACT = 1 } grape_traj_derivative;
int grape_set_trajectory_derivative(grape_ctx *ctx, int32_t mode);

/* ABI v8 (additive).  The derivative rule of the running cost's gradient (grape_set_running_cost), in every evaluation:
 * grape_eval, grape_eval_device, the batched forms and grape_lbfgs.  GRAPE_TRAJ_FIRST_ORDER (the default) is the rule
 * documented at grape_set_running_cost.  GRAPE_TRAJ_EXACT takes the Frechet derivative DF_t of the map the sweep itself
 * evaluated, as defined above; with X_{k,t} the state BEFORE slice t:
 *   dJ/dx[c,t] = sum_k w_k Re tr( DF_t[W_{k,t}] B'_kc ) ,   W_{k,t} = X_{k,t} Lam_{k,t+1}' ,   B' = -i dt B
 *   Lam_{k,N}  = 2 sum_j rho[N-1,j] y_{k,j,N} R_kj
 *   Lam_{k,s}  = P_{k,s}' Lam_{k,s+1} + 2 sum_j rho[s-1,j] y_{k,j,s} R_kj
 * -- the w-weighted sum over the members of grape_eval_vjp's exact pull-back with the probes R and the cotangents
 * ybar_{k,j,s} = 2 rho[s-1,j] y_{k,j,s}, ybar_{k,j,0} = 0.  One derivative per (member, slice) serves all K controls and all
 * terms.  J itself is unchanged, bit for bit; the penalties, the basis / bounds tails and the ensemble sum work on the
 * result as ever.
 * Served where grape_set_running_cost is served -- family 0 (n = 2, 3, 4), GRAPE_UNITARY_GATE with any m, single-device
 * contexts, member-chunked ones and max_batch > 1 included -- and ALSO on contexts created with gradient = exact, with
 * objective fom or c1 (J never looks at the objective): there grape_set_running_cost is accepted only while this mode is
 * exact (with the default mode it is refused as before, the message names "exact"), and switching back to
 * GRAPE_TRAJ_FIRST_ORDER while a running cost stands on such a context is refused with GRAPE_ERR_UNSUPPORTED.  On a first-order
 * context the exact mode gives F first order and J exact.  Elsewhere mode = GRAPE_TRAJ_EXACT is refused with
 * GRAPE_ERR_UNSUPPORTED and grape_set_running_cost's reason ("dimension", "StateTransfer", "c1", "multi-device",
 * "communicator").  Unchanged: the refusal of a running cost under a risk and of grape_comm_attach / grape_ipc_attach under
 * a running cost, grape_eval_fom's fallback, grape_get_member_results and member_F WITHOUT J (on gradient = exact contexts
 * too: J's rows join a private copy of the members' rows), grape_set_trajectory_derivative and everything grape_eval_vjp /
 * grape_eval_jvp return.
 * Kernels (grape_get_kernel_names tells which ran): the exact instance of running_cost_kernel (running_cost_exact_kernel)
 * stores W_t, summed over the terms, per slice; the running-cost instance of traj_frechet_rows_kernel rebuilds G_t from the
 * physical pulse of the evaluation and writes the K N gradient entries of the member's row; running_cost_fold_kernel
 * (first-order contexts) or running_cost_join_kernel (gradient = exact contexts) joins the rows to the ensemble sum in member
 * order.  Scratch: one n x n c128 block per slice and (control array, member) of a workspace block, shared with the exact
 * trajectory pair (stream order separates the users), grown where the running cost's rows are and counted in
 * grape_info.workspace_bytes.  No atomics: bitwise reproducible call to call, member-chunked = unchunked, host form = device
 * form = one-array batch.
 * A setting like the other grape_set_*: valid any time after grape_create, persists across grape_set_operators, ordered
 * behind an in-flight grape_eval_device, clears the "trajectory valid" flag.  GRAPE_ERR_INVALID_ARG: mode outside {0, 1}.
 * After a failure the previous setting stays in force.  With mode = 0, and on a context that never calls this, every
 * evaluation launches the kernels it always did and returns the same bits. */
int grape_set_running_cost_derivative(grape_ctx *ctx, int32_t mode);

/* Device-resident L-BFGS: stands in for
 *     Optim.optimize(Optim.only_fg!(topt), x0, Optim.LBFGS(), optim_options)       src/solve.jl:138, :244
 * with x, g, the (s, y) history and the line-search trial points kept on the GPU; per evaluation the host
 * reads two scalars (phi, phi').  Optim's LBFGS() defaults are mirrored: memory m = 10, initial inverse-Hessian
 * scaling s'y / y'y, initial step 1 (InitialStatic), g_tol = 1e-8 on |g|_inf, f_tol = x_tol = 0, 1000 iterations, and
 * the line search is Hager-Zhang with LineSearches.jl's constants (delta 0.1, sigma 0.9, rho 5, epsilon 1e-6,
 * gamma 0.66, psi3 0.1, at most 50 evaluations): bracketing, secant^2 and bisection on phi(alpha), phi'(alpha), one
 * GRAPE evaluation per trial step.  line_search:
 *   0  Hager-Zhang; the initial step is taken at once when it satisfies the (approximate) Wolfe conditions
 *   1  Hager-Zhang exactly as Optim runs it behind InitialStatic (`mayterminate` false: the initial step is never
 *      accepted without a second evaluation).  ABI v5: LineSearches.jl's control flow to the letter -- max_linesearch counts
 *      passes of its bracketing / secant^2 loops as `linesearchmax` does (bisections inside a pass are not counted), a
 *      collapsed or flat bracket returns its lower end even at alpha = 0 (status 4: Optim then stops with "x converged"),
 *      a search that runs out of passes ends the run with status 3 as Optim's LineSearchException does (Optim takes the
 *      step of the exception's alpha first; this loop does not), two successive iterations without any change of F end it
 *      with status 1.  oracle/optim_lbfgs.py restates Optim.jl's LBFGS + LineSearches.jl's HagerZhang in NumPy and
 *      tests/test_gpu_lbfgs.py holds this mode to it step length by step length.
 *   2  the factor-2 ladder of ABI v2: `probes` step lengths alpha, alpha/2, ... per BATCHED launch
 *      (grape_config.max_batch >= probes), the largest with sufficient decrease (c1 = 1e-4), preferring the strong Wolfe
 *      curvature condition (c2 = 0.9)
 * Multi-device contexts (n_devices >= 2) and contexts with an attached communicator / mailbox exchange default to modes 0
 * and 1 (one sharded evaluation per trial step); ABI v4: with max_batch >= 2 they take mode 2 as well -- the B probes of a
 * ladder are ONE batched sharded evaluation with ONE exchange of B rows.  The vectors live on the first device (every
 * rank's device).  With grape_comm_attach / grape_ipc_attach all ranks must call grape_lbfgs together (they take identical
 * decisions on identical [G, F]).
 * A Hager-Zhang search that cannot bracket -- the reference's UnitaryGate gradient is not the derivative of its figure
 * of merit -- hands that iteration to the ladder (single-device) or ends with status 3.
 * The gradient is whatever the GRAPE evaluation returns, with the reference's conventions. */
typedef struct grape_lbfgs_options {
    int32_t memory;            /* m; 0 = 10                                              */
    int32_t max_iterations;    /* 0 = 1000                                               */
    double  g_tol;             /* < 0 = 1e-8; stop when |g|_inf <= g_tol                 */
    double  f_tol;             /* stop when |f - f_prev| <= f_tol |f|  (Optim f_tol; 0 = off) */
    int32_t max_linesearch;    /* evaluations per line search before giving up; 0 = 50   */
    int32_t probes;            /* ladder search: step lengths per launch, 1..8; 0 = automatic */
    /* ---- ABI v3 ---- */
    int32_t line_search;       /* 0, 1 Hager-Zhang (see above), 2 ladder                 */
    int32_t reserved;
} grape_lbfgs_options;

typedef struct grape_lbfgs_result {
    double  minimum;           /* Optim's res.minimum                                    */
    double  g_norm;            /* |g|_inf at the minimiser                               */
    double  seconds;           /* wall time of the whole optimisation                    */
    int32_t iterations;
    int32_t evaluations;       /* control arrays evaluated (probes count individually)   */
    int32_t status;            /* 0 g_tol reached, 1 f_tol reached, 2 max_iterations, 3 line search failed,
                                  4 (ABI v5, line_search = 1) zero step: Optim's "x converged" with x_tol = 0 */
    int32_t probes;            /* step lengths per launch actually used                  */
    /* ---- ABI v3 ---- */
    int32_t line_search;       /* the mode that ran                                      */
    int32_t ladder_fallbacks;  /* iterations whose Hager-Zhang search could not bracket  */
} grape_lbfgs_result;

/* x0: host (K,N) f64 initial controls (Problem.guess); x_min: host (K,N) f64, receives res.minimizer.
 * opts may be NULL (all defaults). */
int grape_lbfgs(grape_ctx *ctx, const double *x0, const grape_lbfgs_options *opts, double *x_min,
                grape_lbfgs_result *result);

/* ABI v5.  The last grape_lbfgs run on this context, per iteration: the accepted step length and the number of control
 * arrays evaluated up to the end of that iteration (what Optim's trace shows as `alpha` and f_calls).  *count = iterations
 * recorded; at most `capacity` entries are written (alphas / evals may be NULL). */
int grape_lbfgs_get_trace(const grape_ctx *ctx, double *alphas, int32_t *evals, int32_t capacity, int32_t *count);

/* Debug/parity accessors (valid after an evaluation; needs GRAPE_FLAG_MEMBER_RESULTS; after a batched
 * evaluation they refer to control array 0):
 * per-member unweighted results, as the reference's `gradient[k,:,:]` and the F_k summands:
 *   foms  host f64[E] (nullable)      grads  host f64 (K,N,E) (nullable) */
int grape_get_member_results(grape_ctx *ctx, double *foms, double *grads);

/* The stores the reference keeps per member (src/grape_tools.jl:4-16), for parity tests:
 *   props     c128 (n,n,N)     propagators[t],  t = 0..N-1
 *   states    c128 (n,m,N+1)   fwd_state_store[t], t = 0..N   (states[0] = Xi); the fast flows rebuild
 *                              them on the fly (grape_info.states_stored == 0): then only under
 *                              GRAPE_FLAG_KEEP_COSTATES, else GRAPE_ERR_NOT_READY.
 *   costates  c128 (n,m,N+1)   bwd_costate_store[t], t = 0..N (costates[N] = Xt);
 *                              needs GRAPE_FLAG_KEEP_COSTATES, else GRAPE_ERR_NOT_READY.
 * Any of the three may be NULL. */
int grape_get_trajectory(grape_ctx *ctx, int32_t member, double *props, double *states,
                         double *costates);

/* Sum and count of the sweep kernel's HIP-event durations recorded since the last reset
 * (GRAPE_FLAG_TIME_KERNELS).  Synchronises the recorded events.  reset != 0 clears them. */
int grape_get_kernel_time(grape_ctx *ctx, double *total_ms, int64_t *launches, int32_t reset);

/* The individual durations behind grape_get_kernel_time since its last reset (at most 65536 are kept): the most recent
 * min(capacity, *count) of them, oldest first.  total_ms[i] = all sweep kernels of one evaluation; first_ms[i] (nullable)
 * = the part in front of the chain kernels (n = 5..32: control-sum pre-pass + expm kernel, pw_prop_save!,
 * src/timeevolution.jl:98-110; 0 for n <= 4, where one kernel does everything).  Multi-device contexts report the
 * first device.  *count (nullable) receives the number of durations available. */
int grape_get_kernel_samples(grape_ctx *ctx, double *total_ms, double *first_ms, int64_t capacity, int64_t *count);

/* ABI v4.  The kernels the most recent evaluation launched (grape_eval / grape_eval_device / one batch), by name and in launch
 * order, ';'-separated and NUL-terminated in buf (at most capacity bytes; buf may be NULL): the names rocprofv3 prints, without
 * namespace and template arguments -- e.g. "action_rows_kernel;action_parts_kernel;action_forms_sparse_kernel;reduce_stage1;
 * reduce_stage2".  Which kernels serve src/GRAPE.jl:25-96 depends on what grape_set_operators found (grape_info) and on the
 * ensemble size; benchmarks label their lines with this instead of guessing.  Multi-device contexts report the first device.
 * After grape_lbfgs: the kernels of the run's last evaluation, then the optimiser's own kernels (lbfgs.hip), each name once
 * in order of first launch -- which of the step kernels committed the run's accepted steps.
 * Returns the buffer size the complete list needs (> 0), or a negative status. */
int grape_get_kernel_names(const grape_ctx *ctx, char *buf, int32_t capacity);

/* Host-side cost of the sharded grape_eval of a multi-device context (n_devices >= 2), means over the evaluations since the
 * last reset: out[0] = evaluations, then microseconds: out[1] writing x into every shard's buffer, out[2] first to last
 * shard launch (the issue skew: one issuing thread per shard), out[3] issuing the sum (peer copies + reduction, or
 * the grouped ncclAllReduce + publication), out[4] waiting for [G, F], out[5] the whole call.  out: double[6]. */
int grape_get_group_timing(grape_ctx *ctx, double *out, int32_t reset);

/* Diagnostic (GRAPE_FLAG_PHASE_STAMPS): the stamps of the last evaluation, 10 uint64 per wave,
 * waves ordered (member, wave-in-member): [0..4] shader clock at start / after propagators /
 * after scan / after forward sweep / end, [5],[6] 100 MHz real-time counter at start / end,
 * [7] where the wave ran: HW_REG_XCC_ID << 32 | HW_REG_HW_ID, [8],[9] real-time counter and shader
 * clock at kernel entry, in front of the prologue that stages the operators ([0] and [5] are taken
 * behind it; lane-pair kernel only, 0 from the lane kernel).
 * out: host uint64[capacity]; *count receives the number of values available. */
int grape_get_phase_stamps(grape_ctx *ctx, uint64_t *out, int64_t capacity, int64_t *count);

int grape_get_info(const grape_ctx *ctx, grape_info *info);

/* Message of the last error on this context (ctx == NULL: of the last failed grape_create
 * on the calling thread).  Never NULL. */
const char *grape_last_error(const grape_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* GRAPE_HIP_H */
