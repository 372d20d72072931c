// traj_frechet.hip -- the exact derivative mode of the trajectory pull-back / push-forward (grape_set_trajectory_derivative,
// GRAPE_TRAJ_EXACT) for the small-n family (n = 2, 3, 4) on gfx950: the slice-parallel half of both.
//
// With DF_t[E] the Frechet derivative at G_t = -i dt H_t of the map the sweep evaluated (Taylor-8 at G_t / 2^s, squared s
// times, the sweep's own s per slice; frechet.hpp -- the code path of exact_grad.hip), in direction E:
//   pull-back     G[c,t]  = sum_k Re tr( Lam_{k,t+1}' DF_t[B'_kc] X_{k,t} ) = sum_k Re tr( DF_t[W_{k,t}] B'_kc ),
//                 W_{k,t} = X_{k,t} Lam_{k,t+1}'   -- ONE derivative per slice serves all K controls
//   push-forward  D_{t+1} = P_t D_t + DF_t[V_t] X_t ,   V_t = sum_c xdot[c,t] B'_kc
// The slices do not depend on one another here: one lane (n = 3) or lane pair (n = 2, 4; cmatp.hpp) per (member, slice), a
// wave covers 64 (32) slices of one member, so the member's operators are wave uniform.  Per slice the kernels rebuild G_t
// from the PHYSICAL pulse the evaluation ran on (SweepParams::traj_x), in the sweep's order of the sum, and scale it with the
// same squarings_for(norm1_bound(G)) / s_forced as the sweep.
//   traj_frechet_rows_kernel  reads W_t where the exact instance of trajectory_vjp_kernel left it (SweepParams::traj_w,
//                             chunk-major like the propagators: element e of slice c S + jj at ((k S + jj) n^2 + e) CH + c)
//                             and writes row[t, c] = Re tr(DF_t[W_t] B'_c) into the member's row that vjp_sum_kernel sums
//   traj_frechet_dir_kernel   stores E_t = DF_t[V_t] into the same buffer, for the exact instance of trajectory_jvp_kernel
// The running-cost instance of the rows kernel (grape_set_running_cost_derivative) reads W_t where running_cost_exact_kernel
// left it, for every (control array, member) of an evaluation's launch, rebuilds G_t from that array's pulse and writes
// 2 w_k Re tr(DF_t[W_t] B'_c) into the K N gradient entries of the member's running-cost row.
// No atomics; every number has one fixed evaluation order that does not depend on the member blocks of the launches.  Every
// operation of the direction kernel is linear in xdot (products and FMAs whose addends all carry one factor of it).
#include "cmat.hpp"
#include "cmatp.hpp"
#include "frechet.hpp"
#include "grape_kernels.hpp"

namespace grape {

struct TrajFrechetArgs {
    const double *x;          // (K, N) the physical pulse
    const double *xdot;       // (K, N) the direction in its coordinates (dir kernel)
    double2 *w;               // W_t in (rows kernel) / E_t out (dir kernel), chunk-major
    double *rows;             // K N per member of the launch (rows kernel)
    int32_t K, N, S, CH, s_forced, variant;
    // the running-cost instance of the rows kernel (RC; grape_set_running_cost_derivative): the launch's rows are
    // (control array, member) pairs, row k0 + blockIdx.y = xi E + member -- the operators and the weight are the member's,
    // the pulse is array xi's, and the member's row has K N + 1 entries (the J entry is running_cost_kernel's)
    const double *wts;        // w_k of the launch's members; null: the rows stay unweighted
    int32_t E, k0;
};

template <int N, bool DIR, bool RC = false>
GRAPE_DEV void traj_frechet_lane(const double2 *__restrict__ ops_all, const double *__restrict__ x_all, const TrajFrechetArgs &a)
{
    constexpr int NN = N * N;
    int k = blockIdx.y;                                  // row of W and of the rows
    const int kr = RC ? k + a.k0 : k;
    if constexpr (RC) {                                  // (DIR is false) the member's operators, the array's pulse
        k = kr % a.E;
        x_all += (size_t)(kr / a.E) * a.K * a.N;
    }
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int K = a.K, Nsl = a.N;
    const bool live = t < Nsl;
    const int tt = live ? t : Nsl - 1;                   // surplus lanes repeat the last slice (never stored)
    const double2 *__restrict__ ops = ops_all + (size_t)k * (K + 3) * NN;
    const double2 *__restrict__ opB = ops + NN;
    const int L = tt / a.S, j = tt - L * a.S;
    double2 *__restrict__ wp = a.w + ((size_t)kr * a.S + j) * NN * a.CH + L;
    FrechetLane<N> fr;
    build_generator(fr.G, ops, opB, x_all + (size_t)tt * K, K, a.variant);
    fr.prepare(a.s_forced);
    CMat<N> W, D;
    if (DIR) {
#pragma unroll
        for (int e = 0; e < NN; ++e) { W.re[e] = 0.0; W.im[e] = 0.0; }
        for (int c = 0; c < K; ++c) {
            const double xv = a.xdot[c + (size_t)tt * K];
#pragma unroll
            for (int e = 0; e < NN; ++e) {
                const double2 b = opB[c * NN + e];
                W.re[e] = fma(xv, b.x, W.re[e]);
                W.im[e] = fma(xv, b.y, W.im[e]);
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            const double2 v = wp[(size_t)e * a.CH];
            W.re[e] = v.x;
            W.im[e] = v.y;
        }
    }
    fr.apply(D, W);
    if (DIR) {
        if (live) {
#pragma unroll
            for (int e = 0; e < NN; ++e)
                wp[(size_t)e * a.CH] = make_double2(D.re[e], D.im[e]);
        }
    } else {
        double *__restrict__ row = a.rows + (RC ? (size_t)kr * ((size_t)K * Nsl + 1) : (size_t)k * K * Nsl);
        const double scale = RC ? 2.0 * (a.wts ? a.wts[k] : 1.0) : 1.0;
        for (int c = 0; c < K; ++c) {
            CMat<N> Bc;
#pragma unroll
            for (int e = 0; e < NN; ++e) { const double2 b = opB[c * NN + e]; Bc.re[e] = b.x; Bc.im[e] = b.y; }
            double ar, ai;
            trace_ab(ar, ai, D, Bc);                     // tr(DF[W_t] B'_c); the real part is the gradient entry
            if (live)
                row[(size_t)t * K + c] = RC ? scale * ar : ar;
        }
    }
}

template <int N, bool DIR, bool RC = false>
GRAPE_DEV void traj_frechet_pair(const double2 *__restrict__ ops_all, const double *__restrict__ x_all, const TrajFrechetArgs &a)
{
    constexpr int NN = N * N, NC = N / 2, NE = N * NC;
    const int lane = threadIdx.x, par = lane & 1;
    int k = blockIdx.y;                                  // row of W and of the rows
    const int kr = RC ? k + a.k0 : k;
    if constexpr (RC) {                                  // (DIR is false) the member's operators, the array's pulse
        k = kr % a.E;
        x_all += (size_t)(kr / a.E) * a.K * a.N;
    }
    const int t = blockIdx.x * 32 + (lane >> 1);
    const int K = a.K, Nsl = a.N;
    const bool live = t < Nsl;
    const int tt = live ? t : Nsl - 1;                   // surplus pairs repeat the last slice (never stored)
    const double2 *__restrict__ ops = ops_all + (size_t)k * (K + 3) * NN;
    const double2 *__restrict__ opB = ops + NN;
    int gidx[NE], gidx_t[NE];
    pair_indices<N>(par, gidx, gidx_t);
    const int L = tt / a.S, j = tt - L * a.S;
    double2 *__restrict__ wp = a.w + ((size_t)kr * a.S + j) * NN * a.CH + L;
    FrechetPair<N> fr;
    build_generator_pair(fr.G, ops, opB, x_all + (size_t)tt * K, K, a.variant, gidx);
    fr.prepare(a.s_forced);
    PMat<N> W, D;
    if (DIR) {
#pragma unroll
        for (int e = 0; e < NE; ++e) { W.re[e] = 0.0; W.im[e] = 0.0; }
        for (int c = 0; c < K; ++c) {
            const double xv = a.xdot[c + (size_t)tt * K];
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const double2 b = opB[c * NN + gidx[e]];
                W.re[e] = fma(xv, b.x, W.re[e]);
                W.im[e] = fma(xv, b.y, W.im[e]);
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const double2 v = wp[(size_t)gidx[e] * a.CH];
            W.re[e] = v.x;
            W.im[e] = v.y;
        }
    }
    fr.apply(D, W);
    if (DIR) {
        if (live) {                                      // each lane of the pair stores the columns it owns
#pragma unroll
            for (int e = 0; e < NE; ++e)
                wp[(size_t)gidx[e] * a.CH] = make_double2(D.re[e], D.im[e]);
        }
    } else {
        double *__restrict__ row = a.rows + (RC ? (size_t)kr * ((size_t)K * Nsl + 1) : (size_t)k * K * Nsl);
        const double scale = RC ? 2.0 * (a.wts ? a.wts[k] : 1.0) : 1.0;
        for (int c = 0; c < K; ++c) {
            PMat<N> BT;                                  // B'_c transposed, in the pair layout: tr(D B) = sum D .* B^T
            pair_op_load(BT, opB + c * NN, gidx_t);
            double ar, ai;
            ptrace_elem(ar, ai, D, BT);
            if (live && par == 0)
                row[(size_t)t * K + c] = RC ? scale * ar : ar;
        }
    }
}

// ops_all / x_all are separate `const __restrict__` arguments so that the wave-uniform operator entries can be fetched with
// scalar loads (as in exact_grad.hip)
template <int N, bool RC = false>
__global__ __launch_bounds__(64) void traj_frechet_rows_kernel(const double2 *__restrict__ ops_all, const double *__restrict__ x_all,
                                                               const TrajFrechetArgs a)
{
    if constexpr (N == 3) traj_frechet_lane<N, false, RC>(ops_all, x_all, a);
    else                  traj_frechet_pair<N, false, RC>(ops_all, x_all, a);
}

template <int N>
__global__ __launch_bounds__(64) void traj_frechet_dir_kernel(const double2 *__restrict__ ops_all, const double *__restrict__ x_all,
                                                              const TrajFrechetArgs a)
{
    if constexpr (N == 3) traj_frechet_lane<N, true>(ops_all, x_all, a);
    else                  traj_frechet_pair<N, true>(ops_all, x_all, a);
}

template <int N>
static hipError_t traj_frechet_launch(bool dir, const double2 *ops, const TrajFrechetArgs &a, int E, hipStream_t stream)
{
    const int per = N == 3 ? 64 : 32;                    // slices per wave
    const dim3 grid((a.N + per - 1) / per, E), block(64);
    if (dir) GRAPE_LAUNCH_AS("traj_frechet_dir_kernel", (traj_frechet_dir_kernel<N>), grid, block, 0, stream, ops, a.x, a);
    else     GRAPE_LAUNCH_AS("traj_frechet_rows_kernel", (traj_frechet_rows_kernel<N>), grid, block, 0, stream, ops, a.x, a);
    return hipGetLastError();
}

// the running-cost instance: `rows` (control array, member) pairs, in slabs of the grid's y limit
template <int N>
static hipError_t traj_frechet_launch_rc(const double2 *ops, TrajFrechetArgs a, int rows, hipStream_t stream)
{
    const int per = N == 3 ? 64 : 32;
    for (int k0 = 0; k0 < rows; k0 += 65535) {
        a.k0 = k0;
        const dim3 grid((a.N + per - 1) / per, rows - k0 < 65535 ? rows - k0 : 65535), block(64);
        GRAPE_LAUNCH_AS("traj_frechet_rows_kernel", (traj_frechet_rows_kernel<N, true>), grid, block, 0, stream, ops, a.x, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// dir = false: behind the exact instance of trajectory_vjp_kernel (p.vjp_*); true: in front of that of trajectory_jvp_kernel
// (p.jvp_*).  The members are those of the launch p describes; the workspace decomposition (S, CH) is its sweep's.
hipError_t run_traj_frechet(int n, bool dir, const SweepParams &p, hipStream_t stream)
{
    TrajFrechetArgs a{};
    if (p.rc_only && p.rc_exact) {                       // behind the exact instance of running_cost_kernel (p.rc_*)
        a.x = p.x;                                       // the pulse(s) of this very launch: (K, N, n_x)
        a.w = p.traj_w;
        a.rows = p.rc_rows;
        a.K = p.K;
        a.N = p.N;
        a.S = p.S;
        a.CH = p.rc_CH;
        a.s_forced = p.s_forced;
        a.variant = p.variant;
        a.wts = p.rc_unweighted ? nullptr : p.wts;
        a.E = p.E;
        const long long rows = (long long)p.E * p.n_x;
        if (dir || !a.x || !a.w || !a.rows || !p.ops || !p.wts || a.K < 1 || a.N < 1 || p.E < 1 || p.n_x < 1 || rows > 0x7fffffffll ||
            a.S < 1 || a.CH < 1 || (long long)a.S * a.CH < a.N)
            return hipErrorInvalidConfiguration;
        switch (n) {
        case 2: return traj_frechet_launch_rc<2>(p.ops, a, (int)rows, stream);
        case 3: return traj_frechet_launch_rc<3>(p.ops, a, (int)rows, stream);
        case 4: return traj_frechet_launch_rc<4>(p.ops, a, (int)rows, stream);
        default: return hipErrorInvalidValue;
        }
    }
    a.x = p.traj_x;
    a.xdot = dir ? p.jvp_xdot : nullptr;
    a.w = p.traj_w;
    a.rows = dir ? nullptr : p.vjp_rows;
    a.K = p.K;
    a.N = p.N;
    a.S = p.S;
    a.CH = dir ? p.jvp_CH : p.vjp_CH;
    a.s_forced = p.s_forced;
    a.variant = p.variant;
    if (!a.x || !a.w || !p.ops || (dir ? !a.xdot : !a.rows) || a.K < 1 || a.N < 1 || p.E < 1 || p.E > 65535 || a.S < 1 || a.CH < 1 ||
        (long long)a.S * a.CH < a.N)                     // (every slice lies inside the chunk-major block of its member)
        return hipErrorInvalidConfiguration;
    switch (n) {
    case 2: return traj_frechet_launch<2>(dir, p.ops, a, p.E, stream);
    case 3: return traj_frechet_launch<3>(dir, p.ops, a, p.E, stream);
    case 4: return traj_frechet_launch<4>(dir, p.ops, a, p.E, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace grape
