// traj_chunk.hpp -- the chunk-scan skeleton of the kernels that run behind the small-n sweeps on the propagators those left
// in the workspace: running_cost_kernel, observe_kernel, trajectory_vjp_kernel, trajectory_jvp_kernel, trajectory_hvp_kernel,
// trajectory_gnvp_kernel.
//
// The workspace is chunk-major: element e of slice t = c S + jj of row k at ((k S + jj) n^2 + e) CH + c.  Every kernel of the
// family runs one workgroup per row and one lane per time chunk of S consecutive slices, so every workspace access is
// lane-contiguous, and is built from the steps below:
//   traj_lane            the lane's view of the launch: its slices [lo, hi), its column of the workspace
//   traj_ops             the member's prescaled control operators B'_c and its initial state Xi
//   traj_probes          probe j of the member (shared or per-member probes) and the row step of the (N + 1)-entry probe rows
//   traj_chunk_product   Q_c = P_hi-1 ... P_lo
//   traj_prefix_start    exclusive prefix of the Q_c over lanes: the cumulative propagator at the chunk start
//   traj_start_state     X = U_start Xi
//   traj_walk_store      general flow: the forward walk over the chunk that stores the states
//   traj_affine_suffix   exclusive suffix scan of the affine maps z -> Q_c' z + b_c  (the pull-backs: costates)
//   traj_probe_trace     tr(O' D)
// The forward twin of traj_affine_suffix, the prefix scan of z -> Q_c z + d_c with one offset per tangent direction, is
// written out in its users: trajectory_jvp_kernel (jvp.hip, DB directions) and, in the one-direction form,
// trajectory_hvp_kernel (hvp.hip) and trajectory_gnvp_kernel (gnvp.hip).  As a function of this header it compiled to the same
// arithmetic for the JVP kernel, but the register allocation of the instances with several directions and m >= 2 columns
// came out worse (320 instead of 235 registers at n = m = 2 with 8 directions: one wave per SIMD instead of two).  A
// one-direction function for the other two kernels alone was not tried: their copies are hvp.hip's text, line for line.
// Ragged decompositions: a lane whose chunk starts at or behind N, and the padding lanes behind chunk CH - 1, own no slice
// (cnt = 0: Q = 1, zero offset); the last chunk may be short.  The scans run wave shuffles in a fixed tree and pass wave totals
// through the CALLER's __shared__ arrays, combined in wave order: every number has one fixed evaluation order, whatever the
// kernel.  Each scan through LDS opens with the barrier that ends the previous one's reads, but traj_prefix_start, which is
// the first.
#pragma once
#include "cmat.hpp"
#include "rc_mat.hpp"

namespace grape {

template <int N>
struct TrajLane {
    int L, lane, wave, W;                            // thread of the workgroup, lane of its wave, the wave, waves in the workgroup
    int k, S;                                        // row of the workspace, slices per chunk
    int lo, hi, cnt;                                 // the lane's slices [lo, hi), cnt of them
    size_t stride;                                   // CH: distance of consecutive elements in the workspace
    const double2 *__restrict__ Pw;                  // the lane's column of the propagators

    // the lane's column of another chunk-major array of BLK-element blocks per (row, slice): slot jj at + jj BLK stride,
    // or (slot) its address formed in one piece, where a walk touches the array once per slice
    template <int BLK, typename T>
    GRAPE_DEV T *ws(T *base) const
    {
        return base + (size_t)k * S * BLK * stride + L;
    }
    template <int BLK, typename T>
    GRAPE_DEV T *slot(T *base, int jj) const
    {
        return base + ((size_t)k * S + jj) * BLK * stride + L;
    }
    GRAPE_DEV const double2 *P(int jj) const { return Pw + (size_t)jj * N * N * stride; }
};

// CH is the kernel's own field of SweepParams (rc_CH, obs_CH, vjp_CH, jvp_CH)
template <int N>
GRAPE_DEV TrajLane<N> traj_lane(int CH, int S, int Nsl, const double2 *__restrict__ props, int k)
{
    TrajLane<N> ln;
    ln.L = threadIdx.x;
    ln.lane = ln.L & 63;
    ln.wave = __builtin_amdgcn_readfirstlane(ln.L >> 6);
    ln.W = blockDim.x >> 6;
    ln.k = k;
    ln.S = S;
    // the lane's slices [lo, hi): none for chunks that start at or behind N and for the padding lanes behind chunk CH - 1
    ln.lo = (ln.L < CH && ln.L * S < Nsl) ? ln.L * S : Nsl;
    ln.hi = min(ln.lo + S, Nsl);
    ln.cnt = ln.hi - ln.lo;
    ln.stride = (size_t)CH;
    ln.Pw = props + (size_t)k * S * N * N * ln.stride + ln.L;
    return ln;
}

struct TrajOps {
    const double2 *__restrict__ opB;                 // the K prescaled control operators B'_c = -i dt B_c
    const double2 *__restrict__ opXi;                // the initial state (the first m columns of the zero-padded n x n block)
};

template <int N>
GRAPE_DEV TrajOps traj_ops(const double2 *__restrict__ ops_all, int member, int K)
{
    const double2 *__restrict__ ops = ops_all + (size_t)member * (K + 3) * N * N;
    return TrajOps{ops + N * N, ops + (size_t)(1 + K) * N * N};
}

// probe j of ensemble member kg: shared (n, m, n_obs) or per member (n, m, Etot, n_obs); y_step: entries of one probe's row
struct TrajProbes {
    const double2 *__restrict__ o_mem;
    size_t o_step, y_step;
    GRAPE_DEV const double2 *probe(int j) const { return o_mem + (size_t)j * o_step; }
};

template <int N, int M>
GRAPE_DEV TrajProbes traj_probes(const double2 *__restrict__ o_all, int per_member, int Etot, int kg, int Nsl)
{
    return TrajProbes{o_all + (per_member ? (size_t)kg * N * M : (size_t)0), per_member ? (size_t)Etot * N * M : (size_t)(N * M),
                      (size_t)Nsl + 1};
}

// ---- 1: chunk product
template <int N>
GRAPE_DEV void traj_chunk_product(CMat<N> &Q, const TrajLane<N> &ln)
{
    CMat<N> P, T;
    set_identity(Q);
    for (int jj = 0; jj < ln.cnt; ++jj) {
        rc_load_mat(P, ln.P(jj), ln.stride);
        mul(T, P, Q);
        Q = T;
    }
}

// ---- 2: exclusive prefix of the chunk products over lanes -> U, the cumulative propagator at the chunk start
template <int N>
GRAPE_DEV void traj_prefix_start(CMat<N> &U, const CMat<N> &Q, const TrajLane<N> &ln, double2 (*s_q)[N * N])
{
    CMat<N> inc = Q, T;
    for (int d = 1; d < 64; d <<= 1) {
        shfl_up(U, inc, d);
        if (ln.lane >= d) {
            mul(T, inc, U);
            inc = T;
        }
    }
    shfl_up(U, inc, 1);
    if (ln.lane == 0)
        set_identity(U);
    if (ln.W > 1) {
        if (ln.lane == 63) {
#pragma unroll
            for (int e = 0; e < N * N; ++e)
                s_q[ln.wave][e] = make_double2(inc.re[e], inc.im[e]);
        }
        __syncthreads();
        CMat<N> pre;
        set_identity(pre);
        for (int w = 0; w < ln.wave; ++w) {
            rc_load_lds(inc, &s_q[w][0]);
            mul(T, inc, pre);
            pre = T;
        }
        mul(T, U, pre);
        U = T;
    }
}

// ---- the state at the chunk start, X = U Xi
template <int N, int M>
GRAPE_DEV void traj_start_state(CRect<N, M> &X, const CMat<N> &U, const double2 *__restrict__ opXi)
{
    CRect<N, M> xi;
    rload_uniform(xi, opXi);                         // (the first m columns of the zero-padded n x n block)
    rmul(X, U, xi);
}

// ---- general flow: the forward walk over the chunk, X from the chunk's start state to its end state.  Slot jj of Xw takes
// the state AFTER slice lo + jj, or (BEFORE: the exact derivative modes) the one before it.
template <int N, int M, bool BEFORE>
GRAPE_DEV void traj_walk_store(CRect<N, M> &X, const TrajLane<N> &ln, double2 *__restrict__ Xw)
{
    CMat<N> P;
    CRect<N, M> Xs;
    for (int jj = 0; jj < ln.cnt; ++jj) {
        rc_load_mat(P, ln.P(jj), ln.stride);
        if constexpr (BEFORE)
            rstore_ws(Xw + (size_t)jj * N * M * ln.stride, ln.stride, X);
        rmul(Xs, P, X);
        X = Xs;
        if constexpr (!BEFORE)
            rstore_ws(Xw + (size_t)jj * N * M * ln.stride, ln.stride, X);
    }
}

// ---- exclusive suffix scan over lanes of the affine maps z -> Q_c' z + b_c, composition (Q1' Q2', Q1' b2 + b1) in a fixed
// tree (shuffles inside a wave, wave totals through LDS, combined last wave first): Lin, the costate that enters the chunk
// on the right
template <int N, int M>
GRAPE_DEV void traj_affine_suffix(CRect<N, M> &Lin, const CMat<N> &Q, const CRect<N, M> &bvec, const TrajLane<N> &ln,
                                  double2 (*s_q)[N * N], double2 (*s_v)[N * M])
{
    constexpr int NN = N * N, NM = N * M;
    const int lane = ln.lane;
    CMat<N> G = Q, Go, T;
    CRect<N, M> v = bvec, vo, Tm;
    for (int d = 1; d < 64; d <<= 1) {
        shfl_down(Go, G, d);
        rshfl_down(vo, v, d);
        if (lane + d < 64) {                         // [L, L+d) then [L+d, L+2d):  (Go G)' z + (G' vo + v)
            rmul_ah(Tm, G, vo);
#pragma unroll
            for (int e = 0; e < NM; ++e) {
                v.re[e] += Tm.re[e];
                v.im[e] += Tm.im[e];
            }
            mul(T, Go, G);
            G = T;
        }
    }
    shfl_down(Go, G, 1);                             // the lanes behind this one, inside the wave
    rshfl_down(vo, v, 1);
    if (lane == 63) {
        set_identity(Go);
        rzero(vo);
    }
    if (ln.W > 1) {
        __syncthreads();                             // (the previous readers of s_q / s_v are done)
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < NN; ++e)
                s_q[ln.wave][e] = make_double2(G.re[e], G.im[e]);
#pragma unroll
            for (int e = 0; e < NM; ++e)
                s_v[ln.wave][e] = make_double2(v.re[e], v.im[e]);
        }
        __syncthreads();
        CRect<N, M> z;
        rzero(z);
        for (int w = ln.W - 1; w > ln.wave; --w) {   // what enters this wave on the right, last wave first
            rc_load_lds(G, &s_q[w][0]);
            rmul_ah(Tm, G, z);
#pragma unroll
            for (int e = 0; e < NM; ++e) {
                const double2 vv = s_v[w][e];
                z.re[e] = Tm.re[e] + vv.x;
                z.im[e] = Tm.im[e] + vv.y;
            }
        }
        rmul_ah(Tm, Go, z);
#pragma unroll
        for (int e = 0; e < NM; ++e) {
            Lin.re[e] = Tm.re[e] + vo.re[e];
            Lin.im[e] = Tm.im[e] + vo.im[e];
        }
    } else {
        Lin = vo;
    }
}

// ---- tr(O' D) of one probe (wave-uniform: scalar loads)
template <int N, int M>
GRAPE_DEV double2 traj_probe_trace(const double2 *__restrict__ o, const CRect<N, M> &D)
{
    double yr = 0.0, yi = 0.0;
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        const double2 v = o[e];
        yr = fma(v.x, D.re[e], yr);
        yr = fma(v.y, D.im[e], yr);
        yi = fma(v.x, D.im[e], yi);
        yi = fma(-v.y, D.re[e], yi);
    }
    return make_double2(yr, yi);
}

}  // namespace grape
