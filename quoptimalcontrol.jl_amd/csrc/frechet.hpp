// frechet.hpp -- the Frechet derivative of the sweep's own expm evaluation (Taylor-8 at G / 2^s, squared s times; cmat.hpp:
// expm_t8), operation by operation, for whole matrices per lane (n = 3) and for the lane-pair layout (n = 2, 4; cmatp.hpp).
// Shared by the exact gradient of the main objective (exact_grad.hip) and by the exact derivative mode of the trajectory
// pull-back / push-forward (traj_frechet.hip): one code path, one evaluation order.
//
// The map G -> P is a POLYNOMIAL F in G, and for a polynomial
//     tr( DF_G[B] W ) = tr( DF_G[W] B )        (every term  tr(G^j B G^(k-1-j) W) = tr(G^(k-1-j) W G^j B), summed over j)
// -- so ONE derivative in a direction W serves any number of control operators, each of which is left with a trace.
#pragma once
#include "cmat.hpp"
#include "cmatp.hpp"

namespace grape {

template <int N>
GRAPE_DEV void lin2(CMat<N> &o, double a, const CMat<N> &x, double b, const CMat<N> &y)
{
#pragma unroll
    for (int e = 0; e < N * N; ++e) {
        o.re[e] = fma(a, x.re[e], b * y.re[e]);
        o.im[e] = fma(a, x.im[e], b * y.im[e]);
    }
}

template <int N>
GRAPE_DEV void acc(CMat<N> &o, double a, const CMat<N> &x)
{
#pragma unroll
    for (int e = 0; e < N * N; ++e) {
        o.re[e] = fma(a, x.re[e], o.re[e]);
        o.im[e] = fma(a, x.im[e], o.im[e]);
    }
}

// o += a * b
template <int N>
GRAPE_DEV void mul_acc(CMat<N> &o, const CMat<N> &a, const CMat<N> &b)
{
    CMat<N> t;
    mul(t, a, b);
    acc(o, 1.0, t);
}

// tr(A * B) = sum_ij A[i,j] B[j,i]
template <int N>
GRAPE_DEV void trace_ab(double &zr, double &zi, const CMat<N> &a, const CMat<N> &b)
{
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double ar = a.re[i + j * N], ai = a.im[i + j * N];
            const double br = b.re[j + i * N], bi = b.im[j + i * N];
            sr = fma(ar, br, sr); sr = fma(-ai, bi, sr);
            si = fma(ar, bi, si); si = fma(ai, br, si);
        }
    zr = sr;
    zi = si;
}

// generator of one slice, G = A' + sum_c x[c] B'_c in the sweep's order of the sum (variant 0: the drift last).
// ops: the member's [A' | B'_0 ..], opB = ops + n^2, xt: the K controls of the slice
template <int N>
GRAPE_DEV void build_generator(CMat<N> &G, const double2 *__restrict__ ops, const double2 *__restrict__ opB,
                               const double *__restrict__ xt, int K, int variant)
{
    constexpr int NN = N * N;
    if (variant == 0) {
#pragma unroll
        for (int e = 0; e < NN; ++e) { G.re[e] = 0.0; G.im[e] = 0.0; }
    } else {
#pragma unroll
        for (int e = 0; e < NN; ++e) { const double2 a = ops[e]; G.re[e] = a.x; G.im[e] = a.y; }
    }
    for (int c = 0; c < K; ++c) {
        const double xv = xt[c];
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            const double2 b = opB[c * NN + e];
            G.re[e] = fma(b.x, xv, G.re[e]);
            G.im[e] = fma(b.y, xv, G.im[e]);
        }
    }
    if (variant == 0) {
#pragma unroll
        for (int e = 0; e < NN; ++e) { const double2 a = ops[e]; G.re[e] += a.x; G.im[e] += a.y; }
    }
}

// Whole matrices per lane.  G: the slice's generator (build_generator); prepare() scales it like the sweep (the same
// squarings_for(norm1_bound(G)) / s_forced) and forms the shared part of the Taylor-8 evaluation; apply() is DF_G[W].
template <int N>
struct FrechetLane {
    CMat<N> G, A2, T1, U, T2, Ps;
    int s;
    double sc;

    GRAPE_DEV void prepare(int s_forced)
    {
        constexpr int NN = N * N;
        s = s_forced >= 0 ? s_forced : squarings_for(norm1_bound(G));
        sc = s > 0 ? ldexp(1.0, -s) : 1.0;
#pragma unroll
        for (int e = 0; e < NN; ++e) { G.re[e] *= sc; G.im[e] *= sc; }
        CMat<N> A4;
        mul(A2, G, G);
        lin2(T1, kX1, G, kX2, A2);
        mul(A4, A2, T1);
        lin2(U, kX3, A2, 1.0, A4);
        lin2(T2, kX5, G, kX6, A2);
        acc(T2, kX7, A4);
#pragma unroll
        for (int i = 0; i < N; ++i) T2.re[i + i * N] += kX4;
        // value at the scaled point (needed by the squaring chain rule): Ps = U T2 + G + y2 A2 + I
        mul(Ps, U, T2);
        acc(Ps, 1.0, G);
        acc(Ps, kY2, A2);
#pragma unroll
        for (int i = 0; i < N; ++i) Ps.re[i + i * N] += 1.0;
    }

    GRAPE_DEV void apply(CMat<N> &dP, const CMat<N> &W) const
    {
        constexpr int NN = N * N;
        CMat<N> E, tmp;                                  // direction, scaled like G
#pragma unroll
        for (int e = 0; e < NN; ++e) { E.re[e] = sc * W.re[e]; E.im[e] = sc * W.im[e]; }
        CMat<N> dA2, dT1, dA4, dU, dT2;
        mul(dA2, E, G);
        mul_acc(dA2, G, E);
        lin2(dT1, kX1, E, kX2, dA2);
        mul(dA4, dA2, T1);
        mul_acc(dA4, A2, dT1);
        lin2(dU, kX3, dA2, 1.0, dA4);
        lin2(dT2, kX5, E, kX6, dA2);
        acc(dT2, kX7, dA4);
        mul(dP, dU, T2);
        mul_acc(dP, U, dT2);
        acc(dP, 1.0, E);
        acc(dP, kY2, dA2);
        CMat<N> Pq = Ps;                                 // undo the scaling: P <- P^2, dP <- dP P + P dP
        for (int i = 0; i < s; ++i) {
            mul(tmp, dP, Pq);
            mul_acc(tmp, Pq, dP);
            dP = tmp;
            mul(tmp, Pq, Pq);
            Pq = tmp;
        }
    }
};

// ---- n = 2, 4: the same evaluation on LANE PAIRS (cmatp.hpp: lane parity p owns n/2 columns of every matrix, the partner's
// half comes through DPP).  With whole 4 x 4 matrices per lane the evaluation above holds a dozen 64-register matrices: 512
// registers and 1.1 - 2.3 KB of scratch per lane.  A pair-split matrix is 32 registers; the intermediates are sequenced so
// that at most eleven are alive.
template <int N>
GRAPE_DEV void plin2(PMat<N> &o, double a, const PMat<N> &x, double b, const PMat<N> &y)
{
#pragma unroll
    for (int e = 0; e < N * PMat<N>::NC; ++e) {
        o.re[e] = fma(a, x.re[e], b * y.re[e]);
        o.im[e] = fma(a, x.im[e], b * y.im[e]);
    }
}

template <int N>
GRAPE_DEV void pacc(PMat<N> &o, double a, const PMat<N> &x)
{
#pragma unroll
    for (int e = 0; e < N * PMat<N>::NC; ++e) {
        o.re[e] = fma(a, x.re[e], o.re[e]);
        o.im[e] = fma(a, x.im[e], o.im[e]);
    }
}

// o += a * b   (a's partner half fetched here)
template <int N>
GRAPE_DEV void pmul_acc(PMat<N> &o, const PMat<N> &a, const PMat<N> &b)
{
    PMat<N> par, t;
    fetch_partner(par, a);
    pmul(t, a, par, b);
    pacc(o, 1.0, t);
}

template <int N>
GRAPE_DEV void pmul_f(PMat<N> &o, const PMat<N> &a, const PMat<N> &b)
{
    PMat<N> par;
    fetch_partner(par, a);
    pmul(o, a, par, b);
}

// tr(A B) = sum_ij A[i,j] B[j,i]: the pair layout of B^T is not at hand, so through  tr(A B) = tr((A')' B): conj-transpose
// products are what cmatp.hpp has -- here B comes from memory, loaded directly TRANSPOSED (pair_indices' gidx_t)
template <int N>
GRAPE_DEV void ptrace_elem(double &zr, double &zi, const PMat<N> &a, const PMat<N> &bt)
{
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int e = 0; e < N * PMat<N>::NC; ++e) {
        sr = fma(a.re[e], bt.re[e], sr);
        sr = fma(-a.im[e], bt.im[e], sr);
        si = fma(a.re[e], bt.im[e], si);
        si = fma(a.im[e], bt.re[e], si);
    }
    zr = sr + pair_swap(sr);
    zi = si + pair_swap(si);
}

// local element (r, jl) of the pair layout <-> global (i, j), column-major i + j n; gidx_t: the transposed matrix' element
template <int N>
GRAPE_DEV void pair_indices(int par, int (&gidx)[N * (N / 2)], int (&gidx_t)[N * (N / 2)])
{
    constexpr int NC = N / 2;
#pragma unroll
    for (int jl = 0; jl < NC; ++jl)
#pragma unroll
        for (int r = 0; r < N; ++r) {
            const int i = (((r / NC) ^ par) * NC) + (r % NC), j = par * NC + jl;
            gidx[r + jl * N] = i + j * N;
            gidx_t[r + jl * N] = j + i * N;
        }
}

// m = the lane's part of the n x n matrix at src (wave-uniform or per-lane base), elements picked by idx
template <int N>
GRAPE_DEV void pair_op_load(PMat<N> &m, const double2 *__restrict__ src, const int (&idx)[N * (N / 2)])
{
#pragma unroll
    for (int e = 0; e < N * (N / 2); ++e) {
        const double2 v = src[idx[e]];
        m.re[e] = v.x;
        m.im[e] = v.y;
    }
}

// generator of one slice in the pair layout (the sweep's order of the sum), see build_generator
template <int N>
GRAPE_DEV void build_generator_pair(PMat<N> &G, const double2 *__restrict__ ops, const double2 *__restrict__ opB,
                                    const double *__restrict__ xt, int K, int variant, const int (&gidx)[N * (N / 2)])
{
    constexpr int NN = N * N, NE = N * (N / 2);
    if (variant == 0) {
#pragma unroll
        for (int e = 0; e < NE; ++e) { G.re[e] = 0.0; G.im[e] = 0.0; }
    } else {
        pair_op_load(G, ops, gidx);
    }
    for (int c = 0; c < K; ++c) {
        const double xv = xt[c];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const double2 b = opB[c * NN + gidx[e]];
            G.re[e] = fma(b.x, xv, G.re[e]);
            G.im[e] = fma(b.y, xv, G.im[e]);
        }
    }
    if (variant == 0) {
#pragma unroll
        for (int e = 0; e < NE; ++e) { const double2 a = ops[gidx[e]]; G.re[e] += a.x; G.im[e] += a.y; }
    }
}

template <int N>
struct FrechetPair {
    static constexpr int NC = N / 2, NE = N * NC;
    PMat<N> G, A2, A4, T1;
    int s;
    double sc;

    GRAPE_DEV void prepare(int s_forced)
    {
        s = s_forced >= 0 ? s_forced : squarings_for(pnorm1_bound(G));
        sc = s > 0 ? ldexp(1.0, -s) : 1.0;
#pragma unroll
        for (int e = 0; e < NE; ++e) { G.re[e] *= sc; G.im[e] *= sc; }
        pmul_f(A2, G, G);
        plin2(T1, kX1, G, kX2, A2);
        pmul_f(A4, A2, T1);
    }
    // U = x3 A2 + A4 and T2 = x5 G + x6 A2 + x7 A4 + x4 I are rebuilt where they are used (two registers sets less alive)
    GRAPE_DEV void make_U(PMat<N> &U) const { plin2(U, kX3, A2, 1.0, A4); }
    GRAPE_DEV void make_T2(PMat<N> &T2) const
    {
        plin2(T2, kX5, G, kX6, A2);
        pacc(T2, kX7, A4);
#pragma unroll
        for (int jl = 0; jl < NC; ++jl) T2.re[jl + jl * N] += kX4;      // own diagonal: local row (0, jl) of column jl
    }

    GRAPE_DEV void apply(PMat<N> &dP, const PMat<N> &W) const
    {
        PMat<N> E, dA2, dT, dA4, Tm;
#pragma unroll
        for (int e = 0; e < NE; ++e) { E.re[e] = sc * W.re[e]; E.im[e] = sc * W.im[e]; }
        pmul_f(dA2, E, G);
        pmul_acc(dA2, G, E);
        plin2(dT, kX1, E, kX2, dA2);                     // dT1
        pmul_f(dA4, dA2, T1);
        pmul_acc(dA4, A2, dT);
        plin2(dT, kX3, dA2, 1.0, dA4);                   // dU
        make_T2(Tm);
        pmul_f(dP, dT, Tm);                              // dU T2
        plin2(dT, kX5, E, kX6, dA2);                     // dT2
        pacc(dT, kX7, dA4);
        make_U(Tm);
        pmul_acc(dP, Tm, dT);                            // + U dT2
        pacc(dP, 1.0, E);
        pacc(dP, kY2, dA2);
        if (s > 0) {                                     // undo the scaling: P <- P^2, dP <- dP P + P dP
            PMat<N> Pq, T2;
            make_T2(T2);
            pmul_f(Pq, Tm, T2);                          // value at the scaled point: U T2 + G + y2 A2 + I
            pacc(Pq, 1.0, G);
            pacc(Pq, kY2, A2);
#pragma unroll
            for (int jl = 0; jl < NC; ++jl) Pq.re[jl + jl * N] += 1.0;
            for (int i = 0; i < s; ++i) {
                pmul_f(dT, dP, Pq);
                pmul_acc(dT, Pq, dP);
                dP = dT;
                pmul_f(dT, Pq, Pq);
                Pq = dT;
            }
        }
    }
};

}  // namespace grape
