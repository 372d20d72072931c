// rc_mat.hpp -- n x m complex blocks in registers and their workspace accessors, shared by the kernels that run behind the
// small-n sweeps on the propagators those left in the workspace (running_cost.hip, observe.hip, vjp.hip, jvp.hip; the steps
// those kernels share are in traj_chunk.hpp).
#pragma once
#include "cmat.hpp"

namespace grape {

// n x m complex block (the states, costates and probe matrices), column-major e = i + j n
template <int N, int M>
struct CRect {
    double re[N * M];
    double im[N * M];
};

template <int N, int M>
GRAPE_DEV void rzero(CRect<N, M> &a)
{
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        a.re[e] = 0.0;
        a.im[e] = 0.0;
    }
}

// C = A B  (A n x n, B n x m)
template <int N, int M>
GRAPE_DEV void rmul(CRect<N, M> &c, const CMat<N> &a, const CRect<N, M> &b)
{
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double ar = a.re[i + k * N], ai = a.im[i + k * N];
                const double br = b.re[k + j * N], bi = b.im[k + j * N];
                sr = fma(ar, br, sr);
                sr = fma(-ai, bi, sr);
                si = fma(ar, bi, si);
                si = fma(ai, br, si);
            }
            c.re[i + j * N] = sr;
            c.im[i + j * N] = si;
        }
}

// X <- A X, one column at a time (column j of the product needs column j of X only: the temporary is one column, not a block)
template <int N, int M>
GRAPE_DEV void rmul_inplace(CRect<N, M> &x, const CMat<N> &a)
{
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double tr[N], ti[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double ar = a.re[i + k * N], ai = a.im[i + k * N];
                const double br = x.re[k + j * N], bi = x.im[k + j * N];
                sr = fma(ar, br, sr);
                sr = fma(-ai, bi, sr);
                si = fma(ar, bi, si);
                si = fma(ai, br, si);
            }
            tr[i] = sr;
            ti[i] = si;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            x.re[i + j * N] = tr[i];
            x.im[i + j * N] = ti[i];
        }
    }
}

// C += A B  (A n x n, B n x m)
template <int N, int M>
GRAPE_DEV void rmul_acc(CRect<N, M> &c, const CMat<N> &a, const CRect<N, M> &b)
{
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double sr = c.re[i + j * N], si = c.im[i + j * N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double ar = a.re[i + k * N], ai = a.im[i + k * N];
                const double br = b.re[k + j * N], bi = b.im[k + j * N];
                sr = fma(ar, br, sr);
                sr = fma(-ai, bi, sr);
                si = fma(ar, bi, si);
                si = fma(ai, br, si);
            }
            c.re[i + j * N] = sr;
            c.im[i + j * N] = si;
        }
}

// C = A^H B
template <int N, int M>
GRAPE_DEV void rmul_ah(CRect<N, M> &c, const CMat<N> &a, const CRect<N, M> &b)
{
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double ar = a.re[k + i * N], ai = -a.im[k + i * N];
                const double br = b.re[k + j * N], bi = b.im[k + j * N];
                sr = fma(ar, br, sr);
                sr = fma(-ai, bi, sr);
                si = fma(ar, bi, si);
                si = fma(ai, br, si);
            }
            c.re[i + j * N] = sr;
            c.im[i + j * N] = si;
        }
}

// C (n x n) = X Lam^H  (both n x m)
template <int N, int M>
GRAPE_DEV void rmul_a_bh(CMat<N> &c, const CRect<N, M> &a, const CRect<N, M> &b)
{
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const double ar = a.re[i + k * N], ai = a.im[i + k * N];
                const double br = b.re[j + k * N], bi = -b.im[j + k * N];
                sr = fma(ar, br, sr);
                sr = fma(-ai, bi, sr);
                si = fma(ar, bi, si);
                si = fma(ai, br, si);
            }
            c.re[i + j * N] = sr;
            c.im[i + j * N] = si;
        }
}

template <int N, int M>
GRAPE_DEV void rshfl_down(CRect<N, M> &dst, const CRect<N, M> &src, int delta)
{
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        dst.re[e] = __shfl_down(src.re[e], delta, 64);
        dst.im[e] = __shfl_down(src.im[e], delta, 64);
    }
}

template <int N, int M>
GRAPE_DEV void rshfl_up(CRect<N, M> &dst, const CRect<N, M> &src, int delta)
{
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        dst.re[e] = __shfl_up(src.re[e], delta, 64);
        dst.im[e] = __shfl_up(src.im[e], delta, 64);
    }
}

template <int N, int M>
GRAPE_DEV void rload_uniform(CRect<N, M> &m, const double2 *__restrict__ src)
{
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        const double2 v = src[e];
        m.re[e] = v.x;
        m.im[e] = v.y;
    }
}

template <int N>
GRAPE_DEV void rc_load_mat(CMat<N> &m, const double2 *__restrict__ base, size_t stride)
{
#pragma unroll
    for (int e = 0; e < N * N; ++e) {
        const double2 v = base[e * stride];
        m.re[e] = v.x;
        m.im[e] = v.y;
    }
}

template <int N>
GRAPE_DEV void rc_load_lds(CMat<N> &m, const double2 *src)
{
#pragma unroll
    for (int e = 0; e < N * N; ++e) {
        const double2 v = src[e];
        m.re[e] = v.x;
        m.im[e] = v.y;
    }
}

template <int N, int M>
GRAPE_DEV void rload_ws(CRect<N, M> &m, const double2 *__restrict__ base, size_t stride)
{
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        const double2 v = base[e * stride];
        m.re[e] = v.x;
        m.im[e] = v.y;
    }
}

template <int N, int M>
GRAPE_DEV void rstore_ws(double2 *__restrict__ base, size_t stride, const CRect<N, M> &m)
{
#pragma unroll
    for (int e = 0; e < N * M; ++e)
        base[e * stride] = make_double2(m.re[e], m.im[e]);
}

// workgroup size limit of those kernels (traj_max_threads, grape_kernels.hpp: the host layer's LDS budget uses it too)
template <int N>
struct RcTraits {
    static_assert(N >= 2 && N <= 4, "the small-n family");
    static constexpr int MAXT = traj_max_threads(N);
};

}  // namespace grape
