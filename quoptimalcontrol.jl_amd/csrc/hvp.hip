// hvp.hip -- the directional derivative of the trajectory pull-back (grape_eval_hvp: second-order products of the read-out) for
// the small-n family (n = 2, 3, 4; n x m states under left multiplication, UnitaryGate) on gfx950.
//
//   the pull-back of grape_eval_vjp, differentiated along a direction xdot of the PHYSICAL pulse (the host layer has applied
//   the pulse map's tangent) and a tangent (ybar_dot, Xbar_dot) of its cotangents, under the rule of the first-order pair,
//   Pdot_s = V_s P_s with V_s = sum_c xdot[c,s] B'_{k,c},  B' = -i dt B:
//   Xd_0    = 0 ,                              Xd_{s+1}  = P_s Xd_s + V_s X_{s+1}                       (grape_eval_jvp's tangent)
//   Lam_N   = Xbar + sum_j ybar[N,j] O_j ,     Lam_s     = P_s' Lam_{s+1} + sum_j ybar[s,j] O_j          (grape_eval_vjp's costate)
//   Lamd_N  = Xbar_dot + sum_j ybar_dot[N,j] O_j ,
//   Lamd_s  = P_s' (Lamd_{s+1} + V_s' Lam_{s+1}) + sum_j ybar_dot[s,j] O_j
//   Gdot[c,t] = sum_k Re tr(B'_{k,c} (X_{k,t+1} Lamd_{k,t+1}' + Xd_{k,t+1} Lam_{k,t+1}'))
//
// It runs behind the sweep of the same launch and reads the propagators P_t that sweep left in the workspace (chunk-major).
// The decomposition and the steps marked * are traj_chunk.hpp's: one workgroup per member of the launch, one lane per time
// chunk of S consecutive slices, every workspace access lane-contiguous:
//   1  ONE forward walk over the chunk in relative form: the chunk product Q_c and the chunk tangent
//      R_c = sum_j P_hi-1 .. P_j+1 V_j P_j .. P_lo (the first pass of jvp.hip)
//   2* exclusive prefix of the Q_c: X at the chunk start; d_c = R_c X_lo
//   3  exclusive prefix scan of the affine maps z -> Q_c z + d_c (jvp.hip's, one direction): Xd at the chunk start
//   4  forward walk on (X, Xd) from the true start values.  General flow: [X_t+1 | Xd_t+1] of every slice goes into the
//      scratch (SweepParams::hvp_xs).  Unitary flow: only the pair at the chunk END is kept (one slot per lane of the same
//      scratch, which also takes Lam_in across step 8: none of the three blocks is live in registers across a scan -- with
//      them the n = m = 3 instance spilled) and the last walk steps back with X_t = P_t' X_t+1,
//      Xd_t = P_t' (Xd_t+1 - V_t X_t+1)
//   5  backward walk of Lam from 0: b_c;  6* suffix scan of z -> Q_c' z + b_c: Lam that enters the chunk on the right
//   7  backward walk of (Lam, Lamd) from (Lam_in, 0): bt_c = R_c' Lam_in + bd_c, the chunk's contribution to Lamd
//   8* suffix scan of z -> Q_c' z + bt_c: Lamd that enters the chunk on the right
//   9  the walk from (Lam_in, Lamd_in) with X and Xd: the K entries of the member's row per slice
// Steps 6 and 8 are the ONE suffix scan of the pair maps (Lam, Lamd) -> (Q' Lam + b, Q' Lamd + R' Lam + bd), composition
// (Q2 Q1, Q2 R1 + R2 Q1, Q1' b2 + b1, Q1' bd2 + R1' b2 + bd1), taken apart: the Lam half does not depend on the Lamd half, and
// with Lam_in known the Lamd half is an affine map of Lamd alone.  Two runs of traj_affine_suffix keep the scan state at
// three n x n and three n x m blocks instead of four and four (which does not fit the register file at n = m = 4 next to what
// lives across the scan), do not carry R through the tree (two matrix products per level less) and reuse the tree every
// pull-back of the family is reduced in.  The price is one more walk of Lam alone.
// Every number has one fixed evaluation order; the members' rows are unweighted, written with plain vector stores, and summed
// by vjp_sum_kernel in the tree fixed by the members' ensemble indices: a member-chunked launch sequence gives the bits of an
// unchunked one.  Every operation that touches (xdot, ybar_dot, Xbar_dot) is linear in that triple (products and FMAs whose
// addends all carry one factor of it): twice the triple gives twice the bits, the negated triple the negated bits.
#include "cmat.hpp"
#include "grape_kernels.hpp"
#include "rc_mat.hpp"
#include "traj_chunk.hpp"

namespace grape {

// C += A^H B
template <int N, int M>
GRAPE_DEV void hvp_mul_ah_acc(CRect<N, M> &c, const CMat<N> &a, const CRect<N, M> &b)
{
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double sr = c.re[i + j * N], si = c.im[i + j * N];
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

// C -= A B
template <int N, int M>
GRAPE_DEV void hvp_mul_sub(CRect<N, M> &c, const CMat<N> &a, const CRect<N, M> &b)
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
                sr = fma(-ar, br, sr);
                sr = fma(ai, bi, sr);
                si = fma(-ar, bi, si);
                si = fma(-ai, br, si);
            }
            c.re[i + j * N] = sr;
            c.im[i + j * N] = si;
        }
}

// X <- A^H X, one column at a time (the temporary is one column, not a block)
template <int N, int M>
GRAPE_DEV void hvp_mul_ah_inplace(CRect<N, M> &x, const CMat<N> &a)
{
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double tr[N], ti[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double ar = a.re[k + i * N], ai = -a.im[k + i * N];
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

// C (n x n) += A B^H  (both n x m)
template <int N, int M>
GRAPE_DEV void hvp_mul_a_bh_acc(CMat<N> &c, const CRect<N, M> &a, const CRect<N, M> &b)
{
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double sr = c.re[i + j * N], si = c.im[i + j * N];
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

// V = sum_c xd[c] B'_c  (opB: the member's K prescaled control operators, wave-uniform; xd: the slice's row of xdot)
template <int N>
GRAPE_DEV void hvp_direction(CMat<N> &V, const double *__restrict__ xd, const double2 *__restrict__ opB, int K)
{
#pragma unroll
    for (int e = 0; e < N * N; ++e) {
        V.re[e] = 0.0;
        V.im[e] = 0.0;
    }
#pragma unroll 1
    for (int c = 0; c < K; ++c) {
        const double a = xd[c];
#pragma unroll
        for (int e = 0; e < N * N; ++e) {
            const double2 b = opB[c * N * N + e];
            V.re[e] = fma(a, b.x, V.re[e]);
            V.im[e] = fma(a, b.y, V.im[e]);
        }
    }
}

// one slice of the tangent recurrence on an n x c block:  X <- P X,  D <- P D + V X  (jvp.hip's step, one direction)
template <int N, int C>
GRAPE_DEV void hvp_step(CRect<N, C> &X, CRect<N, C> &D, const double2 *__restrict__ Pt, size_t stride, const double *__restrict__ xd,
                        const double2 *__restrict__ opB, int K)
{
    CMat<N> P;
    rc_load_mat(P, Pt, stride);
    rmul_inplace(X, P);
    rmul_inplace(D, P);
    hvp_direction(P, xd, opB, K);
    rmul_acc(D, P, X);
}

// Lam += c O  (one probe, wave-uniform; the VJP kernel's source term)
template <int N, int M>
GRAPE_DEV void hvp_source(CRect<N, M> &Lam, const double2 c, const double2 *__restrict__ o)
{
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        const double2 v = o[e];
        Lam.re[e] = fma(c.x, v.x, fma(-c.y, v.y, Lam.re[e]));
        Lam.im[e] = fma(c.x, v.y, fma(c.y, v.x, Lam.im[e]));
    }
}

template <int N, int M>
GRAPE_DEV void hvp_add_block(CRect<N, M> &Lam, const double2 *__restrict__ xb)
{
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        const double2 v = xb[e];
        Lam.re[e] += v.x;
        Lam.im[e] += v.y;
    }
}

// ops_all / o_all are separate `const __restrict__` arguments so that the wave-uniform operator and probe entries can be
// fetched with scalar loads (as in vjp.hip).  UNI: every propagator is unitary.
template <int N, int M, bool UNI, int MAXT>
__global__ __launch_bounds__(MAXT) void trajectory_hvp_kernel(const double2 *__restrict__ ops_all,
                                                              const double2 *__restrict__ o_all,
                                                              const double2 *__restrict__ ybar_all,
                                                              const double2 *__restrict__ xbar_all,
                                                              const double2 *__restrict__ ybd_all,
                                                              const double2 *__restrict__ xbd_all,
                                                              const double *__restrict__ xdot, const SweepParams p)
{
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    __shared__ double2 s_q[MAXW][NN];              // wave totals: prefix products, then the affine maps' matrices ...
    __shared__ double2 s_v[MAXW][NM];              // ... and their offsets

    const int K = p.K, Nsl = p.N, n_obs = (ybar_all || ybd_all) ? p.vjp_n : 0;
    const int k = blockIdx.x;                        // member within the launch: row of the workspace and of the rows
    const int kg = k + p.vjp_E0;                     // member of the ensemble: row of the probes and of the cotangents
    const TrajLane<N> ln = traj_lane<N>(p.vjp_CH, p.S, Nsl, p.props, k);
    const int lo = ln.lo, cnt = ln.cnt;
    const size_t stride = ln.stride;
    // general flow: slot jj = [X | Xd] behind slice lo + jj; unitary flow: ONE slot per lane, [X | Xd] at the chunk end and
    // Lam_in across the second suffix scan (only lanes that own a slice touch it: the padding lanes behind chunk CH - 1
    // have no column)
    double2 *__restrict__ Xw = UNI ? p.hvp_xs + (size_t)k * 3 * NM * stride + ln.L : ln.template ws<2 * NM>(p.hvp_xs);
    const TrajOps op = traj_ops<N>(ops_all, k, K);
    const double2 *__restrict__ opB = op.opB;
    const TrajProbes pr = traj_probes<N, M>(o_all, p.vjp_per_member, p.vjp_Etot, kg, Nsl);
    const size_t y_step = pr.y_step;
    const double2 *__restrict__ yb = ybar_all ? ybar_all + (size_t)kg * p.vjp_n * y_step : nullptr;
    const double2 *__restrict__ ybd = ybd_all ? ybd_all + (size_t)kg * p.vjp_n * y_step : nullptr;
    const double *__restrict__ xd = xdot + (size_t)lo * K;         // (never read by a lane without a slice)
    double *__restrict__ row = p.vjp_rows + (size_t)k * K * Nsl;

    CMat<N> Q;
    {
        // ------------------------------------------------------------ 1: chunk product and chunk tangent
        CRect<N, N> R, Rd;
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            R.re[e] = ((e % N) == (e / N)) ? 1.0 : 0.0;
            R.im[e] = 0.0;
        }
        rzero(Rd);
#pragma unroll 1
        for (int jj = 0; jj < cnt; ++jj)
            hvp_step(R, Rd, ln.P(jj), stride, xd + (size_t)jj * K, opB, K);
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            Q.re[e] = R.re[e];
            Q.im[e] = R.im[e];
        }
        // ------------------------------------------------------------ 2: X at the chunk start, d_c
        CRect<N, M> X, dvec, D;
        {
            CMat<N> U;
            traj_prefix_start(U, Q, ln, s_q);
            traj_start_state(X, U, op.opXi);
#pragma unroll
            for (int e = 0; e < NN; ++e) {
                U.re[e] = Rd.re[e];
                U.im[e] = Rd.im[e];
            }
            rmul(dvec, U, X);
        }
        // ------------------------------------------------------------ 3: exclusive prefix scan of (Q, d): Xd at the chunk start
        {
            const int lane = ln.lane, wave = ln.wave, W = ln.W;
            CMat<N> G = Q, Go, T;
            CRect<N, M> vo, Tm;
            for (int s = 1; s < 64; s <<= 1) {       // (L-2s, L-s] then (L-s, L]:  (G Go) z + (G vo + v)
                rshfl_up(vo, dvec, s);
                if (lane >= s)
                    rmul_acc(dvec, G, vo);
                shfl_up(Go, G, s);
                if (lane >= s) {
                    mul(T, G, Go);
                    G = T;
                }
            }
            shfl_up(Go, G, 1);                       // the lanes in front of this one, inside the wave
            if (lane == 0)
                set_identity(Go);
            rshfl_up(vo, dvec, 1);
            if (lane == 0)
                rzero(vo);
            if (W > 1) {
                __syncthreads();                     // (the readers of the prefix totals in s_q are done)
                if (lane == 63) {
#pragma unroll
                    for (int e = 0; e < NN; ++e)
                        s_q[wave][e] = make_double2(G.re[e], G.im[e]);
#pragma unroll
                    for (int e = 0; e < NM; ++e)
                        s_v[wave][e] = make_double2(dvec.re[e], dvec.im[e]);
                }
                __syncthreads();
                CRect<N, M> z;
                rzero(z);
                for (int w = 0; w < wave; ++w) {     // what enters this wave on the left, first wave first
                    rc_load_lds(G, &s_q[w][0]);
                    rmul(Tm, G, z);
#pragma unroll
                    for (int e = 0; e < NM; ++e) {
                        const double2 vv = s_v[w][e];
                        z.re[e] = Tm.re[e] + vv.x;
                        z.im[e] = Tm.im[e] + vv.y;
                    }
                }
                rmul(Tm, Go, z);
#pragma unroll
                for (int e = 0; e < NM; ++e) {
                    D.re[e] = Tm.re[e] + vo.re[e];
                    D.im[e] = Tm.im[e] + vo.im[e];
                }
            } else {
                D = vo;
            }
        }
        // ------------------------------------------------------------ 4: the chunk's states and tangents
#pragma unroll 1
        for (int jj = 0; jj < cnt; ++jj) {
            hvp_step(X, D, ln.P(jj), stride, xd + (size_t)jj * K, opB, K);
            if (!UNI) {
                double2 *__restrict__ sl = Xw + (size_t)jj * 2 * NM * stride;
                rstore_ws(sl, stride, X);
                rstore_ws(sl + (size_t)NM * stride, stride, D);
            }
        }
        if (UNI && cnt > 0) {
            rstore_ws(Xw, stride, X);
            rstore_ws(Xw + (size_t)NM * stride, stride, D);
        }
    }

    // the cotangent sources of slice t's right end, s = t + 1: the caller's (ybar, Xbar) onto Lam
    auto source = [&](CRect<N, M> &Lam, const int t, const double2 *__restrict__ y, const double2 *__restrict__ xall) {
        if (xall && t + 1 == Nsl)
            hvp_add_block(Lam, xall + (size_t)kg * NM);
        if (y)
            for (int j = 0; j < n_obs; ++j)
                hvp_source(Lam, y[(size_t)(t + 1) + (size_t)j * y_step], pr.probe(j));
    };

    CRect<N, M> Lin;
    {
        // ------------------------------------------------------------ 5: b_c
        CRect<N, M> bvec;
        rzero(bvec);
#pragma unroll 1
        for (int jj = cnt - 1; jj >= 0; --jj) {
            CMat<N> P;
            source(bvec, lo + jj, yb, xbar_all);
            rc_load_mat(P, ln.P(jj), stride);
            hvp_mul_ah_inplace(bvec, P);
        }
        // ------------------------------------------------------------ 6: Lam that enters the chunk on the right
        traj_affine_suffix(Lin, Q, bvec, ln, s_q, s_v);
    }
    CRect<N, M> Ldin;
    {
        // ------------------------------------------------------------ 7: bt_c
        CRect<N, M> Lam = Lin, bt;
        rzero(bt);
        if (UNI && cnt > 0)                          // (not live across the second scan: a third block of the lane's slot)
            rstore_ws(Xw + (size_t)2 * NM * stride, stride, Lin);
#pragma unroll 1
        for (int jj = cnt - 1; jj >= 0; --jj) {
            CMat<N> P;
            source(Lam, lo + jj, yb, xbar_all);
            source(bt, lo + jj, ybd, xbd_all);
            hvp_direction(P, xd + (size_t)jj * K, opB, K);
            hvp_mul_ah_acc(bt, P, Lam);              // Lamd + V' Lam
            rc_load_mat(P, ln.P(jj), stride);
            hvp_mul_ah_inplace(bt, P);
            hvp_mul_ah_inplace(Lam, P);
        }
        // ------------------------------------------------------------ 8: Lamd that enters the chunk on the right
        traj_affine_suffix(Ldin, Q, bt, ln, s_q, s_v);
    }
    // ---------------------------------------------------------------- 9: the true pair, the traces
    CRect<N, M> X, D;
    rzero(X);
    rzero(D);
    if (UNI)
        rzero(Lin);                                  // (a lane without a slice walks nothing)
    if (UNI && cnt > 0) {
        rload_ws(Lin, Xw + (size_t)2 * NM * stride, stride);
        rload_ws(X, Xw, stride);
        rload_ws(D, Xw + (size_t)NM * stride, stride);
    }
#pragma unroll 1
    for (int jj = cnt - 1; jj >= 0; --jj) {
        const int t = lo + jj;                       // slice index; the state behind it is X_{t+1}, cotangent row s = t + 1
        CMat<N> P;
        source(Lin, t, yb, xbar_all);
        source(Ldin, t, ybd, xbd_all);
        if (!UNI) {
            const double2 *__restrict__ sl = Xw + (size_t)jj * 2 * NM * stride;
            rload_ws(X, sl, stride);
            rload_ws(D, sl + (size_t)NM * stride, stride);
        }
        rmul_a_bh(P, X, Ldin);                       // X Lamd' + Xd Lam'
        hvp_mul_a_bh_acc(P, D, Lin);
        for (int c = 0; c < K; ++c) {
            double re = 0.0;
#pragma unroll
            for (int b2 = 0; b2 < N; ++b2)
#pragma unroll
                for (int a2 = 0; a2 < N; ++a2) {
                    const double2 b = opB[c * NN + a2 + b2 * N];
                    re = fma(b.x, P.re[b2 + a2 * N], re);
                    re = fma(-b.y, P.im[b2 + a2 * N], re);
                }
            row[(size_t)t * K + c] = re;
        }
        hvp_direction(P, xd + (size_t)jj * K, opB, K);
        hvp_mul_ah_acc(Ldin, P, Lin);                // Lamd + V' Lam
        if (UNI)
            hvp_mul_sub(D, P, X);                    // Xd_{t+1} - V X_{t+1}
        rc_load_mat(P, ln.P(jj), stride);
        hvp_mul_ah_inplace(Ldin, P);
        hvp_mul_ah_inplace(Lin, P);
        if (UNI) {
            hvp_mul_ah_inplace(D, P);
            hvp_mul_ah_inplace(X, P);
        }
    }
}

template <int N, int M>
static hipError_t hvp_launch_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = RcTraits<N>::MAXT;
    const int threads = (p.vjp_CH + 63) & ~63;
    const bool any_y = p.vjp_ybar || p.hvp_ybar_dot;
    if (threads > MAXT || p.vjp_CH < 1 || (long long)p.S * p.vjp_CH < p.N || p.N < 1 || p.E < 1 || p.K < 1 || p.vjp_E0 < 0 ||
        p.vjp_E0 + p.E > p.vjp_Etot || p.vjp_n < 0 || p.vjp_n > 16 || (!p.vjp_ybar && !p.vjp_xbar) ||
        (any_y && (p.vjp_n < 1 || !p.vjp_O)) || !p.vjp_rows || !p.vjp_part || !p.hvp_xs || !p.hvp_xdot || !p.props || !p.ops ||
        (long long)p.K * p.N > 0x7fffff00ll)
        return hipErrorInvalidConfiguration;
    const dim3 grid(p.E), block(threads);
    // (n = m = 3: the walk-back instance needs 28 bytes of scratch per lane at 256 registers; the storing one holds its state
    // and is right for unitary propagators too, so that shape always stores -- hvp_walks_back, grape_kernels.hpp)
    constexpr bool WB = hvp_walks_back(N, M);
    if (p.vjp_unitary && WB)
        GRAPE_LAUNCH_AS("trajectory_hvp_kernel", (trajectory_hvp_kernel<N, M, WB, MAXT>), grid, block, 0, stream, p.ops, p.vjp_O,
                        p.vjp_ybar, p.vjp_xbar, p.hvp_ybar_dot, p.hvp_xbar_dot, p.hvp_xdot, p);
    else
        GRAPE_LAUNCH_AS("trajectory_hvp_kernel", (trajectory_hvp_kernel<N, M, false, MAXT>), grid, block, 0, stream, p.ops, p.vjp_O,
                        p.vjp_ybar, p.vjp_xbar, p.hvp_ybar_dot, p.hvp_xbar_dot, p.hvp_xdot, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    return launch_vjp_rows_sum(p, stream);
}

hipError_t run_trajectory_hvp(int n, const SweepParams &p, hipStream_t stream)
{
    return dispatch_nm(n, p.vjp_m, [&](auto N, auto M) {
        return hvp_launch_nm<decltype(N)::value, decltype(M)::value>(p, stream);
    });
}

}  // namespace grape
