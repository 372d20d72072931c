// gnvp.hip -- the weighted Gauss-Newton product of the trajectory read-out (grape_eval_gnvp: J' W J v in ONE pass over the
// trajectory) for the small-n family (n = 2, 3, 4; n x m states under left multiplication, UnitaryGate) on gfx950.
//
//   the push-forward of grape_eval_jvp along a direction xdot of the PHYSICAL pulse (the host layer has applied the pulse
//   map's tangent), weighted entry by entry, into the pull-back of grape_eval_vjp, under the rule of the first-order pair,
//   Pdot_s = V_s P_s with V_s = sum_c xdot[c,s] B'_{k,c},  B' = -i dt B:
//   D_0     = 0 ,                              D_{s+1}   = P_s D_s + V_s X_{s+1}                         (grape_eval_jvp's tangent)
//   ydot    = tr(O_kj' D_{k,s}) ,              c[s,j,k]  = (w_rr Re ydot + w_ri Im ydot) + i (w_ri Re ydot + w_ii Im ydot)
//   Lam_N   = wf_k D_N + sum_j c[N,j,k] O_kj , Lam_s     = P_s' Lam_{s+1} + sum_j c[s,j,k] O_kj          (grape_eval_vjp's costate)
//   Gn[c,t] = sum_k Re tr(Lam_{k,t+1}' B'_{k,c} X_{k,t+1})
//
// It runs behind the sweep of the same launch and reads the propagators P_t that sweep left in the workspace (chunk-major).
// The decomposition and the steps marked * are traj_chunk.hpp's: one workgroup per member of the launch, one lane per time
// chunk of S consecutive slices, every workspace access lane-contiguous:
//   1  ONE forward walk over the chunk in relative form: the chunk product Q_c and the chunk tangent
//      R_c = sum_j P_hi-1 .. P_j+1 V_j P_j .. P_lo (the first pass of jvp.hip)
//   2* exclusive prefix of the Q_c: X at the chunk start; d_c = R_c X_lo
//   3  exclusive prefix scan of the affine maps z -> Q_c z + d_c (jvp.hip's, one direction): D at the chunk start
//   4  forward walk on (X, D) from the true start values.  Per slice: the n_obs traces, their weight blocks, and the SOURCE
//      of the costate recurrence at the slice's right end, Src_{t+1} = [t + 1 = N] wf_k D_N + sum_j c[t+1,j,k] O_kj, one n x m
//      block, into the scratch SweepParams::gnvp_src (chunk-major like props, n m elements per slice).  D is dead behind this
//      walk.  Unitary flow: X at the chunk END stays in registers and the last walk steps back with X_t = P_t' X_{t+1};
//      general flow: X_{t+1} of every slice goes into the scratch of the VJP's general flow (SweepParams::vjp_xs)
//   5  backward walk of Lam from 0 with the stored sources: b_c
//   6* suffix scan of z -> Q_c' z + b_c: Lam that enters the chunk on the right
//   7  the walk from the true costate: the K entries of the member's row per slice
// The stored block, not the n_obs coefficients: both backward walks then add one block per slice (no probe is read behind
// walk 4, where the coefficients would cost 4 n m FMAs per probe and slice in EACH walk), the final-state term rides in the
// same block, and the scratch does not depend on the probe count of a call.
// Every number has one fixed evaluation order; the members' rows are unweighted, written with plain vector stores, and summed
// by vjp_sum_kernel in the tree fixed by the members' ensemble indices: a member-chunked launch sequence gives the bits of an
// unchunked one.  Every operation that touches xdot is linear in it (products and FMAs whose addends all carry one factor of
// it): twice the direction gives twice the bits, the negated direction the negated bits; the same holds for the weights.
#include "cmat.hpp"
#include "grape_kernels.hpp"
#include "rc_mat.hpp"
#include "traj_chunk.hpp"

namespace grape {

// V = sum_c xd[c] B'_c  (opB: the member's K prescaled control operators, wave-uniform; xd: the slice's row of xdot)
template <int N>
GRAPE_DEV void gnvp_direction(CMat<N> &V, const double *__restrict__ xd, const double2 *__restrict__ opB, int K)
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
GRAPE_DEV void gnvp_step(CRect<N, C> &X, CRect<N, C> &D, const double2 *__restrict__ Pt, size_t stride, const double *__restrict__ xd,
                         const double2 *__restrict__ opB, int K)
{
    CMat<N> P;
    rc_load_mat(P, Pt, stride);
    rmul_inplace(X, P);
    rmul_inplace(D, P);
    gnvp_direction(P, xd, opB, K);
    rmul_acc(D, P, X);
}

// Lam += the stored source block of one slice
template <int N, int M>
GRAPE_DEV void gnvp_add_ws(CRect<N, M> &Lam, const double2 *__restrict__ base, size_t stride)
{
    CRect<N, M> S;
    rload_ws(S, base, stride);
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        Lam.re[e] += S.re[e];
        Lam.im[e] += S.im[e];
    }
}

// ops_all / o_all / wy_all / wf_all are separate `const __restrict__` arguments so that the wave-uniform operator and probe
// entries can be fetched with scalar loads (as in vjp.hip).  UNI: every propagator is unitary.
template <int N, int M, bool UNI, int MAXT>
__global__ __launch_bounds__(MAXT) void trajectory_gnvp_kernel(const double2 *__restrict__ ops_all,
                                                               const double2 *__restrict__ o_all,
                                                               const double *__restrict__ wy_all,
                                                               const double *__restrict__ wf_all,
                                                               const double *__restrict__ xdot, const SweepParams p)
{
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    __shared__ double2 s_q[MAXW][NN];              // wave totals: prefix products, then the affine maps' matrices ...
    __shared__ double2 s_v[MAXW][NM];              // ... and their offsets

    const int K = p.K, Nsl = p.N, n_obs = wy_all ? p.vjp_n : 0;
    const int k = blockIdx.x;                        // member within the launch: row of the workspace and of the rows
    const int kg = k + p.vjp_E0;                     // member of the ensemble: row of the probes and of the weights
    const TrajLane<N> ln = traj_lane<N>(p.vjp_CH, p.S, Nsl, p.props, k);
    const int lo = ln.lo, cnt = ln.cnt;
    const size_t stride = ln.stride;
    double2 *__restrict__ Sw = ln.template ws<NM>(p.gnvp_src);     // slot jj: the source at the right end of slice lo + jj
    double2 *__restrict__ Xw = UNI ? nullptr : ln.template ws<NM>(p.vjp_xs);
    const TrajOps op = traj_ops<N>(ops_all, k, K);
    const double2 *__restrict__ opB = op.opB;
    const TrajProbes pr = traj_probes<N, M>(o_all, p.vjp_per_member, p.vjp_Etot, kg, Nsl);
    const size_t y_step = pr.y_step;
    // the weights: (N + 1, n_obs, 3) shared or (N + 1, n_obs, Etot, 3) per member, planes rr, ri, ii slowest
    const double *__restrict__ wy = wy_all ? wy_all + (p.gnvp_w_per_member ? (size_t)kg * p.vjp_n * y_step : (size_t)0) : nullptr;
    const size_t w_plane = (size_t)p.vjp_n * y_step * (p.gnvp_w_per_member ? (size_t)p.vjp_Etot : (size_t)1);
    const double *__restrict__ xd = xdot + (size_t)lo * K;         // (never read by a lane without a slice)
    double *__restrict__ row = p.vjp_rows + (size_t)k * K * Nsl;

    CMat<N> Q;
    CRect<N, M> Xhi;
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
            gnvp_step(R, Rd, ln.P(jj), stride, xd + (size_t)jj * K, opB, K);
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
        // ------------------------------------------------------------ 3: exclusive prefix scan of (Q, d): D at the chunk start
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
        // ------------------------------------------------------------ 4: the chunk's states, tangents and sources
#pragma unroll 1
        for (int jj = 0; jj < cnt; ++jj) {
            const int s = lo + jj + 1;               // the right end of slice lo + jj: row s of y and of the weights
            gnvp_step(X, D, ln.P(jj), stride, xd + (size_t)jj * K, opB, K);
            CRect<N, M> Src;
            rzero(Src);
            if (wf_all && s == Nsl) {                // Lam_N starts from wf_k D_N
                const double wf = wf_all[kg];
#pragma unroll
                for (int e = 0; e < NM; ++e) {
                    Src.re[e] = wf * D.re[e];
                    Src.im[e] = wf * D.im[e];
                }
            }
            for (int j = 0; j < n_obs; ++j) {
                const double2 *__restrict__ o = pr.probe(j);
                const double2 yd = traj_probe_trace<N, M>(o, D);
                const double *__restrict__ w = wy + (size_t)s + (size_t)j * y_step;
                const double wrr = w[0], wri = w[w_plane], wii = w[2 * w_plane];
                const double cr = fma(wri, yd.y, wrr * yd.x), ci = fma(wii, yd.y, wri * yd.x);
#pragma unroll
                for (int e = 0; e < NM; ++e) {       // Src += c O_j  (the VJP kernel's source term)
                    const double2 v = o[e];
                    Src.re[e] = fma(cr, v.x, fma(-ci, v.y, Src.re[e]));
                    Src.im[e] = fma(cr, v.y, fma(ci, v.x, Src.im[e]));
                }
            }
            rstore_ws(Sw + (size_t)jj * NM * stride, stride, Src);
            if (!UNI)
                rstore_ws(Xw + (size_t)jj * NM * stride, stride, X);
        }
        Xhi = X;                                     // (unitary flow: X at the chunk end, for walk 7)
    }

    CRect<N, M> Lam;
    {
        // ------------------------------------------------------------ 5: b_c
        CRect<N, M> bvec, Tm;
        rzero(bvec);
#pragma unroll 1
        for (int jj = cnt - 1; jj >= 0; --jj) {
            CMat<N> P;
            gnvp_add_ws(bvec, Sw + (size_t)jj * NM * stride, stride);
            rc_load_mat(P, ln.P(jj), stride);
            rmul_ah(Tm, P, bvec);
            bvec = Tm;
        }
        // ------------------------------------------------------------ 6: Lam that enters the chunk on the right
        traj_affine_suffix(Lam, Q, bvec, ln, s_q, s_v);
    }
    // ---------------------------------------------------------------- 7: the true costate, the traces
#pragma unroll 1
    for (int jj = cnt - 1; jj >= 0; --jj) {
        const int t = lo + jj;                       // slice index; the state behind it is X_{t+1}, source row s = t + 1
        CMat<N> P;
        CRect<N, M> Tm;
        gnvp_add_ws(Lam, Sw + (size_t)jj * NM * stride, stride);
        if (!UNI)
            rload_ws(Xhi, Xw + (size_t)jj * NM * stride, stride);
        rmul_a_bh(P, Xhi, Lam);                      // X Lam'
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
        rc_load_mat(P, ln.P(jj), stride);
        if (UNI) {
            rmul_ah(Tm, P, Xhi);                     // X_t = P_t' X_{t+1}
            Xhi = Tm;
        }
        rmul_ah(Tm, P, Lam);                         // pull the costate back over slice t
        Lam = Tm;
    }
}

template <int N, int M>
static hipError_t gnvp_launch_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = RcTraits<N>::MAXT;
    const int threads = (p.vjp_CH + 63) & ~63;
    if (threads > MAXT || p.vjp_CH < 1 || (long long)p.S * p.vjp_CH < p.N || p.N < 1 || p.E < 1 || p.K < 1 || p.vjp_E0 < 0 ||
        p.vjp_E0 + p.E > p.vjp_Etot || p.vjp_n < 0 || p.vjp_n > 16 || (!p.gnvp_wy && !p.gnvp_wf) ||
        (p.gnvp_wy && (p.vjp_n < 1 || !p.vjp_O)) || !p.vjp_rows || !p.vjp_part || !p.gnvp_src || !p.hvp_xdot || !p.props || !p.ops ||
        (!p.vjp_unitary && !p.vjp_xs) || (long long)p.K * p.N > 0x7fffff00ll)
        return hipErrorInvalidConfiguration;
    const dim3 grid(p.E), block(threads);
    if (p.vjp_unitary)
        GRAPE_LAUNCH_AS("trajectory_gnvp_kernel", (trajectory_gnvp_kernel<N, M, true, MAXT>), grid, block, 0, stream, p.ops, p.vjp_O,
                        p.gnvp_wy, p.gnvp_wf, p.hvp_xdot, p);
    else
        GRAPE_LAUNCH_AS("trajectory_gnvp_kernel", (trajectory_gnvp_kernel<N, M, false, MAXT>), grid, block, 0, stream, p.ops, p.vjp_O,
                        p.gnvp_wy, p.gnvp_wf, p.hvp_xdot, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    return launch_vjp_rows_sum(p, stream);
}

hipError_t run_trajectory_gnvp(int n, const SweepParams &p, hipStream_t stream)
{
    return dispatch_nm(n, p.vjp_m, [&](auto N, auto M) {
        return gnvp_launch_nm<decltype(N)::value, decltype(M)::value>(p, stream);
    });
}

}  // namespace grape
