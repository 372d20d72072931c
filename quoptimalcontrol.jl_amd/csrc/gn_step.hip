// gn_step.hip -- the kernels of grape_gn_step: one Levenberg-Marquardt step of the least-squares trajectory loss
//   L = 1/2 sum r' W r + 1/2 sum_k wf_k |X_{k,N} - T_k|^2 ,  r = y - y_target  (gauss_newton.py's module text)
// solved on the device, for the small-n family (n = 2, 3, 4; n x m states under left multiplication) on gfx950.
//
//   gn_residual_kernel    the read-out of observe.hip with the residual and the weights formed where observe_kernel stores
//                         tr(O' X_s): c = (w_rr Re r + w_ri Im r) + i (w_ri Re r + w_ii Im r) into y's layout (the pull-back's
//                         ybar), wf (X_N - T) into X_final's layout (its Xbar), and the member's share of L.  y never exists.
//   gn_cg_init_kernel     L from the members' shares; r = d = -g, p = Ap = 0, r.r, the stop threshold, the cases that end
//                         the solve before its first product (g = 0, NaN, no iteration allowed)
//   gn_cg_step_kernel     one iteration of gauss_newton._cg behind the product H d that trajectory_gnvp_kernel + vjp_sum_kernel
//                         left in Hd, with apply(d) = H d + lambda d.  Once GnRecord::done is set it changes nothing: the host
//                         enqueues iterations in blocks and reads the record between them
//   gn_cg_finish_kernel   |r|, |p| and the model decrease -g'p - p'Hp / 2 (H p = Ap - lambda p) from the vectors as they stand
//
// The residual kernel's decomposition is traj_chunk.hpp's (one workgroup per member, one lane per time chunk, lane-contiguous
// workspace accesses); its walk is observe_kernel's, operation for operation, so with unit weights the cotangents carry the
// bits of observe() - y_target.  A lane adds its terms of L in ascending s, probe by probe; the lanes' sums go through a fixed
// tree (xor butterfly inside a wave, the waves' totals in wave order).  The CG kernels run ONE workgroup: every dot product is
// a strided per-thread sum in ascending order and the same tree, so every number is bitwise reproducible for any Q = K cols,
// and the members' shares of L are added in segments of kMeanSeg consecutive members like traj_mean.hip's sums.  No atomics.
// Reached through launch_sweep_small / launch_sweep_pair (SweepParams::gn) only.
#include "cmat.hpp"
#include "grape_kernels.hpp"
#include "rc_mat.hpp"
#include "traj_chunk.hpp"

namespace grape {

constexpr int kGnThreads = 1024;               // the CG kernels' one workgroup

// sum (MAX: maximum) of v over the workgroup, the same bits in every thread.  s_w: one slot per wave; opens with the barrier
// that ends the previous call's reads
template <bool MAX>
GRAPE_DEV double gn_block_reduce(double v, double *s_w)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {              // (a + b and b + a are the same bits: every lane ends with the wave's total)
        const double o = __shfl_xor(v, d);
        v = MAX ? fmax(v, o) : v + o;
    }
    const int W = blockDim.x >> 6;
    if (W == 1)
        return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
        s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = s_w[0];
    for (int w = 1; w < W; ++w)
        t = MAX ? fmax(t, s_w[w]) : t + s_w[w];
    return t;
}

// ops_all / o_all / wy_all / wf_all are separate `const __restrict__` arguments so that the wave-uniform operator, probe and
// weight entries can be fetched with scalar loads (as in observe.hip and gnvp.hip)
template <int N, int M, int MAXT>
__global__ __launch_bounds__(MAXT) void gn_residual_kernel(const double2 *__restrict__ ops_all, const double2 *__restrict__ o_all,
                                                           const double *__restrict__ wy_all, const double *__restrict__ wf_all,
                                                           const double2 *__restrict__ yt_all, const double2 *__restrict__ xt_all,
                                                           double2 *__restrict__ ybar, double2 *__restrict__ xbar,
                                                           double *__restrict__ member_loss, const SweepParams p)
{
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    __shared__ double2 s_q[MAXW][NN];              // wave totals of the prefix scan
    __shared__ double s_w[MAXW];                   // ... and of the loss

    const int Nsl = p.N, n_obs = wy_all ? p.obs_n : 0;
    const int k = blockIdx.x;                        // member within the launch: row of the workspace
    const int kg = k + p.obs_E0;                     // member of the ensemble: row of the probes, the targets and the outputs
    const TrajLane<N> ln = traj_lane<N>(p.obs_CH, p.S, Nsl, p.props, k);
    const int L = ln.L, lo = ln.lo, hi = ln.hi, cnt = ln.cnt;
    const TrajProbes pr = traj_probes<N, M>(o_all, p.obs_per_member, p.obs_Etot, kg, Nsl);
    const size_t y_step = pr.y_step, y_mem = (size_t)kg * p.obs_n * y_step;
    // the weights: (N + 1, n_obs, 3) shared or (N + 1, n_obs, Etot, 3) per member, planes rr, ri, ii slowest (gnvp.hip)
    const double *__restrict__ wy = wy_all ? wy_all + (p.gnvp_w_per_member ? y_mem : (size_t)0) : nullptr;
    const size_t w_plane = (size_t)p.obs_n * y_step * (p.gnvp_w_per_member ? (size_t)p.obs_Etot : (size_t)1);
    const double2 *__restrict__ yt = yt_all ? yt_all + y_mem : nullptr;
    double2 *__restrict__ yb = ybar ? ybar + y_mem : nullptr;

    // ---------------------------------------------------------------- chunk product, U at the chunk start (observe.hip 1, 2)
    CMat<N> P, U;
    {
        CMat<N> Q;
        traj_chunk_product(Q, ln);
        traj_prefix_start(U, Q, ln, s_q);
    }
    // ---------------------------------------------------------------- the state at the chunk start (3)
    CRect<N, M> X, Tm;
    rload_uniform(X, traj_ops<N>(ops_all, k, p.K).opXi);
    rmul(Tm, U, X);
    X = Tm;

    double loss = 0.0;                               // twice the lane's share of L
    // the n_obs residuals of the state behind s slices, one probe at a time: the cotangent and its term r' W r
    auto emit = [&](int s) {
        for (int j = 0; j < n_obs; ++j) {
            const double2 y = traj_probe_trace(pr.probe(j), X);
            const size_t at = (size_t)s + (size_t)j * y_step;
            const double2 t = yt[at];
            const double rr = y.x - t.x, ri = y.y - t.y;
            const double *__restrict__ w = wy + at;
            const double wrr = w[0], wri = w[w_plane], wii = w[2 * w_plane];
            const double cr = fma(wri, ri, wrr * rr), ci = fma(wii, ri, wri * rr);
            yb[at] = make_double2(cr, ci);
            loss = fma(rr, cr, loss);
            loss = fma(ri, ci, loss);
        }
    };
    if (n_obs > 0 && L == 0)
        emit(0);                                     // (U_start = 1: X is Xi)
    // ---------------------------------------------------------------- the walk (4)
    for (int jj = 0; jj < cnt; ++jj) {
        rc_load_mat(P, ln.P(jj), ln.stride);
        rmul(Tm, P, X);
        X = Tm;
        if (n_obs > 0)
            emit(lo + jj + 1);
    }
    // ---------------------------------------------------------------- X_N: wf (X_N - T) and its term (5)
    if (wf_all && cnt > 0 && hi == Nsl) {
        const double wf = wf_all[kg];
        const double2 *__restrict__ xt = xt_all + (size_t)kg * NM;
        double2 *__restrict__ xb = xbar + (size_t)kg * NM;
#pragma unroll
        for (int e = 0; e < NM; ++e) {
            const double2 t = xt[e];
            const double dr = X.re[e] - t.x, di = X.im[e] - t.y;
            const double cr = wf * dr, ci = wf * di;
            xb[e] = make_double2(cr, ci);
            loss = fma(dr, cr, loss);
            loss = fma(di, ci, loss);
        }
    }
    const double tot = gn_block_reduce<false>(loss, s_w);
    if (L == 0)
        member_loss[kg] = 0.5 * tot;
}

// the strided per-thread part of a dot product: entries threadIdx.x, threadIdx.x + blockDim.x, ... in ascending order
#define GN_FOR_OWN(i, Q) for (int i = (int)threadIdx.x; i < (Q); i += (int)blockDim.x)

__global__ __launch_bounds__(kGnThreads) void gn_cg_init_kernel(const GnOp op)
{
    __shared__ double s_w[kGnThreads / 64];
    const int Q = op.Q;
    // L: the members' shares, a segment of kMeanSeg consecutive members at a time, in member order
    double l = 0.0;
    const int nseg = (op.E + kMeanSeg - 1) / kMeanSeg;
    GN_FOR_OWN(sg, nseg) {
        const int k0 = sg * kMeanSeg, k1 = min(k0 + kMeanSeg, op.E);
        double a = op.member_loss[k0];
        for (int k = k0 + 1; k < k1; ++k)
            a += op.member_loss[k];
        l += a;
    }
    const double loss = gn_block_reduce<false>(l, s_w);
    double rr = 0.0, gi = 0.0;
    GN_FOR_OWN(i, Q) {
        const double v = -op.g[i];
        op.r[i] = v;
        op.d[i] = v;
        op.p[i] = 0.0;
        op.Ap[i] = 0.0;
        rr = fma(v, v, rr);
        gi = fmax(gi, fabs(v));
    }
    rr = gn_block_reduce<false>(rr, s_w);
    gi = gn_block_reduce<true>(gi, s_w);
    if (threadIdx.x == 0) {
        GnRecord r;
        r.loss = loss;
        r.g_norm = sqrt(rr);
        r.g_inf = rr == rr ? gi : rr;                // (fmax drops a NaN: the norm keeps it)
        r.rr = rr;
        r.stop = op.rtol * op.rtol * rr;
        r.residual = r.g_norm;
        r.p_norm = 0.0;
        r.predicted = 0.0;
        r.iter = 0;
        r.pad = 0;
        // what ends the solve in front of its first product: g = 0; NaN; already below the threshold; no iteration allowed
        if (rr == 0.0) {
            r.status = 3;
            r.done = 1;
        } else if (!(rr == rr) || !(loss == loss)) {
            r.status = 2;
            r.done = 1;
        } else if (rr <= r.stop) {
            r.status = 0;
            r.done = 1;
        } else {
            r.status = 1;
            r.done = op.max_iter == 0 ? 1 : 0;
        }
        *op.rec = r;
    }
}

// gauss_newton._cg's loop body with Hd = H d (op.Hd) + lambda d:
//   curv = d.Hd; stop unless curv > 0; a = rr / curv; p += a d; Ap += a Hd; r -= a Hd; rr' = r.r; d = r + (rr' / rr) d
// The test rr <= stop that stands in front of the NEXT application is made here, behind the update: a launch behind it is a no-op.
__global__ __launch_bounds__(kGnThreads) void gn_cg_step_kernel(const GnOp op)
{
    __shared__ double s_w[kGnThreads / 64];
    const GnRecord rec = *op.rec;                    // (thread 0 writes it behind the last barrier of this kernel)
    if (rec.done)
        return;
    const int Q = op.Q;
    const double lam = op.lambda;
    double curv = 0.0;
    GN_FOR_OWN(i, Q) {
        const double di = op.d[i];
        const double ld = lam * di;
        const double hd = op.Hd[i] + ld;
        curv = fma(di, hd, curv);
    }
    curv = gn_block_reduce<false>(curv, s_w);
    if (!(curv > 0.0)) {                             // no positive curvature along d (or NaN): the state stays
        if (threadIdx.x == 0) {
            op.rec->status = 2;
            op.rec->done = 1;
        }
        return;
    }
    const double a = rec.rr / curv;
    double rr = 0.0;
    GN_FOR_OWN(i, Q) {
        const double di = op.d[i];
        const double ld = lam * di;
        const double hd = op.Hd[i] + ld;
        op.p[i] = fma(a, di, op.p[i]);
        op.Ap[i] = fma(a, hd, op.Ap[i]);
        const double ri = fma(-a, hd, op.r[i]);
        op.r[i] = ri;
        rr = fma(ri, ri, rr);
    }
    rr = gn_block_reduce<false>(rr, s_w);
    const double beta = rr / rec.rr;
    GN_FOR_OWN(i, Q)
        op.d[i] = fma(beta, op.d[i], op.r[i]);
    if (threadIdx.x == 0) {
        const int it = rec.iter + 1;
        op.rec->rr = rr;
        op.rec->iter = it;
        if (rr <= rec.stop) {
            op.rec->status = 0;
            op.rec->done = 1;
        } else if (!(rr == rr)) {
            op.rec->status = 2;
            op.rec->done = 1;
        } else if (it >= op.max_iter) {
            op.rec->status = 1;
            op.rec->done = 1;
        }
    }
}

__global__ __launch_bounds__(kGnThreads) void gn_cg_finish_kernel(const GnOp op)
{
    __shared__ double s_w[kGnThreads / 64];
    const int Q = op.Q;
    double pp = 0.0, gp = 0.0, pAp = 0.0;
    GN_FOR_OWN(i, Q) {
        const double pi = op.p[i];
        pp = fma(pi, pi, pp);
        gp = fma(op.g[i], pi, gp);
        pAp = fma(pi, op.Ap[i], pAp);
    }
    pp = gn_block_reduce<false>(pp, s_w);
    gp = gn_block_reduce<false>(gp, s_w);
    pAp = gn_block_reduce<false>(pAp, s_w);
    if (threadIdx.x == 0) {
        op.rec->residual = sqrt(op.rec->rr);
        op.rec->p_norm = sqrt(pp);
        op.rec->predicted = -gp - 0.5 * (pAp - op.lambda * pp);
    }
}
#undef GN_FOR_OWN

template <int N, int M>
static hipError_t gn_residual_launch_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = RcTraits<N>::MAXT;
    const GnOp &op = *p.gn;
    const int threads = (p.obs_CH + 63) & ~63;
    const bool has_y = p.gnvp_wy != nullptr, has_x = p.gnvp_wf != nullptr;
    if (threads > MAXT || p.obs_CH < 1 || (long long)p.S * p.obs_CH < p.N || p.N < 1 || p.E < 1 || p.obs_E0 < 0 ||
        p.obs_E0 + p.E > p.obs_Etot || p.obs_n < 0 || p.obs_n > 16 || (!has_y && !has_x) ||
        (has_y && (p.obs_n < 1 || !p.obs_O || !op.y_target || !op.ybar)) || (has_x && (!op.xf_target || !op.xbar)) ||
        !op.member_loss || !p.props || !p.ops)
        return hipErrorInvalidConfiguration;
    GRAPE_LAUNCH_AS("gn_residual_kernel", (gn_residual_kernel<N, M, MAXT>), dim3(p.E), dim3(threads), 0, stream, p.ops, p.obs_O,
                    p.gnvp_wy, p.gnvp_wf, op.y_target, op.xf_target, op.ybar, op.xbar, op.member_loss, p);
    return hipGetLastError();
}

hipError_t run_gn_step(int n, const SweepParams &p, hipStream_t stream)
{
    if (!p.gn)
        return hipErrorInvalidValue;
    const GnOp &op = *p.gn;
    if (op.kind == 1)
        return dispatch_nm(n, p.obs_m, [&](auto N, auto M) {
            return gn_residual_launch_nm<decltype(N)::value, decltype(M)::value>(p, stream);
        });
    if (op.Q < 1 || !op.g || !op.p || !op.Ap || !op.r || !op.d || !op.rec)
        return hipErrorInvalidValue;
    switch (op.kind) {
    case 2:
        if (op.E < 1 || !op.member_loss || op.max_iter < 0)
            return hipErrorInvalidValue;
        GRAPE_LAUNCH(gn_cg_init_kernel, dim3(1), dim3(kGnThreads), 0, stream, op);
        break;
    case 3:
        if (!op.Hd)
            return hipErrorInvalidValue;
        GRAPE_LAUNCH(gn_cg_step_kernel, dim3(1), dim3(kGnThreads), 0, stream, op);
        break;
    case 4:
        GRAPE_LAUNCH(gn_cg_finish_kernel, dim3(1), dim3(kGnThreads), 0, stream, op);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace grape
