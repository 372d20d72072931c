// basis.hip -- grape_set_basis: the two kernels around an evaluation in parameter mode.
//
//   x[c,t]        = x0[c,t] + sum_{m<M} theta[c,m] phi_b[t,m]          (basis_expand_kernel, in front of the sweeps)
//   G_theta[c,m]  = sum_t G_tot[c,t] phi_b[t,m]                         (basis_project_kernel, behind the final sum)
//
// b = 0 for a shared basis, c for one basis per control.  Both sums have a fixed order (m ascending; t in a lane stride of
// 64, ascending, then a 64-lane xor butterfly), so a parameter-mode evaluation is bitwise reproducible call to call.  The
// expansion writes the (K, N[, n_x]) control array the sweep kernels and the penalty terms already read; the projection
// reads the complete summed rows { G_tot, F } -- behind the cross-device sum / exchange, penalties included -- and is the
// evaluation's LAST kernel: it publishes to the host as copy_kernel does (done_signal.hpp).
// Both are reached through launch_copy (DoneSignal::basis), so the host layer links against the same launcher set as before.
//
// grape_set_bounds (BasisOp::bounded) sits at the same seam: a pointwise smooth saturation behind the expansion and its slope
// in front of the projection,
//   x[c,t]   = mid_c + half_c tanh((a[c,t] - mid_c) / half_c),   s[c,t] = 1 - tanh^2(...),   G_a[c,t] = G_tot[c,t] s[c,t]
// with a = x0 + theta phi^T (fused into the two kernels above: no second pass over x, the projection keeps its order), or
// a = the entry point's argument when no basis is in force (M = 0: bounds_saturate_kernel / bounds_slope_kernel).  With
// bounded == 0 the two basis kernels do exactly the arithmetic they always did.
//
// grape_eval_jvp (BasisOp::tangent) pushes a DIRECTION through the same seam: xdot[c,t] = s[c,t] sum_m thetadot[c,m] phi_b[t,m],
// the expansion without x0 and without the saturation, times the slope array the evaluation's own expansion has just written
// (read here, not written; 1 without bounds; M = 0: bounds_tangent_kernel) -- the transpose of the projection.
#include "done_signal.hpp"

namespace grape {

// the saturation of one entry and its derivative.  A control without bounds (lo = -inf, hi = +inf; the host layer admits
// nothing one-sided) is the identity.  tanh rounds to +-1 from |argument| ~ 19 on: the result is then held at the last
// double inside the open interval, so the physical pulse never touches a bound, and the slope is 0.
__device__ __forceinline__ double saturate(double a, double lo, double hi, double &s)
{
    if (!(lo > -INFINITY)) {
        s = 1.0;
        return a;
    }
    const double mid = 0.5 * lo + 0.5 * hi, half = 0.5 * hi - 0.5 * lo;
    const double th = tanh((a - mid) / half);
    s = fma(-th, th, 1.0);
    double x = fma(half, th, mid);
    if (x >= hi) x = nextafter(hi, lo);
    if (x <= lo) x = nextafter(lo, hi);
    return x;
}

// one thread per entry of x: an M-term FMA chain, m ascending.  A workgroup owns 256 slices of ONE control (blockIdx.y) of
// one array (blockIdx.z) and passes that control's coefficients through LDS in tiles of 256: theta may live in mapped host
// memory (the blocking entry points stage it there -- the expansion IS the upload), where every read is a trip over the
// bus; this way each coefficient is fetched once per workgroup instead of once per slice.  phi is read coalesced in t.
constexpr int kBasisTile = 256;
__global__ __launch_bounds__(256) void basis_expand_kernel(const BasisOp op, const double *__restrict__ theta,
                                                           double *__restrict__ x)
{
    __shared__ double s_th[kBasisTile];
    const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    const bool live = t < op.N;
    const double *ph = op.phi + (size_t)(op.n_bases == 1 ? 0 : c) * op.N * op.M + (live ? t : 0);
    const double *th = theta + (size_t)b * op.K * op.M + c;
    double acc = live && op.x0 && !op.tangent ? op.x0[c + (size_t)op.K * t] : 0.0;
    for (int m0 = 0; m0 < op.M; m0 += kBasisTile) {
        const int cnt = op.M - m0 < kBasisTile ? op.M - m0 : kBasisTile;
        __syncthreads();
        if ((int)threadIdx.x < cnt)
            s_th[threadIdx.x] = th[(size_t)op.K * (m0 + threadIdx.x)];
        __syncthreads();
        if (live)
            for (int j = 0; j < cnt; ++j)
                acc = fma(s_th[j], ph[(size_t)op.N * (m0 + j)], acc);
    }
    if (live) {
        const size_t i = (size_t)b * op.K * op.N + c + (size_t)op.K * t;
        if (op.tangent) {                                    // grape_eval_jvp: the direction, times the slope in place
            if (op.bounded)
                acc *= op.slope[i];
        } else if (op.bounded) {
            double s;
            acc = saturate(acc, op.lo[c], op.hi[c], s);
            op.slope[i] = s;
        }
        x[i] = acc;
    }
}

// one wave per output (c, m) of control array blockIdx.y; four waves per workgroup.  Lane l sums t = l, l + 64, ...
// ascending, the 64 partial sums meet in an xor butterfly (every lane ends with the same bits).  The wave of output 0 also
// carries F through.
__global__ __launch_bounds__(256) void basis_project_kernel(const BasisOp op, const double *__restrict__ rows,
                                                            double *__restrict__ out, DoneSignal done)
{
    const int KM = op.K * op.M, Qn = op.K * op.N + 1, Qm = KM + 1;
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);       // c + K m
    const int b = blockIdx.y;
    if (o < KM) {
        const int c = o % op.K, m = o / op.K;
        const double *g = rows + (size_t)b * Qn + c;
        const double *ph = op.phi + ((size_t)(op.n_bases == 1 ? 0 : c) * op.M + m) * op.N;
        double part = 0.0;
        if (op.bounded) {                                    // (same order: the slope scales the entry, nothing else moves)
            const double *s = op.slope + (size_t)b * op.K * op.N + c;
            for (int t = lane; t < op.N; t += 64)
                part = fma(g[(size_t)op.K * t] * s[(size_t)op.K * t], ph[t], part);
        } else
            for (int t = lane; t < op.N; t += 64)
                part = fma(g[(size_t)op.K * t], ph[t], part);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            part += __shfl_xor(part, d, 64);
        if (lane == 0) {
            out[(size_t)b * Qm + o] = part;
            if (o == 0 && !op.no_f)
                out[(size_t)b * Qm + KM] = rows[(size_t)b * Qn + Qn - 1];
        }
    }
    if (done.flag) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0)
            signal_done(done, gridDim.x * gridDim.y);
    }
}

// grape_set_bounds without a basis, in front of the evaluation: one thread per entry of (K, N, n_x).  u may live in mapped
// host memory (the saturation is the upload, as the expansion is); x and the slope are written coalesced.
__global__ __launch_bounds__(256) void bounds_saturate_kernel(const BasisOp op, const double *__restrict__ u,
                                                              double *__restrict__ x)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, KN = (size_t)op.K * op.N;
    if (i >= KN * op.n_x)
        return;
    const int c = (int)((i % KN) % op.K);
    double s;
    x[i] = saturate(u[i], op.lo[c], op.hi[c], s);
    op.slope[i] = s;
}

// grape_eval_jvp under bounds without a basis: the direction times the slope array of the evaluation (BasisOp::tangent)
__global__ __launch_bounds__(256) void bounds_tangent_kernel(const BasisOp op, const double *__restrict__ udot,
                                                             double *__restrict__ xdot)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)op.K * op.N)
        xdot[i] = udot[i] * op.slope[i];
}

// ... and behind it, the evaluation's LAST kernel in this mode: out = n_x blocks of { G_tot s, F } from the complete summed
// rows, published as basis_project_kernel publishes.
__global__ __launch_bounds__(256) void bounds_slope_kernel(const BasisOp op, const double *__restrict__ rows,
                                                           double *__restrict__ out, DoneSignal done)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, KN = (size_t)op.K * op.N, Q = KN + (op.no_f ? 0 : 1);
    if (i < Q * op.n_x) {
        const size_t b = i / Q, j = i % Q;
        out[i] = j < KN ? rows[i] * op.slope[b * KN + j] : rows[i];
    }
    if (done.flag) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0)
            signal_done(done, gridDim.x);
    }
}

hipError_t launch_basis(const BasisOp &op, const double *src, double *dst, hipStream_t stream, DoneSignal done)
{
    if (op.mean)                                             // the *_mean trajectory calls: traj_mean.hip stands in
        return run_traj_mean(*op.mean, stream);
    if (op.K < 1 || op.K > 65535 || op.N < 1 || op.M < 0 || op.M > op.N || op.n_x < 1 || op.n_x > 65535 || !src || !dst)
        return hipErrorInvalidValue;
    if (op.M > 0 ? !op.phi : !op.bounded)                    // (M = 0, the identity expansion, exists for the bounds alone)
        return hipErrorInvalidValue;
    if (op.bounded && (!op.lo || !op.hi || !op.slope))
        return hipErrorInvalidValue;
    if (op.no_f && (!op.project || op.n_x != 1))
        return hipErrorInvalidValue;
    if (op.tangent && (op.project || op.n_x != 1))
        return hipErrorInvalidValue;
    done.basis = nullptr;                                    // (a host address: nothing for the device)
    if (op.M == 0) {
        const size_t n = ((size_t)op.K * op.N + (op.project && !op.no_f ? 1 : 0)) * op.n_x;
        if (n > 0x7fffff00u)
            return hipErrorInvalidValue;
        if (op.tangent) {
            GRAPE_LAUNCH(bounds_tangent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, op, src, dst);
            return hipGetLastError();
        }
        if (!op.project) {
            GRAPE_LAUNCH(bounds_saturate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, op, src, dst);
            return hipGetLastError();
        }
        GRAPE_LAUNCH(bounds_slope_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, op, src, dst, done);
        return hipGetLastError();
    }
    if (!op.project) {
        GRAPE_LAUNCH(basis_expand_kernel, dim3((op.N + 255) / 256, op.K, op.n_x), dim3(256), 0, stream, op, src, dst);
        return hipGetLastError();
    }
    GRAPE_LAUNCH(basis_project_kernel, dim3((op.K * op.M + 3) / 4, op.n_x), dim3(256), 0, stream, op, src, dst, done);
    return hipGetLastError();
}

}  // namespace grape
