// traj_mean.hip -- the ensemble-averaged trajectory calls (grape_eval_observables_mean / _vjp_mean / _jvp_mean): the two
// kernels that stand between the member axis of the trajectory kernels' arrays and the caller.
//
//   reduction   out[i] = sum_k v_k a[i + L k]      behind the last member block of a read-out / push-forward: the
//                                                  (N + 1, n_obs, E) array that observe_kernel / trajectory_jvp_kernel wrote,
//                                                  and the (n, m, E) final states, summed over their slowest axis
//   broadcast   a[i + L k] = (v_k Re s_i, v_k Im s_i)   in front of a pull-back: the caller's ONE cotangent block, spread over
//                                                  the members' places in the buffers trajectory_vjp_kernel reads -- one rounded
//                                                  product per component, exactly what the caller would have uploaded
//
// The summation tree is a function of E alone: the member axis is cut into segments of kMeanSeg consecutive members, a segment
// is summed in member order (the first term a product, every further one an FMA), and -- more than one segment --
// traj_mean_combine_kernel adds the segments' sums in segment order.  Neither N, n_obs, the probe index, the context's member
// chunk nor the sweep's workgroup layout enters, so the result is bitwise reproducible, chunked = unchunked, and column j of
// a 16-probe call is the 1-probe call with probe j.  No atomics.  One lane per complex entry, consecutive lanes on
// consecutive entries (16-byte loads and stores); the segments give a 1-probe call (N + 1 entries) E / kMeanSeg times as
// many waves as entries alone would.
//
// Both arrays of a call (the y type and the final-state type) ride in one launch: the blocks [0, nb0) of the grid's x axis
// belong to array 0, the rest to array 1.  Reached through launch_copy (DoneSignal::basis -> BasisOp::mean) only.
#include "grape_kernels.hpp"

namespace grape {

constexpr int kMeanThreads = 128;

struct MeanWhere {
    int a;              // which array
    long long i;        // entry inside it; < 0: none
};
__device__ __forceinline__ MeanWhere mean_where(const MeanOp &op, int nb0)
{
    MeanWhere w;
    w.a = (int)blockIdx.x >= nb0 ? 1 : 0;
    w.i = (long long)((int)blockIdx.x - (w.a ? nb0 : 0)) * kMeanThreads + threadIdx.x;
    if (w.i >= op.L[w.a])
        w.i = -1;
    return w;
}

// segment blockIdx.y of the member axis, one entry per lane.  One segment in all: straight into `out`; else into the
// segment's row of `part` ((L0 + L1) entries per row, array 1 behind array 0)
__global__ __launch_bounds__(kMeanThreads) void traj_mean_reduce_kernel(const MeanOp op, int nb0)
{
    const MeanWhere w = mean_where(op, nb0);
    if (w.i < 0)
        return;
    const long long L = op.L[w.a];
    const int k0 = (int)blockIdx.y * kMeanSeg;
    const int cnt = op.E - k0 < kMeanSeg ? op.E - k0 : kMeanSeg;
    const double2 *__restrict__ s = op.src[w.a] + w.i + (size_t)L * k0;
    const double *__restrict__ v = op.v + k0;
    double2 acc;
    if (cnt == kMeanSeg) {                                   // a whole segment: every load in flight before the first FMA
        double2 t[kMeanSeg];
#pragma unroll
        for (int k = 0; k < kMeanSeg; ++k)
            t[k] = s[(size_t)L * k];
        acc.x = v[0] * t[0].x;
        acc.y = v[0] * t[0].y;
#pragma unroll
        for (int k = 1; k < kMeanSeg; ++k) {
            acc.x = fma(v[k], t[k].x, acc.x);
            acc.y = fma(v[k], t[k].y, acc.y);
        }
    } else {                                                 // the ragged last one: the same order
        const double2 t0 = s[0];
        acc.x = v[0] * t0.x;
        acc.y = v[0] * t0.y;
        for (int k = 1; k < cnt; ++k) {
            const double2 t = s[(size_t)L * k];
            acc.x = fma(v[k], t.x, acc.x);
            acc.y = fma(v[k], t.y, acc.y);
        }
    }
    const long long j = (w.a ? op.L[0] : 0) + w.i;
    if (gridDim.y == 1)
        op.out[j] = acc;
    else
        op.part[(size_t)blockIdx.y * (size_t)(op.L[0] + op.L[1]) + j] = acc;
}

// out[j] = the segments' sums added in segment order, one entry of [array 0 | array 1] per lane
__global__ __launch_bounds__(kMeanThreads) void traj_mean_combine_kernel(const MeanOp op, int nseg)
{
    const long long Lt = op.L[0] + op.L[1];
    const long long j = (long long)blockIdx.x * kMeanThreads + threadIdx.x;
    if (j >= Lt)
        return;
    const double2 *__restrict__ p = op.part + j;
    double2 acc = p[0];
    for (int s = 1; s < nseg; ++s) {
        const double2 t = p[(size_t)Lt * s];
        acc.x += t.x;
        acc.y += t.y;
    }
    op.out[j] = acc;
}

// the members of segment blockIdx.y, one entry per lane: the entry is read once, each member's copy is one product per component
__global__ __launch_bounds__(kMeanThreads) void traj_mean_broadcast_kernel(const MeanOp op, int nb0)
{
    const MeanWhere w = mean_where(op, nb0);
    if (w.i < 0)
        return;
    const long long L = op.L[w.a];
    const int k0 = (int)blockIdx.y * kMeanSeg;
    const int cnt = op.E - k0 < kMeanSeg ? op.E - k0 : kMeanSeg;
    const double2 s = op.in[(w.a ? op.L[0] : 0) + w.i];
    double2 *__restrict__ d = op.dst[w.a] + w.i + (size_t)L * k0;
    const double *__restrict__ v = op.v + k0;
    for (int k = 0; k < cnt; ++k) {
        double2 t;
        t.x = v[k] * s.x;
        t.y = v[k] * s.y;
        d[(size_t)L * k] = t;
    }
}

hipError_t run_traj_mean(const MeanOp &op, hipStream_t stream)
{
    if (op.E < 1 || !op.v || op.L[0] < 0 || op.L[1] < 0 || op.L[0] + op.L[1] < 1)
        return hipErrorInvalidValue;
    const long long nb0 = (op.L[0] + kMeanThreads - 1) / kMeanThreads, nb1 = (op.L[1] + kMeanThreads - 1) / kMeanThreads;
    const long long nseg = ((long long)op.E + kMeanSeg - 1) / kMeanSeg;
    if (nb0 + nb1 > 0x7fffffffll || nseg > 65535)
        return hipErrorInvalidValue;
    for (int a = 0; a < 2; ++a)
        if (op.L[a] > 0 && (op.broadcast ? !op.dst[a] : !op.src[a]))
            return hipErrorInvalidValue;
    const dim3 grid((unsigned)(nb0 + nb1), (unsigned)nseg);
    if (op.broadcast) {
        if (!op.in)
            return hipErrorInvalidValue;
        GRAPE_LAUNCH(traj_mean_broadcast_kernel, grid, dim3(kMeanThreads), 0, stream, op, (int)nb0);
        return hipGetLastError();
    }
    if (!op.out || (nseg > 1 && !op.part))
        return hipErrorInvalidValue;
    GRAPE_LAUNCH(traj_mean_reduce_kernel, grid, dim3(kMeanThreads), 0, stream, op, (int)nb0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || nseg == 1)
        return e;
    const long long Lt = op.L[0] + op.L[1];
    GRAPE_LAUNCH(traj_mean_combine_kernel, dim3((unsigned)((Lt + kMeanThreads - 1) / kMeanThreads)), dim3(kMeanThreads), 0, stream, op,
                 (int)nseg);
    return hipGetLastError();
}

}  // namespace grape
