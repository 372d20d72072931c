// vjp.hip -- the vector-Jacobian product of the trajectory read-out (grape_eval_vjp; the backward of grape_eval_observables)
// for the small-n family (n = 2, 3, 4; n x m states under left multiplication, UnitaryGate) on gfx950.
//
//   the caller's loss l is a function of y_{k,j,s} = tr(O_kj' X_{k,s}) and of X_{k,N}; its cotangents are
//   ybar = dl/dRe y + i dl/dIm y and Xbar likewise, so that dl = Re tr((ybar O)' dX) + Re tr(Xbar' dX_N)
//   Lam_{k,N} = Xbar_k + sum_j ybar[N,j,k] O_kj ,   Lam_{k,s} = P_s' Lam_{k,s+1} + sum_j ybar[s,j,k] O_kj
//   G[c,t]    = sum_k Re tr(Lam_{k,t+1}' B'_{k,c} X_{k,t+1}) ,   B' = -i dt B  (first order in dt, as grad_func!)
//
// It runs behind the sweep of the same launch and reads the propagators P_t that sweep left in the workspace (chunk-major:
// element e of slice t = c S + jj of member k at ((k S + jj) n^2 + e) CH + c).  The decomposition and the steps marked * are
// traj_chunk.hpp's: one workgroup per member of the launch, one lane per time chunk of S consecutive slices, every workspace
// access lane-contiguous:
//   1* chunk product Q_c = P_hi-1 ... P_lo
//   2* exclusive prefix scan of the Q_c over lanes (wave shuffles, wave totals through LDS): X at the chunk start
//   3  the states of the chunk: unitary flow: only X at the chunk END is kept and the last walk steps back with
//      X_s = P_s' X_s+1; general flow: a forward walk* stores X_s+1 per slice in the scratch of the chunk-major layout
//   4  backward walk from Lam = 0: b_c, the chunk's own contribution to the costate that leaves it on the left
//   5* suffix scan of the affine maps z -> Q_c' z + b_c over lanes, composition (Q1' Q2', Q1' b2 + b1) in a fixed tree
//   6  the same walk from the true incoming costate: Lam_t+1 at every slice and the K traces Re tr(B'_c X_t+1 Lam_t+1')
// The source of the recurrence does not depend on the states and is linear in the cotangents: ONE pair of walks serves any
// number of probes (running_cost_kernel walks once per term).  The probes are wave-uniform (scalar loads); ybar is read in
// the caller's layout (a lane reads its chunk's S + 1 consecutive entries of every probe row).
// Ragged decompositions: a lane whose chunk starts at or behind N owns no slice (Q = 1, b = 0), the last chunk may be short.
// The members' rows are unweighted, K N doubles each, written with plain vector stores; vjp_sum_kernel adds them in a tree
// fixed by the members' ensemble indices (groups of 32 in member order, then the groups in order), so a member-chunked
// launch sequence gives the bits of an unchunked one.
//
// STAGED (trajectory_vjp_staged_kernel; the device forms, SweepParams::vjp_staged): a member's ybar block is ONE contiguous run
// of n_obs (N + 1) entries, read twice (once per walk) at a lane stride of S 16 B.  The staged instance loads the block into
// LDS once, lane-contiguous, in front of the first walk (one barrier more, reached by every lane) and both walks read the
// image: every ybar byte leaves HBM once.  Same arithmetic, same order, same bits.
#include "cmat.hpp"
#include "grape_kernels.hpp"
#include "rc_mat.hpp"
#include "traj_chunk.hpp"

namespace grape {

// ops_all / o_all are separate `const __restrict__` arguments so that the wave-uniform operator and probe entries can be
// fetched with scalar loads (as in running_cost.hip).  UNI: every propagator is unitary.
// EXACT (grape_set_trajectory_derivative, GRAPE_TRAJ_EXACT): walk 6 stores W_t = X_t Lam_{t+1}' (n x n whatever m is; X_t the
// state BEFORE slice t) chunk-major into SweepParams::traj_w instead of the K traces; traj_frechet_rows_kernel
// (traj_frechet.hip) turns every W_t into the row entries behind this kernel.  Unitary flow: X_t is at hand after the step
// back X_t = P_t' X_{t+1}; general flow: the forward walk stores the state BEFORE every slice (slot jj: X_{lo+jj}).
template <int N, int M, bool UNI, int MAXT, bool STAGED, bool EXACT = false>
__global__ __launch_bounds__(MAXT) void trajectory_vjp_kernel(const double2 *__restrict__ ops_all,
                                                              const double2 *__restrict__ o_all,
                                                              const double2 *__restrict__ ybar_all,
                                                              const double2 *__restrict__ xbar_all, const SweepParams p)
{
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    __shared__ double2 s_q[MAXW][NN];              // wave totals: prefix products, then the affine maps' matrices ...
    __shared__ double2 s_v[MAXW][NM];              // ... and their offsets
    extern __shared__ double2 s_img[];             // STAGED: the member's ybar block, [j][s] as the caller lays it out

    const int K = p.K, Nsl = p.N, n_obs = ybar_all ? p.vjp_n : 0;
    const int k = blockIdx.x;                        // member within the launch: row of the workspace and of the rows
    const int kg = k + p.vjp_E0;                     // member of the ensemble: row of the probes and of the cotangents
    const TrajLane<N> ln = traj_lane<N>(p.vjp_CH, p.S, Nsl, p.props, k);
    const int L = ln.L, lo = ln.lo, cnt = ln.cnt;
    const size_t stride = ln.stride;
    double2 *__restrict__ Xw = UNI ? nullptr : ln.template ws<NM>(p.vjp_xs);
    const TrajOps op = traj_ops<N>(ops_all, k, K);
    const double2 *__restrict__ opB = op.opB;
    const TrajProbes pr = traj_probes<N, M>(o_all, p.vjp_per_member, p.vjp_Etot, kg, Nsl);
    const size_t y_step = pr.y_step;
    const double2 *__restrict__ yb = ybar_all ? ybar_all + (size_t)kg * p.vjp_n * y_step : nullptr;
    double *__restrict__ row = p.vjp_rows + (size_t)k * K * Nsl;
    if constexpr (STAGED) {                          // (the barrier in front of the first walk publishes the image)
        if (yb) {                                    // eight 16 B loads in flight per lane: one load per round trip left the
            const int tot = n_obs * (Nsl + 1), bd = (int)blockDim.x;      // 16-probe block (31 trips) slower than two strided reads
            int i = L;
            for (; i + 7 * bd < tot; i += 8 * bd) {
                double2 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    v[u] = yb[i + u * bd];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    s_img[i + u * bd] = v[u];
            }
            for (; i < tot; i += bd)
                s_img[i] = yb[i];
        }
    }

    // ---------------------------------------------------------------- 1, 2: chunk product, X at the chunk start
    CMat<N> Q, P;
    traj_chunk_product(Q, ln);
    CRect<N, M> Xhi;
    {
        CMat<N> U;
        traj_prefix_start(U, Q, ln, s_q);
        CRect<N, M> Xs;
        traj_start_state(Xs, U, op.opXi);
        // ------------------------------------------------------------ 3: the chunk's states
        if (UNI) {
            rmul(Xhi, Q, Xs);
        } else {
            Xhi = Xs;
            traj_walk_store<N, M, EXACT>(Xhi, ln, Xw);
        }
    }

    // one backward walk over the chunk from the costate Lam that enters it on the right; EMIT: with the gradient traces (the
    // only place the states are needed: the source is the caller's)
    auto walk = [&](CRect<N, M> &Lam, const bool emit) {
        CRect<N, M> X = Xhi, Tm;
        for (int jj = cnt - 1; jj >= 0; --jj) {
            const int t = lo + jj;                   // slice index; the state behind it is X_{t+1}, cotangent row s = t + 1
            rc_load_mat(P, ln.P(jj), stride);
            if (xbar_all && t + 1 == Nsl) {          // Lam_N starts from Xbar
                const double2 *__restrict__ xb = xbar_all + (size_t)kg * NM;
#pragma unroll
                for (int e = 0; e < NM; ++e) {
                    const double2 v = xb[e];
                    Lam.re[e] += v.x;
                    Lam.im[e] += v.y;
                }
            }
            for (int j = 0; j < n_obs; ++j) {        // Lam_{t+1} = (what came from the right) + sum_j ybar O_j
                double2 c;
                if constexpr (STAGED)
                    c = s_img[(t + 1) + j * (Nsl + 1)];
                else
                    c = yb[(size_t)(t + 1) + (size_t)j * y_step];
                const double2 *__restrict__ o = pr.probe(j);
#pragma unroll
                for (int e = 0; e < NM; ++e) {
                    const double2 v = o[e];
                    Lam.re[e] = fma(c.x, v.x, fma(-c.y, v.y, Lam.re[e]));
                    Lam.im[e] = fma(c.x, v.y, fma(c.y, v.x, Lam.im[e]));
                }
            }
            if (emit) {
                if constexpr (EXACT) {
                    if (UNI) {
                        rmul_ah(Tm, P, X);           // X_t = P_t' X_{t+1}
                        X = Tm;
                    } else {
                        rload_ws(X, Xw + (size_t)jj * NM * stride, stride);
                    }
                    CMat<N> Mx;
                    rmul_a_bh(Mx, X, Lam);           // W_t = X_t Lam_{t+1}'
                    double2 *__restrict__ wp = ln.template slot<NN>(p.traj_w, jj);
#pragma unroll
                    for (int e = 0; e < NN; ++e)
                        wp[e * stride] = make_double2(Mx.re[e], Mx.im[e]);
                } else {
                    if (!UNI)
                        rload_ws(X, Xw + (size_t)jj * NM * stride, stride);
                    CMat<N> Mx;
                    rmul_a_bh(Mx, X, Lam);               // X Lam'
                    for (int c = 0; c < K; ++c) {
                        double re = 0.0;
#pragma unroll
                        for (int b2 = 0; b2 < N; ++b2)
#pragma unroll
                            for (int a2 = 0; a2 < N; ++a2) {
                                const double2 b = opB[c * NN + a2 + b2 * N];
                                re = fma(b.x, Mx.re[b2 + a2 * N], re);
                                re = fma(-b.y, Mx.im[b2 + a2 * N], re);
                            }
                        row[(size_t)t * K + c] = re;
                    }
                    if (UNI) {
                        rmul_ah(Tm, P, X);
                        X = Tm;
                    }
                }
            }
            rmul_ah(Tm, P, Lam);                     // pull the costate back over slice t
            Lam = Tm;
        }
    };
    // ---------------------------------------------------------------- 4: the chunk's affine map
    CRect<N, M> bvec;
    rzero(bvec);
    if constexpr (STAGED)
        __syncthreads();                             // the image is complete (every lane arrives: no path above leaves)
    walk(bvec, false);
    // ---------------------------------------------------------------- 5: suffix scan of (Q', b)
    CRect<N, M> Lin;
    traj_affine_suffix(Lin, Q, bvec, ln, s_q, s_v);
    // ---------------------------------------------------------------- 6: the true costates, the traces
    walk(Lin, true);
}

// The members' rows -> G in a tree fixed by the members' ensemble indices, whatever the member blocks of the launches are:
//   grp > 0   part[g][q] = sum of rows[m][q] over the members m of group g = m / grp, ascending, for the members [E0, E0 + E)
//             of this launch (one thread per (q, group)); a group that a previous launch began goes on from the partial sum
//             that launch left in part -- the same chain of additions as in one piece
//   grp == 0  dst[q] = sum of the E rows of `rows`, ascending: the groups' sums into G, behind the last member block
// A single chain over 1024 members took 250 us of dependent 16 KB-strided loads on 32 waves at the headline shape.
__global__ __launch_bounds__(256) void vjp_sum_kernel(const double *__restrict__ rows, double *__restrict__ dst, int E0, int E,
                                                      int Q, int grp)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q)
        return;
    int lo = 0, hi = E;                              // rows of this thread, relative to the launch
    double acc = 0.0;
    if (grp > 0) {
        const int g = E0 / grp + blockIdx.y;
        lo = max(g * grp, E0) - E0;
        hi = min((g + 1) * grp, E0 + E) - E0;
        dst += (size_t)g * Q;
        if (lo + E0 != g * grp)
            acc = dst[q];
    }
    const double *__restrict__ src = rows + q;
    int m = lo;
    for (; m + 8 <= hi; m += 8) {                    // eight loads in flight, added in order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            v[u] = src[(size_t)(m + u) * Q];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            acc += v[u];
    }
    for (; m < hi; ++m)
        acc += src[(size_t)m * Q];
    dst[q] = acc;
}

template <int N, int M>
static hipError_t vjp_launch_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = RcTraits<N>::MAXT;
    const int threads = (p.vjp_CH + 63) & ~63;
    if (threads > MAXT || p.vjp_CH < 1 || (long long)p.S * p.vjp_CH < p.N || p.N < 1 || p.E < 1 || p.K < 1 || p.vjp_E0 < 0 ||
        p.vjp_E0 + p.E > p.vjp_Etot || p.vjp_n < 0 || p.vjp_n > 16 || (!p.vjp_ybar && !p.vjp_xbar) ||
        (p.vjp_ybar && (p.vjp_n < 1 || !p.vjp_O)) || !p.vjp_rows || !p.vjp_part || (!p.vjp_unitary && !p.vjp_xs) || !p.props ||
        !p.ops || (long long)p.K * p.N > 0x7fffff00ll)
        return hipErrorInvalidConfiguration;
    const dim3 grid(p.E), block(threads);
    hipError_t e = hipSuccess;
    if (p.traj_exact) {
        // the exact derivative mode: the direct instance alone (vjp_staged is ignored), W_t into traj_w, then one Frechet
        // derivative per (member, slice) into the rows
        if (!p.traj_w || !p.traj_x)
            return hipErrorInvalidConfiguration;
        if (p.vjp_unitary)
            GRAPE_LAUNCH_AS("trajectory_vjp_exact_kernel", (trajectory_vjp_kernel<N, M, true, MAXT, false, true>), grid, block, 0, stream,
                            p.ops, p.vjp_O, p.vjp_ybar, p.vjp_xbar, p);
        else
            GRAPE_LAUNCH_AS("trajectory_vjp_exact_kernel", (trajectory_vjp_kernel<N, M, false, MAXT, false, true>), grid, block, 0, stream,
                            p.ops, p.vjp_O, p.vjp_ybar, p.vjp_xbar, p);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
        e = run_traj_frechet(N, false, p, stream);
        if (e != hipSuccess)
            return e;
    } else if (p.vjp_staged) {
        // the image is exactly the member's block, and static + dynamic LDS fit a workgroup of this device
        const size_t lds = (size_t)p.vjp_staged;
        if (!p.vjp_ybar || lds != sizeof(double2) * (size_t)p.vjp_n * ((size_t)p.N + 1))
            return hipErrorInvalidConfiguration;
        int dev = 0, cap = 0;
        e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        if (e != hipSuccess) return e;
        if (lds + traj_static_lds(N, M, true) > (size_t)cap) return hipErrorInvalidConfiguration;
        const auto kern = p.vjp_unitary ? trajectory_vjp_kernel<N, M, true, MAXT, true> : trajectory_vjp_kernel<N, M, false, MAXT, true>;
        e = ensure_dynamic_lds((const void *)kern, lds);
        if (e != hipSuccess) return e;
        GRAPE_LAUNCH_AS("trajectory_vjp_staged_kernel", kern, grid, block, lds, stream, p.ops, p.vjp_O, p.vjp_ybar, p.vjp_xbar, p);
    } else if (p.vjp_unitary)
        GRAPE_LAUNCH_AS("trajectory_vjp_kernel", (trajectory_vjp_kernel<N, M, true, MAXT, false>), grid, block, 0, stream, p.ops, p.vjp_O,
                        p.vjp_ybar, p.vjp_xbar, p);
    else
        GRAPE_LAUNCH_AS("trajectory_vjp_kernel", (trajectory_vjp_kernel<N, M, false, MAXT, false>), grid, block, 0, stream, p.ops, p.vjp_O,
                        p.vjp_ybar, p.vjp_xbar, p);
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    return launch_vjp_rows_sum(p, stream);
}

// the rows of this launch's members onto the sums of their groups (behind trajectory_vjp_kernel, and behind
// trajectory_hvp_kernel of hvp.hip, which writes the same rows)
hipError_t launch_vjp_rows_sum(const SweepParams &p, hipStream_t stream)
{
    const int Q = p.K * p.N;
    const int groups = (p.vjp_E0 + p.E - 1) / kVjpGroup - p.vjp_E0 / kVjpGroup + 1;
    GRAPE_LAUNCH(vjp_sum_kernel, dim3((Q + 255) / 256, groups), dim3(256), 0, stream, p.vjp_rows, p.vjp_part, p.vjp_E0, p.E, Q,
                 kVjpGroup);
    return hipGetLastError();
}

// behind the last member block: the groups' sums, in group order, into G
static hipError_t vjp_launch_total(const SweepParams &p, hipStream_t stream)
{
    const long long Q = (long long)p.K * p.N;
    if (p.K < 1 || p.N < 1 || p.vjp_Etot < 1 || Q > 0x7fffff00ll || !p.vjp_part || !p.vjp_G)
        return hipErrorInvalidConfiguration;
    GRAPE_LAUNCH(vjp_sum_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, stream, p.vjp_part, p.vjp_G, 0,
                 (p.vjp_Etot + kVjpGroup - 1) / kVjpGroup, (int)Q, 0);
    return hipGetLastError();
}

hipError_t run_trajectory_vjp(int n, const SweepParams &p, hipStream_t stream)
{
    if (p.vjp_only == 2)
        return vjp_launch_total(p, stream);
    return dispatch_nm(n, p.vjp_m, [&](auto N, auto M) {
        return vjp_launch_nm<decltype(N)::value, decltype(M)::value>(p, stream);
    });
}

}  // namespace grape
