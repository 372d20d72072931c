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
//
// ONE kernel template serves grape_eval_vjp and grape_eval_vjp_multi: trajectory_vjp_kernel<N, M, UNI, MAXT, STAGED, EXACT, RB>
// pulls RB cotangent sets back next to ONE chunk product, ONE prefix scan, ONE start state, ONE state image of the general
// flow, ONE propagator load per slice of either walk and ONE step back X_t = P_t' X_{t+1} of the unitary flow.  Per set: its
// sources (ybar row, Xbar), its costate, its chunk offset b_r, M_r = X Lam_r' and its K traces; the affine suffix scan carries
// one matrix part and RB offsets.  Per set the operations and their order do not depend on RB: block r of a multi call holds
// the single call's bits.  RB = 1, bound to RcTraits<N>::MAXT threads, is the single call under its names; the multi instances
// (reported as trajectory_vjp_multi_kernel: direct ybar reads, first-order mode) are bound to 256 threads for every n (one
// wave per SIMD, 512 registers per lane), RB per (n, m) is vjp_multi_block.  Set r reads ybar + r vjp_set_ybar /
// xbar + r vjp_set_xbar and writes its members' rows at vjp_rows + r vjp_set_rows; nr <= RB sets are live in a launch (the
// ragged last block), uniform over the grid.
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
// RB sets ride next to ONE state walk; RB = 1 is the single call: its one set is live by construction, every guard is a
// compile-time constant, its suffix scan is traj_affine_suffix, and it reads neither vjp_nset nor the vjp_set_* strides.
template <int N, int M, bool UNI, int MAXT, bool STAGED, bool EXACT = false, int RB = 1>
__global__ __launch_bounds__(MAXT) void trajectory_vjp_kernel(const double2 *__restrict__ ops_all,
                                                              const double2 *__restrict__ o_all,
                                                              const double2 *__restrict__ ybar_all,
                                                              const double2 *__restrict__ xbar_all, const SweepParams p)
{
    static_assert(RB == 1 || (!STAGED && !EXACT), "the multi instances read ybar directly, in the first-order mode");
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    // the unitary flow keeps X at the chunk end from step 3 to walk 6.  Across the suffix scan of a block that is the seventh
    // n x m block alive (Go, G, z, Tm, two offsets), 448 of the 512 registers at n = m = 4 before any address: the instance
    // parks it in the dynamic LDS image (one 16 B column per lane and element, lane-contiguous) and takes it back for walk 6
    constexpr bool STASH = RB > 1 && UNI && vjp_multi_stash(N, M);
    __shared__ double2 s_q[MAXW][NN];              // wave totals: prefix products, then the affine maps' matrices ...
    __shared__ double2 s_v[MAXW][RB][NM];          // ... and their offsets, one per set
    extern __shared__ double2 s_img[];             // STAGED: the member's ybar block, [j][s] as the caller lays it out; STASH: X

    const int K = p.K, Nsl = p.N, n_obs = ybar_all ? p.vjp_n : 0;
    const int nr = RB == 1 ? 1 : p.vjp_nset;         // live sets of this launch, 1..RB
    // set r's arrays lie r strides behind set 0's (RB = 1: there is no other set, the fields are not read)
    const size_t ys = RB == 1 ? 0 : (size_t)p.vjp_set_ybar, xs = RB == 1 ? 0 : (size_t)p.vjp_set_xbar;
    const size_t rs = RB == 1 ? 0 : (size_t)p.vjp_set_rows;
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
            if constexpr (STASH) {                   // (each lane its own column of the image: nothing to wait for)
#pragma unroll
                for (int e = 0; e < NM; ++e)
                    s_img[e * blockDim.x + L] = make_double2(Xhi.re[e], Xhi.im[e]);
            }
        } else {
            Xhi = Xs;
            traj_walk_store<N, M, EXACT>(Xhi, ln, Xw);
        }
    }

    // one backward walk over the chunk from the costates Lam_r that enter it on the right; EMIT: with the gradient traces (the
    // only place the states are needed: the source is the caller's).  P and X once per slice, the rest per set.
    auto walk = [&](CRect<N, M> (&Lam)[RB], const bool emit) {
        CRect<N, M> X = Xhi, Tm;
        for (int jj = cnt - 1; jj >= 0; --jj) {
            const int t = lo + jj;                   // slice index; the state behind it is X_{t+1}, cotangent row s = t + 1
            rc_load_mat(P, ln.P(jj), stride);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (r < nr) {
                    if (xbar_all && t + 1 == Nsl) {  // Lam_N starts from Xbar
                        const double2 *__restrict__ xb = xbar_all + (size_t)r * xs + (size_t)kg * NM;
#pragma unroll
                        for (int e = 0; e < NM; ++e) {
                            const double2 v = xb[e];
                            Lam[r].re[e] += v.x;
                            Lam[r].im[e] += v.y;
                        }
                    }
                    for (int j = 0; j < n_obs; ++j) {        // Lam_{t+1} = (what came from the right) + sum_j ybar O_j
                        double2 c;
                        if constexpr (STAGED)
                            c = s_img[(t + 1) + j * (Nsl + 1)];
                        else
                            c = yb[(size_t)r * ys + (size_t)(t + 1) + (size_t)j * y_step];
                        const double2 *__restrict__ o = pr.probe(j);
#pragma unroll
                        for (int e = 0; e < NM; ++e) {
                            const double2 v = o[e];
                            Lam[r].re[e] = fma(c.x, v.x, fma(-c.y, v.y, Lam[r].re[e]));
                            Lam[r].im[e] = fma(c.x, v.y, fma(c.y, v.x, Lam[r].im[e]));
                        }
                    }
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
                    rmul_a_bh(Mx, X, Lam[0]);        // W_t = X_t Lam_{t+1}'
                    double2 *__restrict__ wp = ln.template slot<NN>(p.traj_w, jj);
#pragma unroll
                    for (int e = 0; e < NN; ++e)
                        wp[e * stride] = make_double2(Mx.re[e], Mx.im[e]);
                } else {
                    if (!UNI)
                        rload_ws(X, Xw + (size_t)jj * NM * stride, stride);
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        if (r < nr) {
                            CMat<N> Mx;
                            rmul_a_bh(Mx, X, Lam[r]);        // X Lam_r'
                            double *__restrict__ rr = row + (size_t)r * rs;
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
                                rr[(size_t)t * K + c] = re;
                            }
                        }
                    }
                    if (UNI) {
                        rmul_ah(Tm, P, X);
                        X = Tm;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (r < nr) {
                    rmul_ah(Tm, P, Lam[r]);          // pull the costate back over slice t
                    Lam[r] = Tm;
                }
            }
        }
    };
    // ---------------------------------------------------------------- 4: the chunk's affine map
    CRect<N, M> bvec[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r)
        rzero(bvec[r]);
    if constexpr (STAGED)
        __syncthreads();                             // the image is complete (every lane arrives: no path above leaves)
    walk(bvec, false);
    // ---------------------------------------------------------------- 5: suffix scan of (Q', b_0 .. b_nr-1)
    CRect<N, M> Lin[RB];
    if constexpr (RB == 1) {
        traj_affine_suffix(Lin[0], Q, bvec[0], ln, s_q, &s_v[0][0]);
    } else {
        // traj_affine_suffix with one matrix part and an offset per set, written out here, its one user (as the forward twin
        // in jvp.hip): the function of traj_chunk.hpp stays what the single instance and trajectory_hvp_kernel compile today.
        // Per set: that function's operations in its order (the offsets first, each with the old G).
        const int lane = ln.lane, wave = ln.wave, W = ln.W;
        CMat<N> G = Q, Go, T;
        CRect<N, M> vo, Tm;
        for (int d = 1; d < 64; d <<= 1) {           // [L, L+d) then [L+d, L+2d):  (Go G)' z + (G' vo + v)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (r < nr) {
                    rshfl_down(vo, bvec[r], d);
                    if (lane + d < 64) {
                        rmul_ah(Tm, G, vo);
#pragma unroll
                        for (int e = 0; e < NM; ++e) {
                            bvec[r].re[e] += Tm.re[e];
                            bvec[r].im[e] += Tm.im[e];
                        }
                    }
                }
            }
            shfl_down(Go, G, d);
            if (lane + d < 64) {
                mul(T, Go, G);
                G = T;
            }
        }
        shfl_down(Go, G, 1);                         // the lanes behind this one, inside the wave
        if (lane == 63)
            set_identity(Go);
        if (W > 1) {
            __syncthreads();                         // (the readers of the prefix totals in s_q are done)
            if (lane == 0) {
#pragma unroll
                for (int e = 0; e < NN; ++e)
                    s_q[wave][e] = make_double2(G.re[e], G.im[e]);
#pragma unroll
                for (int r = 0; r < RB; ++r)
                    if (r < nr) {
#pragma unroll
                        for (int e = 0; e < NM; ++e)
                            s_v[wave][r][e] = make_double2(bvec[r].re[e], bvec[r].im[e]);
                    }
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            if (r < nr) {
                rshfl_down(vo, bvec[r], 1);
                if (lane == 63)
                    rzero(vo);
                if (W > 1) {
                    CRect<N, M> z;
                    rzero(z);
                    for (int w = W - 1; w > wave; --w) {     // what enters this wave on the right, last wave first
                        rc_load_lds(G, &s_q[w][0]);
                        rmul_ah(Tm, G, z);
#pragma unroll
                        for (int e = 0; e < NM; ++e) {
                            const double2 vv = s_v[w][r][e];
                            z.re[e] = Tm.re[e] + vv.x;
                            z.im[e] = Tm.im[e] + vv.y;
                        }
                    }
                    rmul_ah(Tm, Go, z);
#pragma unroll
                    for (int e = 0; e < NM; ++e) {
                        Lin[r].re[e] = Tm.re[e] + vo.re[e];
                        Lin[r].im[e] = Tm.im[e] + vo.im[e];
                    }
                } else {
                    Lin[r] = vo;
                }
            } else {
                rzero(Lin[r]);
            }
        }
    }
    // ---------------------------------------------------------------- 6: the true costates, the traces
    if constexpr (STASH) {
#pragma unroll
        for (int e = 0; e < NM; ++e) {
            const double2 v = s_img[e * blockDim.x + L];
            Xhi.re[e] = v.x;
            Xhi.im[e] = v.y;
        }
    }
    walk(Lin, true);
}

// The members' rows -> G in a tree fixed by the members' ensemble indices, whatever the member blocks of the launches are:
//   grp > 0   part[g][q] = sum of rows[m][q] over the members m of group g = m / grp, ascending, for the members [E0, E0 + E)
//             of this launch (one thread per (q, group)); a group that a previous launch began goes on from the partial sum
//             that launch left in part -- the same chain of additions as in one piece
//   grp == 0  dst[q] = sum of the E rows of `rows`, ascending: the groups' sums into G, behind the last member block
// A single chain over 1024 members took 250 us of dependent 16 KB-strided loads on 32 waves at the headline shape.
// grape_eval_vjp_multi: blockIdx.z is the cotangent set, whose rows / sums lie src_set / dst_set doubles behind set 0's; every
// set's elements are added in exactly the single call's chain.  (The single call launches one z layer.)
__global__ __launch_bounds__(256) void vjp_sum_kernel(const double *__restrict__ rows, double *__restrict__ dst, int E0, int E,
                                                      int Q, int grp, size_t src_set, size_t dst_set)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q)
        return;
    rows += (size_t)blockIdx.z * src_set;
    dst += (size_t)blockIdx.z * dst_set;
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

// what every launch of the kernel above requires; threads is the workgroup size of the decomposition
template <int N>
static bool vjp_launch_ok(const SweepParams &p, int threads)
{
    return !(threads > RcTraits<N>::MAXT || p.vjp_CH < 1 || (long long)p.S * p.vjp_CH < p.N || p.N < 1 || p.E < 1 || p.K < 1 ||
             p.vjp_E0 < 0 || p.vjp_E0 + p.E > p.vjp_Etot || p.vjp_n < 0 || p.vjp_n > 16 || (!p.vjp_ybar && !p.vjp_xbar) ||
             (p.vjp_ybar && (p.vjp_n < 1 || !p.vjp_O)) || !p.vjp_rows || !p.vjp_part || (!p.vjp_unitary && !p.vjp_xs) ||
             !p.props || !p.ops || (long long)p.K * p.N > 0x7fffff00ll);
}

// the single call: the RB = 1 instances
template <int N, int M>
static hipError_t vjp_launch_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = RcTraits<N>::MAXT;
    const int threads = (p.vjp_CH + 63) & ~63;
    if (!vjp_launch_ok<N>(p, threads))
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
// trajectory_hvp_kernel of hvp.hip, which writes the same rows); vjp_nset > 0: of every set of the launch
hipError_t launch_vjp_rows_sum(const SweepParams &p, hipStream_t stream)
{
    const int Q = p.K * p.N;
    const int groups = (p.vjp_E0 + p.E - 1) / kVjpGroup - p.vjp_E0 / kVjpGroup + 1;
    GRAPE_LAUNCH(vjp_sum_kernel, dim3((Q + 255) / 256, groups, p.vjp_nset > 0 ? p.vjp_nset : 1), dim3(256), 0, stream, p.vjp_rows,
                 p.vjp_part, p.vjp_E0, p.E, Q, kVjpGroup, (size_t)p.vjp_set_rows, (size_t)p.vjp_set_part);
    return hipGetLastError();
}

// behind the last member block: the groups' sums, in group order, into G (vjp_nset > 0: every set's)
static hipError_t vjp_launch_total(const SweepParams &p, hipStream_t stream)
{
    const long long Q = (long long)p.K * p.N;
    if (p.K < 1 || p.N < 1 || p.vjp_Etot < 1 || Q > 0x7fffff00ll || !p.vjp_part || !p.vjp_G)
        return hipErrorInvalidConfiguration;
    GRAPE_LAUNCH(vjp_sum_kernel, dim3((unsigned)((Q + 255) / 256), 1, p.vjp_nset > 0 ? p.vjp_nset : 1), dim3(256), 0, stream,
                 p.vjp_part, p.vjp_G, 0, (p.vjp_Etot + kVjpGroup - 1) / kVjpGroup, (int)Q, 0, (size_t)p.vjp_set_part,
                 (size_t)p.vjp_set_G);
    return hipGetLastError();
}

// sets [r0, r0 + nr) of a multi-set launch as a launch of their own (nr = 0: set r0 alone as the single call)
static SweepParams vjp_sets(const SweepParams &p, int r0, int nr)
{
    SweepParams q = p;
    q.vjp_nset = nr;
    if (p.vjp_ybar) q.vjp_ybar = p.vjp_ybar + (size_t)r0 * p.vjp_set_ybar;
    if (p.vjp_xbar) q.vjp_xbar = p.vjp_xbar + (size_t)r0 * p.vjp_set_xbar;
    q.vjp_rows = p.vjp_rows + (size_t)r0 * p.vjp_set_rows;
    q.vjp_part = p.vjp_part + (size_t)r0 * p.vjp_set_part;
    return q;
}

// grape_eval_vjp_multi: p.vjp_nset sets in blocks of RB through the multi instance (trajectory_vjp_multi_kernel), or (no
// instance for this launch -- more than 256 time chunks per member, the exact mode -- or not asked for) one behind the other
// through the single call's kernels -- the same bits either way.  Every set's rows end on its own groups' sums.
template <int N, int M>
static hipError_t vjp_launch_multi_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int RB = vjp_multi_block(N, M), MAXT = kVjpMultiMaxThreads;  // (RB = 0: no multi instance at this shape)
    const int threads = (p.vjp_CH + 63) & ~63, nset = p.vjp_nset;
    if (nset < 1 || nset > 64 || p.vjp_set_ybar < 0 || p.vjp_set_xbar < 0 || p.vjp_set_rows < (long long)p.E * p.K * p.N ||
        p.vjp_set_part < 0 || !p.vjp_rows || !p.vjp_part)
        return hipErrorInvalidConfiguration;
    if (RB < 2 || !p.vjp_multi || threads > MAXT || p.traj_exact) {
        for (int r = 0; r < nset; ++r) {
            const hipError_t e = vjp_launch_nm<N, M>(vjp_sets(p, r, 0), stream);
            if (e != hipSuccess)
                return e;
        }
        return hipSuccess;
    }
    if constexpr (RB >= 2) {
    // a block of ONE set (n_set = 1, or the ragged remainder) takes the single kernels unless the multi kernel is forced
    // (vjp_multi = 2)
    for (int r0 = 0; r0 < nset; r0 += RB) {
        SweepParams q = vjp_sets(p, r0, nset - r0 < RB ? nset - r0 : RB);
        if (q.vjp_nset == 1 && p.vjp_multi == 1) {
            const hipError_t e = vjp_launch_nm<N, M>(vjp_sets(q, 0, 0), stream);
            if (e != hipSuccess)
                return e;
            continue;
        }
        q.vjp_staged = 0;                            // (the multi instance reads ybar directly)
        if (!vjp_launch_ok<N>(q, threads))
            return hipErrorInvalidConfiguration;
        if (q.vjp_unitary) {
            const auto kern = trajectory_vjp_kernel<N, M, true, MAXT, false, false, RB>;
            // (n = m = 4: the image that holds X at the chunk end across the scan, n m 16 B per lane)
            const size_t lds = vjp_multi_stash(N, M) ? sizeof(double2) * (size_t)threads * N * M : 0;
            if (lds) {
                const hipError_t el = ensure_dynamic_lds((const void *)kern, lds);
                if (el != hipSuccess)
                    return el;
            }
            GRAPE_LAUNCH_AS("trajectory_vjp_multi_kernel", kern, dim3(q.E), dim3(threads), lds, stream, q.ops, q.vjp_O, q.vjp_ybar,
                            q.vjp_xbar, q);
        } else
            GRAPE_LAUNCH_AS("trajectory_vjp_multi_kernel", (trajectory_vjp_kernel<N, M, false, MAXT, false, false, RB>), dim3(q.E),
                            dim3(threads), 0, stream, q.ops, q.vjp_O, q.vjp_ybar, q.vjp_xbar, q);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
        e = launch_vjp_rows_sum(q, stream);
        if (e != hipSuccess)
            return e;
    }
    }
    return hipSuccess;
}

hipError_t run_trajectory_vjp(int n, const SweepParams &p, hipStream_t stream)
{
    if (p.vjp_only == 2)
        return vjp_launch_total(p, stream);
    return dispatch_nm(n, p.vjp_m, [&](auto N, auto M) {
        constexpr int Nn = decltype(N)::value, Mm = decltype(M)::value;
        return p.vjp_nset > 0 ? vjp_launch_multi_nm<Nn, Mm>(p, stream) : vjp_launch_nm<Nn, Mm>(p, stream);
    });
}

}  // namespace grape
