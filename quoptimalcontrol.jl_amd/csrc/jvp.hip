// jvp.hip -- the Jacobian-vector product of the trajectory read-out (grape_eval_jvp; the forward-mode twin of grape_eval_vjp)
// for the small-n family (n = 2, 3, 4; n x m states under left multiplication, UnitaryGate) on gfx950.
//
//   the caller's direction xdot (K, N) in the PHYSICAL pulse's coordinates (the host layer has applied the pulse map's tangent)
//   V_t = sum_c xdot[c,t] B'_{k,c} ,   B' = -i dt B  (first order in dt: grape_eval_vjp's rule, its exact transpose)
//   D_{k,0} = 0 ,   D_{k,t+1} = P_{k,t} D_{k,t} + V_t X_{k,t+1} ,   X_{k,t+1} = P_{k,t} X_{k,t}
//   ydot[s, j, k] = tr(O_kj' D_{k,s}) ,  s = 0..N  (row 0 is zero and written) ,   Xdot_final_k = D_{k,N}
//
// It runs behind the sweep of the same launch and reads the propagators P_t that sweep left in the workspace (chunk-major:
// element e of slice t = c S + jj of member k at ((k S + jj) n^2 + e) CH + c).  The decomposition and the steps it shares with
// the other kernels behind the sweeps are traj_chunk.hpp's: one workgroup per member of the launch, one lane per time chunk of
// S consecutive slices, every workspace access lane-contiguous:
//   1  ONE forward walk over the chunk in relative form, carrying R = P_t ... P_lo (from 1) and its tangent Rdot (from 0),
//      Rdot <- P Rdot + V_t R_{t+1}: the chunk product Q_c = R and, with the state at the chunk start, the chunk's own
//      contribution d_c = Rdot X_lo to the tangent that leaves it on the right -- the chunk product and the walk from D = 0
//      of the pull-back's decomposition in one pass over the propagators, with two n x n blocks live next to P and V
//      (a walk on X and D would keep Q and X_lo alive across the loop: six blocks, and scratch traffic in it at n = m = 3)
//   2  exclusive prefix scan of the Q_c over lanes (traj_prefix_start): X at the chunk start, d_c
//   3  exclusive prefix scan of the affine maps z -> Q_c z + d_c over lanes, composition (Q2 Q1, Q2 d1 + d2) in a fixed tree:
//      the forward twin of the pull-back's suffix scan (traj_affine_suffix), written out in the kernel
//   4  the walk on X and D from the true incoming tangent: D_t+1 behind every slice and its n_obs traces, D_N on slice N - 1
// The states are walked forward WITH the tangent in both walks (X_t+1 is what V_t multiplies), so neither flow stores states
// and one instance serves unitary and non-unitary propagators.  The probes are wave-uniform (scalar loads); xdot is read in
// the caller's layout (a lane's chunk is K S consecutive doubles).
// Ragged decompositions: a lane whose chunk starts at or behind N owns no slice (Q = 1, d = 0), the last chunk may be short.
// Members are independent: no sum over members, plain vector stores, every number has one fixed evaluation order, so a
// member-chunked launch sequence gives the bits of an unchunked one.  Every operation is linear in xdot (products and FMAs
// whose addends all carry one factor of it): 2 xdot gives twice the bits, -xdot the negated ones, 0 gives 0.
//
// The ydot stores are direct (lane c stores at s = c S + jj: neighbouring lanes S 16 B apart in a probe row); there is no
// staged instance.
//
// ONE kernel template serves grape_eval_jvp and grape_eval_jvp_multi: trajectory_jvp_kernel<N, M, MAXT, DB, EXACT> carries DB
// tangents through the four steps next to ONE chunk product, ONE scan of Q and ONE state walk -- R once and Rdot per direction
// in step 1, the affine scan with one matrix part and an offset per direction, X once and D per direction in step 4 -- so the
// propagators are read once per pass for the block.  Per direction the operations and their order do not depend on DB: block
// d of a multi call holds the single call's bits.  DB = 1, bound to RcTraits<N>::MAXT threads, is the single call (reported as
// trajectory_jvp_kernel / trajectory_jvp_exact_kernel); the multi instances (reported as trajectory_jvp_multi_kernel /
// trajectory_jvp_multi_exact_kernel) are bound to 256 threads for every n (one wave per SIMD, 512 registers per lane), DB per
// (n, m) is jvp_multi_block.
#include "cmat.hpp"
#include "grape_kernels.hpp"
#include "rc_mat.hpp"
#include "traj_chunk.hpp"

namespace grape {

// one slice of the tangent recurrence on an n x c block and its DB tangents, nd of them live:
//   X <- P X,  D_d <- P D_d + V_d X  with  V_d = sum_c xd_d[c] B'_c   (direction d's xdot row at xd + d xs)
// (opB: the member's K prescaled control operators, wave-uniform; V_d is built from zero in the registers P has left, one
// direction after the other)
template <int N, int C, int DB>
GRAPE_DEV void jvp_step(CRect<N, C> &X, CRect<N, C> (&D)[DB], int nd, const double2 *__restrict__ Pt, size_t stride,
                        const double *__restrict__ xd, size_t xs, const double2 *__restrict__ opB, int K)
{
    CMat<N> P;
    rc_load_mat(P, Pt, stride);
    rmul_inplace(X, P);
#pragma unroll
    for (int d = 0; d < DB; ++d)
        if (d < nd)
            rmul_inplace(D[d], P);
#pragma unroll
    for (int d = 0; d < DB; ++d) {
        if (d < nd) {
            const double *__restrict__ xdd = xd + (size_t)d * xs;
#pragma unroll
            for (int e = 0; e < N * N; ++e) {
                P.re[e] = 0.0;
                P.im[e] = 0.0;
            }
#pragma unroll 1
            for (int c = 0; c < K; ++c) {
                const double a = xdd[c];
#pragma unroll
                for (int e = 0; e < N * N; ++e) {
                    const double2 b = opB[c * N * N + e];
                    P.re[e] = fma(a, b.x, P.re[e]);
                    P.im[e] = fma(a, b.y, P.im[e]);
                }
            }
            rmul_acc(D[d], P, X);
        }
    }
}

// The same slice in the exact derivative mode (GRAPE_TRAJ_EXACT):  D_d <- P D_d + E_d X,  X <- P X  with E_d = DF_t[V_d] from
// traj_frechet_dir_kernel (image d of traj_w, ws apart) and X the state BEFORE the slice.  P is loaded a second time behind
// the E_d (from L2) instead of kept: one n x n block live next to X and the D_d, as in the first-order step.
template <int N, int C, int DB>
GRAPE_DEV void jvp_step_exact(CRect<N, C> &X, CRect<N, C> (&D)[DB], int nd, const double2 *__restrict__ Pt,
                              const double2 *__restrict__ Et, size_t ws, size_t stride)
{
    CMat<N> P;
    rc_load_mat(P, Pt, stride);
#pragma unroll
    for (int d = 0; d < DB; ++d)
        if (d < nd)
            rmul_inplace(D[d], P);
#pragma unroll
    for (int d = 0; d < DB; ++d) {
        if (d < nd) {
            rc_load_mat(P, Et + (size_t)d * ws, stride);
            rmul_acc(D[d], P, X);
        }
    }
    rc_load_mat(P, Pt, stride);
    rmul_inplace(X, P);
}

// ops_all / o_all are separate `const __restrict__` arguments so that the wave-uniform operator and probe entries can be
// fetched with scalar loads (as in vjp.hip).  EXACT: the instance of the exact derivative mode, which consumes the E_t that
// traj_frechet_dir_kernel left chunk-major in SweepParams::traj_w (xdot is not read there).
// DB tangents ride next to ONE state walk; nd <= DB of them are live in a launch (the ragged last block).  nd is uniform over
// the grid, so the guards are scalar branches.  DB = 1 is the single call (trajectory_jvp_kernel; bound to RcTraits<N>::MAXT
// threads): its one direction is live by construction, every guard is a compile-time constant, and it reads neither jvp_ndir
// nor the jvp_dir_* strides.
template <int N, int M, int MAXT, int DB, bool EXACT = false>
__global__ __launch_bounds__(MAXT) void trajectory_jvp_kernel(const double2 *__restrict__ ops_all,
                                                              const double2 *__restrict__ o_all,
                                                              const double *__restrict__ xdot, const SweepParams p)
{
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    __shared__ double2 s_q[MAXW][NN];              // wave totals: prefix products, then the affine maps' matrices ...
    __shared__ double2 s_v[MAXW][DB][NM];          // ... and their offsets, one per direction

    const int K = p.K, Nsl = p.N, n_obs = p.jvp_ydot ? p.jvp_n : 0;
    const int nd = DB == 1 ? 1 : p.jvp_ndir;         // live directions of this launch, 1..DB
    // direction d's arrays lie d strides behind direction 0's (DB = 1: there is no other direction, the fields are not read)
    const size_t xs = DB == 1 ? 0 : (size_t)p.jvp_dir_xdot, ys = DB == 1 ? 0 : (size_t)p.jvp_dir_ydot;
    const size_t fs = DB == 1 ? 0 : (size_t)p.jvp_dir_xf, ws = DB == 1 ? 0 : (size_t)p.jvp_dir_w;
    const int k = blockIdx.x;                        // member within the launch: row of the workspace
    const int kg = k + p.jvp_E0;                     // member of the ensemble: row of the probes and of the outputs
    const TrajLane<N> ln = traj_lane<N>(p.jvp_CH, p.S, Nsl, p.props, k);
    const int L = ln.L, lo = ln.lo, cnt = ln.cnt;
    const size_t stride = ln.stride;
    const TrajOps op = traj_ops<N>(ops_all, k, K);
    const TrajProbes pr = traj_probes<N, M>(o_all, p.jvp_per_member, p.jvp_Etot, kg, Nsl);
    double2 *__restrict__ yk = p.jvp_ydot ? p.jvp_ydot + (size_t)kg * p.jvp_n * pr.y_step : nullptr;
    const double *__restrict__ xd = xdot + (size_t)lo * K;        // direction 0 (never read by a lane without a slice)
    const double2 *__restrict__ Ew = EXACT ? ln.template ws<NN>(p.traj_w) : nullptr;

    // ---------------------------------------------------------------- 1: chunk product, and its tangent per direction
    CMat<N> Q;
    CRect<N, N> Rdot[DB];
    {
        CRect<N, N> R;
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            R.re[e] = ((e % N) == (e / N)) ? 1.0 : 0.0;
            R.im[e] = 0.0;
        }
#pragma unroll
        for (int d = 0; d < DB; ++d)
            rzero(Rdot[d]);
#pragma unroll 1
        for (int jj = 0; jj < cnt; ++jj) {
            if constexpr (EXACT)
                jvp_step_exact(R, Rdot, nd, ln.P(jj), Ew + (size_t)jj * NN * stride, ws, stride);
            else
                jvp_step(R, Rdot, nd, ln.P(jj), stride, xd + (size_t)jj * K, xs, op.opB, K);
        }
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            Q.re[e] = R.re[e];
            Q.im[e] = R.im[e];
        }
    }
    // ---------------------------------------------------------------- 2: exclusive prefix over lanes -> X at the chunk start, d_c
    CRect<N, M> Xlo, dvec[DB];
    {
        CMat<N> U;
        traj_prefix_start(U, Q, ln, s_q);
        traj_start_state(Xlo, U, op.opXi);
#pragma unroll
        for (int d = 0; d < DB; ++d) {
            if (d < nd) {
                CMat<N> Rd;
#pragma unroll
                for (int e = 0; e < NN; ++e) {
                    Rd.re[e] = Rdot[d].re[e];
                    Rd.im[e] = Rdot[d].im[e];
                }
                rmul(dvec[d], Rd, Xlo);
            } else {
                rzero(dvec[d]);
            }
        }
    }
    // ---------------------------------------------------------------- 3: exclusive prefix scan of (Q, d_0 .. d_nd-1)
    // (the forward twin of traj_affine_suffix; written out here, its one user: traj_chunk.hpp says why)
    CRect<N, M> Din[DB];
    {
        const int lane = ln.lane, wave = ln.wave, W = ln.W;
        CMat<N> G = Q, Go, T;
        CRect<N, M> vo, Tm;
        for (int s = 1; s < 64; s <<= 1) {           // (L-2s, L-s] then (L-s, L]:  (G Go) z + (G vo + v)
#pragma unroll
            for (int d = 0; d < DB; ++d) {           // (the offsets first, each with the old G: vo is dead before Go lives)
                if (d < nd) {
                    rshfl_up(vo, dvec[d], s);
                    if (lane >= s)
                        rmul_acc(dvec[d], G, vo);
                }
            }
            shfl_up(Go, G, s);
            if (lane >= s) {
                mul(T, G, Go);
                G = T;
            }
        }
        shfl_up(Go, G, 1);                           // the lanes in front of this one, inside the wave
        if (lane == 0)
            set_identity(Go);
        if (W > 1) {
            __syncthreads();                         // (the readers of the prefix totals in s_q are done)
            if (lane == 63) {
#pragma unroll
                for (int e = 0; e < NN; ++e)
                    s_q[wave][e] = make_double2(G.re[e], G.im[e]);
#pragma unroll
                for (int d = 0; d < DB; ++d)
                    if (d < nd) {
#pragma unroll
                        for (int e = 0; e < NM; ++e)
                            s_v[wave][d][e] = make_double2(dvec[d].re[e], dvec[d].im[e]);
                    }
            }
            __syncthreads();
        }
#pragma unroll
        for (int d = 0; d < DB; ++d) {
            if (d < nd) {
                rshfl_up(vo, dvec[d], 1);
                if (lane == 0)
                    rzero(vo);
                if (W > 1) {
                    CRect<N, M> z;
                    rzero(z);
                    for (int w = 0; w < wave; ++w) { // what enters this wave on the left, first wave first
                        rc_load_lds(G, &s_q[w][0]);
                        rmul(Tm, G, z);
#pragma unroll
                        for (int e = 0; e < NM; ++e) {
                            const double2 vv = s_v[w][d][e];
                            z.re[e] = Tm.re[e] + vv.x;
                            z.im[e] = Tm.im[e] + vv.y;
                        }
                    }
                    rmul(Tm, Go, z);
#pragma unroll
                    for (int e = 0; e < NM; ++e) {
                        Din[d].re[e] = Tm.re[e] + vo.re[e];
                        Din[d].im[e] = Tm.im[e] + vo.im[e];
                    }
                } else {
                    Din[d] = vo;
                }
            } else {
                rzero(Din[d]);
            }
        }
    }
    // ---------------------------------------------------------------- 4: the true tangents, the traces
    if (yk && L == 0) {                              // row 0: D_0 = 0
        for (int d = 0; d < nd; ++d)
            for (int j = 0; j < n_obs; ++j)
                yk[(size_t)d * ys + (size_t)j * pr.y_step] = make_double2(0.0, 0.0);
    }
#pragma unroll 1
    for (int jj = 0; jj < cnt; ++jj) {
        const int t = lo + jj;                       // slice index; the state and the tangents behind it are X_{t+1}, D_{t+1}
        if constexpr (EXACT)
            jvp_step_exact(Xlo, Din, nd, ln.P(jj), Ew + (size_t)jj * NN * stride, ws, stride);
        else
            jvp_step(Xlo, Din, nd, ln.P(jj), stride, xd + (size_t)jj * K, xs, op.opB, K);
#pragma unroll
        for (int d = 0; d < DB; ++d) {
            if (d < nd) {
                double2 *__restrict__ yd = yk + (size_t)d * ys;
#pragma unroll 1
                for (int j = 0; j < n_obs; ++j)      // ydot_j = tr(O_j' D_d), one probe at a time
                    yd[(size_t)(t + 1) + (size_t)j * pr.y_step] = traj_probe_trace(pr.probe(j), Din[d]);
                if (p.jvp_xf && t + 1 == Nsl) {
                    double2 *__restrict__ xf = p.jvp_xf + (size_t)d * fs + (size_t)kg * NM;
#pragma unroll
                    for (int e = 0; e < NM; ++e)
                        xf[e] = make_double2(Din[d].re[e], Din[d].im[e]);
                }
            }
        }
    }
}

// what every launch of the kernel above requires; threads is the workgroup size of the decomposition
template <int N>
static bool jvp_launch_ok(const SweepParams &p, int threads)
{
    return !(threads > RcTraits<N>::MAXT || p.jvp_CH < 1 || (long long)p.S * p.jvp_CH < p.N || p.N < 1 || p.E < 1 || p.K < 1 ||
             p.jvp_E0 < 0 || p.jvp_E0 + p.E > p.jvp_Etot || p.jvp_n < 0 || p.jvp_n > 16 || (!p.jvp_ydot && !p.jvp_xf) ||
             (p.jvp_ydot && (p.jvp_n < 1 || !p.jvp_O)) || !p.jvp_xdot || !p.props || !p.ops ||
             (long long)p.K * p.N > 0x7fffff00ll || (p.traj_exact && (!p.traj_w || !p.traj_x)));
}

// the single call: the DB = 1 instance
template <int N, int M>
static hipError_t jvp_launch_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = RcTraits<N>::MAXT;
    const int threads = (p.jvp_CH + 63) & ~63;
    if (!jvp_launch_ok<N>(p, threads))
        return hipErrorInvalidConfiguration;
    if (p.traj_exact) {
        // the exact derivative mode: E_t = DF_t[V_t] per (member, slice) into traj_w, then the instance that consumes it
        const hipError_t e = run_traj_frechet(N, true, p, stream);
        if (e != hipSuccess)
            return e;
        GRAPE_LAUNCH_AS("trajectory_jvp_exact_kernel", (trajectory_jvp_kernel<N, M, MAXT, 1, true>), dim3(p.E), dim3(threads), 0,
                        stream, p.ops, p.jvp_O, p.jvp_xdot, p);
        return hipGetLastError();
    }
    GRAPE_LAUNCH_AS("trajectory_jvp_kernel", (trajectory_jvp_kernel<N, M, MAXT, 1>), dim3(p.E), dim3(threads), 0, stream, p.ops,
                    p.jvp_O, p.jvp_xdot, p);
    return hipGetLastError();
}

// direction d0 of a multi-direction launch as a launch of its own (nd directions from there on)
static SweepParams jvp_direction(const SweepParams &p, int d0, int nd)
{
    SweepParams q = p;
    q.jvp_ndir = nd;
    q.jvp_xdot = p.jvp_xdot + (size_t)d0 * p.jvp_dir_xdot;
    if (p.jvp_ydot) q.jvp_ydot = p.jvp_ydot + (size_t)d0 * p.jvp_dir_ydot;
    if (p.jvp_xf) q.jvp_xf = p.jvp_xf + (size_t)d0 * p.jvp_dir_xf;
    return q;
}

// grape_eval_jvp_multi: p.jvp_ndir directions in blocks of DB through the multi instance (trajectory_jvp_multi_kernel), or (no
// instance for this launch, or not asked for) one behind the other through the DB = 1 instance -- the same bits either way
template <int N, int M>
static hipError_t jvp_launch_multi_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int DB = jvp_multi_block(N, M), MAXT = kJvpMultiMaxThreads;
    const int threads = (p.jvp_CH + 63) & ~63, ndir = p.jvp_ndir;
    if (ndir < 1 || ndir > 64 || p.jvp_dir_xdot < 0 || p.jvp_dir_ydot < 0 || p.jvp_dir_xf < 0 || p.jvp_dir_w < 0 || !p.jvp_xdot)
        return hipErrorInvalidConfiguration;
    if (!p.jvp_multi || threads > MAXT) {
        for (int d = 0; d < ndir; ++d) {
            const hipError_t e = jvp_launch_nm<N, M>(jvp_direction(p, d, 0), stream);
            if (e != hipSuccess)
                return e;
        }
        return hipSuccess;
    }
    if (!jvp_launch_ok<N>(p, threads))
        return hipErrorInvalidConfiguration;
    // a block of ONE direction (n_dir = 1, or the ragged remainder) measured slower through the multi kernel than through the
    // single one, but for n = 4 in the exact mode: it takes the single kernel unless the multi kernel is forced (jvp_multi = 2)
    const bool lone_single = p.jvp_multi == 1 && !(N == 4 && p.traj_exact);
    for (int d0 = 0; d0 < ndir; d0 += DB) {
        const SweepParams q = jvp_direction(p, d0, ndir - d0 < DB ? ndir - d0 : DB);
        if (q.jvp_ndir == 1 && lone_single) {
            const hipError_t e = jvp_launch_nm<N, M>(jvp_direction(q, 0, 0), stream);
            if (e != hipSuccess)
                return e;
            continue;
        }
        if (p.traj_exact) {
            // E_t = DF_t[V_t] of every direction of the block into its own image of traj_w, then the instance that consumes them
            for (int d = 0; d < q.jvp_ndir; ++d) {
                SweepParams r = jvp_direction(q, d, 0);
                r.traj_w = q.traj_w + (size_t)d * q.jvp_dir_w;
                const hipError_t e = run_traj_frechet(N, true, r, stream);
                if (e != hipSuccess)
                    return e;
            }
            GRAPE_LAUNCH_AS("trajectory_jvp_multi_exact_kernel", (trajectory_jvp_kernel<N, M, MAXT, DB, true>), dim3(q.E),
                            dim3(threads), 0, stream, q.ops, q.jvp_O, q.jvp_xdot, q);
        } else {
            GRAPE_LAUNCH_AS("trajectory_jvp_multi_kernel", (trajectory_jvp_kernel<N, M, MAXT, DB>), dim3(q.E), dim3(threads), 0,
                            stream, q.ops, q.jvp_O, q.jvp_xdot, q);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

hipError_t run_trajectory_jvp(int n, const SweepParams &p, hipStream_t stream)
{
    return dispatch_nm(n, p.jvp_m, [&](auto N, auto M) {
        constexpr int Nn = decltype(N)::value, Mm = decltype(M)::value;
        return p.jvp_ndir > 0 ? jvp_launch_multi_nm<Nn, Mm>(p, stream) : jvp_launch_nm<Nn, Mm>(p, stream);
    });
}

}  // namespace grape
