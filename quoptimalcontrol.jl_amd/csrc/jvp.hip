// jvp.hip -- the Jacobian-vector product of the trajectory read-out (grape_eval_jvp; the forward-mode twin of grape_eval_vjp)
// for the small-n family (n = 2, 3, 4; n x m states under left multiplication, UnitaryGate) on gfx950.
//
//   the caller's direction xdot (K, N) in the PHYSICAL pulse's coordinates (the host layer has applied the pulse map's tangent)
//   V_t = sum_c xdot[c,t] B'_{k,c} ,   B' = -i dt B  (first order in dt: grape_eval_vjp's rule, its exact transpose)
//   D_{k,0} = 0 ,   D_{k,t+1} = P_{k,t} D_{k,t} + V_t X_{k,t+1} ,   X_{k,t+1} = P_{k,t} X_{k,t}
//   ydot[s, j, k] = tr(O_kj' D_{k,s}) ,  s = 0..N  (row 0 is zero and written) ,   Xdot_final_k = D_{k,N}
//
// It runs behind the sweep of the same launch and reads the propagators P_t that sweep left in the workspace (chunk-major:
// element e of slice t = c S + jj of member k at ((k S + jj) n^2 + e) CH + c).  The decomposition is trajectory_vjp_kernel's:
// one workgroup per member of the launch, one lane per time chunk of S consecutive slices, every workspace access
// lane-contiguous:
//   1  ONE forward walk over the chunk in relative form, carrying R = P_t ... P_lo (from 1) and its tangent Rdot (from 0),
//      Rdot <- P Rdot + V_t R_{t+1}: the chunk product Q_c = R and, with the state at the chunk start, the chunk's own
//      contribution d_c = Rdot X_lo to the tangent that leaves it on the right -- the chunk product and the walk from D = 0
//      of the pull-back's decomposition in one pass over the propagators, with two n x n blocks live next to P and V
//      (a walk on X and D would keep Q and X_lo alive across the loop: six blocks, and scratch traffic in it at n = m = 3)
//   2  exclusive prefix scan of the Q_c over lanes (wave shuffles, wave totals through LDS): X at the chunk start, d_c
//   3  exclusive prefix scan of the affine maps z -> Q_c z + d_c over lanes, composition (Q2 Q1, Q2 d1 + d2) in a fixed tree:
//      the forward twin of the pull-back's suffix scan
//   4  the walk on X and D from the true incoming tangent: D_t+1 behind every slice and its n_obs traces, D_N on slice N - 1
// The states are walked forward WITH the tangent in both walks (X_t+1 is what V_t multiplies), so neither flow stores states
// and one instance serves unitary and non-unitary propagators.  The probes are wave-uniform (scalar loads); xdot is read in
// the caller's layout (a lane's chunk is K S consecutive doubles).
// Ragged decompositions: a lane whose chunk starts at or behind N owns no slice (Q = 1, d = 0), the last chunk may be short.
// Members are independent: no sum over members, plain vector stores, every number has one fixed evaluation order, so a
// member-chunked launch sequence gives the bits of an unchunked one.  Every operation is linear in xdot (products and FMAs
// whose addends all carry one factor of it): 2 xdot gives twice the bits, -xdot the negated ones, 0 gives 0.
//
// The ydot stores are observe_kernel's direct ones (lane c stores at s = c S + jj: neighbouring lanes S 16 B apart in a probe
// row); there is no staged instance.
//
// grape_eval_jvp_multi: trajectory_jvp_multi_kernel<N, M, MAXT, DB, EXACT> carries DB tangents through the same four steps next
// to ONE chunk product, ONE scan of Q and ONE state walk -- R once and Rdot per direction in step 1, the affine scan with one
// matrix part and an offset per direction, X once and D per direction in step 4 -- so the propagators are read once per pass
// for the block.  Per direction the operations and their order are this kernel's: block d holds the single call's bits.  It is
// bound to 256 threads for every n (one wave per SIMD, 512 registers per lane); DB per (n, m) is jvp_multi_block.
#include "cmat.hpp"
#include "grape_kernels.hpp"
#include "rc_mat.hpp"

namespace grape {

template <int N, int M>
GRAPE_DEV void rshfl_up(CRect<N, M> &dst, const CRect<N, M> &src, int delta)
{
#pragma unroll
    for (int e = 0; e < N * M; ++e) {
        dst.re[e] = __shfl_up(src.re[e], delta, 64);
        dst.im[e] = __shfl_up(src.im[e], delta, 64);
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

// one slice of the tangent recurrence on an n x c block pair:  X <- P X,  D <- P D + V X  with  V = sum_c xd[c] B'_c
// (opB: the member's K prescaled control operators, wave-uniform; V is built in the registers P has left)
template <int N, int C>
GRAPE_DEV void jvp_step(CRect<N, C> &X, CRect<N, C> &D, const double2 *__restrict__ Pt, size_t stride,
                        const double *__restrict__ xd, const double2 *__restrict__ opB, int K)
{
    CMat<N> P;
    rc_load_mat(P, Pt, stride);
    rmul_inplace(X, P);
    rmul_inplace(D, P);
#pragma unroll
    for (int e = 0; e < N * N; ++e) {
        P.re[e] = 0.0;
        P.im[e] = 0.0;
    }
#pragma unroll 1
    for (int c = 0; c < K; ++c) {
        const double a = xd[c];
#pragma unroll
        for (int e = 0; e < N * N; ++e) {
            const double2 b = opB[c * N * N + e];
            P.re[e] = fma(a, b.x, P.re[e]);
            P.im[e] = fma(a, b.y, P.im[e]);
        }
    }
    rmul_acc(D, P, X);
}

// The same slice in the exact derivative mode (GRAPE_TRAJ_EXACT):  D <- P D + E_t X,  X <- P X  with E_t = DF_t[V_t] from
// traj_frechet_dir_kernel and X the state BEFORE the slice.  P is loaded a second time behind E_t (from L2) instead of
// kept: one n x n block live next to X and D, as in the first-order step.
template <int N, int C>
GRAPE_DEV void jvp_step_exact(CRect<N, C> &X, CRect<N, C> &D, const double2 *__restrict__ Pt, const double2 *__restrict__ Et,
                              size_t stride)
{
    CMat<N> P;
    rc_load_mat(P, Pt, stride);
    rmul_inplace(D, P);
    rc_load_mat(P, Et, stride);
    rmul_acc(D, P, X);
    rc_load_mat(P, Pt, stride);
    rmul_inplace(X, P);
}

// ops_all / o_all are separate `const __restrict__` arguments so that the wave-uniform operator and probe entries can be
// fetched with scalar loads (as in vjp.hip).  EXACT: the instance of the exact derivative mode, which consumes the E_t that
// traj_frechet_dir_kernel left chunk-major in SweepParams::traj_w (xdot is not read here).
template <int N, int M, int MAXT, bool EXACT = false>
__global__ __launch_bounds__(MAXT) void trajectory_jvp_kernel(const double2 *__restrict__ ops_all,
                                                              const double2 *__restrict__ o_all,
                                                              const double *__restrict__ xdot, const SweepParams p)
{
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    __shared__ double2 s_q[MAXW][NN];              // wave totals: prefix products, then the affine maps' matrices ...
    __shared__ double2 s_v[MAXW][NM];              // ... and their offsets

    const int CH = p.jvp_CH, S = p.S, K = p.K, Nsl = p.N, n_obs = p.jvp_ydot ? p.jvp_n : 0;
    const int L = threadIdx.x, lane = L & 63;
    const int wave = __builtin_amdgcn_readfirstlane(L >> 6), W = blockDim.x >> 6;
    const int k = blockIdx.x;                        // member within the launch: row of the workspace
    const int kg = k + p.jvp_E0;                     // member of the ensemble: row of the probes and of the outputs
    // the lane's slices [lo, hi): none for chunks that start at or behind N and for the padding lanes behind chunk CH - 1
    const int lo = (L < CH && L * S < Nsl) ? L * S : Nsl;
    const int hi = min(lo + S, Nsl);
    const int cnt = hi - lo;
    const size_t stride = (size_t)CH;
    const double2 *__restrict__ Pw = p.props + (size_t)k * S * NN * stride + L;
    const double2 *__restrict__ ops = ops_all + (size_t)k * (K + 3) * NN;
    const double2 *__restrict__ opB = ops + NN;
    const double2 *__restrict__ opXi = ops + (size_t)(1 + K) * NN;
    // probe j of this member: shared (n, m, n_obs) or per member (n, m, Etot, n_obs)
    const size_t o_step = p.jvp_per_member ? (size_t)p.jvp_Etot * NM : (size_t)NM;
    const double2 *__restrict__ o_mem = o_all + (p.jvp_per_member ? (size_t)kg * NM : (size_t)0);
    const size_t y_step = (size_t)Nsl + 1;
    double2 *__restrict__ yk = p.jvp_ydot ? p.jvp_ydot + (size_t)kg * p.jvp_n * y_step : nullptr;
    const double *__restrict__ xd = xdot + (size_t)lo * K;        // (never read by a lane without a slice)
    const double2 *__restrict__ Ew = EXACT ? p.traj_w + (size_t)k * S * NN * stride + L : nullptr;

    // ---------------------------------------------------------------- 1: chunk product and its tangent, relative to the chunk start
    CMat<N> Q, T;
    CRect<N, N> Rdot;
    {
        CRect<N, N> R;
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            R.re[e] = ((e % N) == (e / N)) ? 1.0 : 0.0;
            R.im[e] = 0.0;
        }
        rzero(Rdot);
#pragma unroll 1
        for (int jj = 0; jj < cnt; ++jj) {
            if constexpr (EXACT)
                jvp_step_exact(R, Rdot, Pw + (size_t)jj * NN * stride, Ew + (size_t)jj * NN * stride, stride);
            else
                jvp_step(R, Rdot, Pw + (size_t)jj * NN * stride, stride, xd + (size_t)jj * K, opB, K);
        }
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            Q.re[e] = R.re[e];
            Q.im[e] = R.im[e];
        }
    }
    // ---------------------------------------------------------------- 2: exclusive prefix over lanes -> X at the chunk start, d_c
    CRect<N, M> Xlo, dvec;
    {
        CMat<N> inc = Q, oth;
        for (int d = 1; d < 64; d <<= 1) {
            shfl_up(oth, inc, d);
            if (lane >= d) {
                mul(T, inc, oth);
                inc = T;
            }
        }
        shfl_up(oth, inc, 1);
        if (lane == 0)
            set_identity(oth);
        if (W > 1) {
            if (lane == 63) {
#pragma unroll
                for (int e = 0; e < NN; ++e)
                    s_q[wave][e] = make_double2(inc.re[e], inc.im[e]);
            }
            __syncthreads();
            CMat<N> pre;
            set_identity(pre);
            for (int w = 0; w < wave; ++w) {
                rc_load_lds(inc, &s_q[w][0]);
                mul(T, inc, pre);
                pre = T;
            }
            mul(T, oth, pre);
            oth = T;
        }
        CRect<N, M> xi;
        rload_uniform(xi, opXi);                     // (the first m columns of the zero-padded n x n block)
        rmul(Xlo, oth, xi);
        CMat<N> Rd;
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            Rd.re[e] = Rdot.re[e];
            Rd.im[e] = Rdot.im[e];
        }
        rmul(dvec, Rd, Xlo);
    }

    // the n_obs traces ydot_j = tr(O_j' D) of the tangent behind s slices, one probe at a time
    auto emit_y = [&](const CRect<N, M> &D, int s) {
#pragma unroll 1
        for (int j = 0; j < n_obs; ++j) {
            const double2 *__restrict__ o = o_mem + (size_t)j * o_step;
            double yr = 0.0, yi = 0.0;
#pragma unroll
            for (int e = 0; e < NM; ++e) {
                const double2 v = o[e];
                yr = fma(v.x, D.re[e], yr);
                yr = fma(v.y, D.im[e], yr);
                yi = fma(v.x, D.im[e], yi);
                yi = fma(-v.y, D.re[e], yi);
            }
            yk[(size_t)s + (size_t)j * y_step] = make_double2(yr, yi);
        }
    };
    // ---------------------------------------------------------------- 3: exclusive prefix scan of (Q, d)
    CRect<N, M> Din;
    {
        CMat<N> G = Q, Go;
        CRect<N, M> v = dvec, vo, Tm;
        for (int d = 1; d < 64; d <<= 1) {           // (L-2d, L-d] then (L-d, L]:  (G Go) z + (G vo + v)
            rshfl_up(vo, v, d);                      // (the offset first, with the old G: vo is dead before Go lives)
            if (lane >= d)
                rmul_acc(v, G, vo);
            shfl_up(Go, G, d);
            if (lane >= d) {
                mul(T, G, Go);
                G = T;
            }
        }
        shfl_up(Go, G, 1);                           // the lanes in front of this one, inside the wave
        rshfl_up(vo, v, 1);
        if (lane == 0) {
            set_identity(Go);
            rzero(vo);
        }
        if (W > 1) {
            __syncthreads();                         // (the readers of the prefix totals in s_q are done)
            if (lane == 63) {
#pragma unroll
                for (int e = 0; e < NN; ++e)
                    s_q[wave][e] = make_double2(G.re[e], G.im[e]);
#pragma unroll
                for (int e = 0; e < NM; ++e)
                    s_v[wave][e] = make_double2(v.re[e], v.im[e]);
            }
            __syncthreads();
            CRect<N, M> z;
            rzero(z);
            for (int w = 0; w < wave; ++w) {         // what enters this wave on the left, first wave first
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
                Din.re[e] = Tm.re[e] + vo.re[e];
                Din.im[e] = Tm.im[e] + vo.im[e];
            }
        } else {
            Din = vo;
        }
    }
    // ---------------------------------------------------------------- 4: the true tangents, the traces
    if (yk && L == 0) {                              // row 0: D_0 = 0
        for (int j = 0; j < n_obs; ++j)
            yk[(size_t)j * y_step] = make_double2(0.0, 0.0);
    }
#pragma unroll 1
    for (int jj = 0; jj < cnt; ++jj) {
        const int t = lo + jj;                       // slice index; the state and the tangent behind it are X_{t+1}, D_{t+1}
        if constexpr (EXACT)
            jvp_step_exact(Xlo, Din, Pw + (size_t)jj * NN * stride, Ew + (size_t)jj * NN * stride, stride);
        else
            jvp_step(Xlo, Din, Pw + (size_t)jj * NN * stride, stride, xd + (size_t)jj * K, opB, K);
        emit_y(Din, t + 1);
        if (p.jvp_xf && t + 1 == Nsl) {
            double2 *__restrict__ xf = p.jvp_xf + (size_t)kg * NM;
#pragma unroll
            for (int e = 0; e < NM; ++e)
                xf[e] = make_double2(Din.re[e], Din.im[e]);
        }
    }
}

// ---- several directions per call (grape_eval_jvp_multi) -----------------------------------------------------------------------
// trajectory_jvp_multi_kernel carries up to DB tangents next to ONE state walk: the propagators, the chunk products, the
// prefix scan of Q and the walk of X are the block's, the tangents are each direction's.  Per direction every operation and
// its order is trajectory_jvp_kernel's (the same inlined products, V_t built from zero in the registers P has left, one
// direction after the other), so block d of the result is bit for bit the single kernel's for direction d alone.  nd <= DB
// directions are live in a launch (the ragged last block); nd is uniform over the grid, so the guards are scalar branches.

// one slice for the block:  X <- P X,  D_d <- P D_d + V_d X  (direction d's xdot row at xd + d xs)
template <int N, int C, int DB>
GRAPE_DEV void jvp_step_multi(CRect<N, C> &X, CRect<N, C> (&D)[DB], int nd, const double2 *__restrict__ Pt, size_t stride,
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

// the exact derivative mode:  D_d <- P D_d + E_d X  with X the state BEFORE the slice, then X <- P X  (E_d: image d of traj_w)
template <int N, int C, int DB>
GRAPE_DEV void jvp_step_multi_exact(CRect<N, C> &X, CRect<N, C> (&D)[DB], int nd, const double2 *__restrict__ Pt,
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

template <int N, int M, int MAXT, int DB, bool EXACT = false>
__global__ __launch_bounds__(MAXT) void trajectory_jvp_multi_kernel(const double2 *__restrict__ ops_all,
                                                                    const double2 *__restrict__ o_all,
                                                                    const double *__restrict__ xdot, const SweepParams p)
{
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    __shared__ double2 s_q[MAXW][NN];              // wave totals: prefix products, then the affine maps' matrices ...
    __shared__ double2 s_v[MAXW][DB][NM];          // ... and their offsets, one per direction

    const int CH = p.jvp_CH, S = p.S, K = p.K, Nsl = p.N, n_obs = p.jvp_ydot ? p.jvp_n : 0;
    const int nd = p.jvp_ndir;                       // live directions of this launch, 1..DB
    const size_t xs = (size_t)p.jvp_dir_xdot, ys = (size_t)p.jvp_dir_ydot, fs = (size_t)p.jvp_dir_xf, ws = (size_t)p.jvp_dir_w;
    const int L = threadIdx.x, lane = L & 63;
    const int wave = __builtin_amdgcn_readfirstlane(L >> 6), W = blockDim.x >> 6;
    const int k = blockIdx.x;
    const int kg = k + p.jvp_E0;
    const int lo = (L < CH && L * S < Nsl) ? L * S : Nsl;
    const int hi = min(lo + S, Nsl);
    const int cnt = hi - lo;
    const size_t stride = (size_t)CH;
    const double2 *__restrict__ Pw = p.props + (size_t)k * S * NN * stride + L;
    const double2 *__restrict__ ops = ops_all + (size_t)k * (K + 3) * NN;
    const double2 *__restrict__ opB = ops + NN;
    const double2 *__restrict__ opXi = ops + (size_t)(1 + K) * NN;
    const size_t o_step = p.jvp_per_member ? (size_t)p.jvp_Etot * NM : (size_t)NM;
    const double2 *__restrict__ o_mem = o_all + (p.jvp_per_member ? (size_t)kg * NM : (size_t)0);
    const size_t y_step = (size_t)Nsl + 1;
    double2 *__restrict__ yk = p.jvp_ydot ? p.jvp_ydot + (size_t)kg * p.jvp_n * y_step : nullptr;
    const double *__restrict__ xd = xdot + (size_t)lo * K;        // direction 0 (never read by a lane without a slice)
    const double2 *__restrict__ Ew = EXACT ? p.traj_w + (size_t)k * S * NN * stride + L : nullptr;

    // ---------------------------------------------------------------- 1: chunk product, and its tangent per direction
    CMat<N> Q, T;
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
                jvp_step_multi_exact(R, Rdot, nd, Pw + (size_t)jj * NN * stride, Ew + (size_t)jj * NN * stride, ws, stride);
            else
                jvp_step_multi(R, Rdot, nd, Pw + (size_t)jj * NN * stride, stride, xd + (size_t)jj * K, xs, opB, K);
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
        CMat<N> inc = Q, oth;
        for (int d = 1; d < 64; d <<= 1) {
            shfl_up(oth, inc, d);
            if (lane >= d) {
                mul(T, inc, oth);
                inc = T;
            }
        }
        shfl_up(oth, inc, 1);
        if (lane == 0)
            set_identity(oth);
        if (W > 1) {
            if (lane == 63) {
#pragma unroll
                for (int e = 0; e < NN; ++e)
                    s_q[wave][e] = make_double2(inc.re[e], inc.im[e]);
            }
            __syncthreads();
            CMat<N> pre;
            set_identity(pre);
            for (int w = 0; w < wave; ++w) {
                rc_load_lds(inc, &s_q[w][0]);
                mul(T, inc, pre);
                pre = T;
            }
            mul(T, oth, pre);
            oth = T;
        }
        CRect<N, M> xi;
        rload_uniform(xi, opXi);
        rmul(Xlo, oth, xi);
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
    CRect<N, M> Din[DB];
    {
        CMat<N> G = Q, Go;
        CRect<N, M> vo, Tm;
        for (int s = 1; s < 64; s <<= 1) {           // the offsets first, each with the old G, then G itself
#pragma unroll
            for (int d = 0; d < DB; ++d) {
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
                yk[(size_t)d * ys + (size_t)j * y_step] = make_double2(0.0, 0.0);
    }
#pragma unroll 1
    for (int jj = 0; jj < cnt; ++jj) {
        const int t = lo + jj;
        if constexpr (EXACT)
            jvp_step_multi_exact(Xlo, Din, nd, Pw + (size_t)jj * NN * stride, Ew + (size_t)jj * NN * stride, ws, stride);
        else
            jvp_step_multi(Xlo, Din, nd, Pw + (size_t)jj * NN * stride, stride, xd + (size_t)jj * K, xs, opB, K);
#pragma unroll
        for (int d = 0; d < DB; ++d) {
            if (d < nd) {
                double2 *__restrict__ yd = yk + (size_t)d * ys;
#pragma unroll 1
                for (int j = 0; j < n_obs; ++j) {    // ydot_j = tr(O_j' D_d), one probe at a time
                    const double2 *__restrict__ o = o_mem + (size_t)j * o_step;
                    double yr = 0.0, yi = 0.0;
#pragma unroll
                    for (int e = 0; e < NM; ++e) {
                        const double2 v = o[e];
                        yr = fma(v.x, Din[d].re[e], yr);
                        yr = fma(v.y, Din[d].im[e], yr);
                        yi = fma(v.x, Din[d].im[e], yi);
                        yi = fma(-v.y, Din[d].re[e], yi);
                    }
                    yd[(size_t)(t + 1) + (size_t)j * y_step] = make_double2(yr, yi);
                }
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

template <int N, int M>
static hipError_t jvp_launch_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = RcTraits<N>::MAXT;
    const int threads = (p.jvp_CH + 63) & ~63;
    if (threads > MAXT || p.jvp_CH < 1 || (long long)p.S * p.jvp_CH < p.N || p.N < 1 || p.E < 1 || p.K < 1 || p.jvp_E0 < 0 ||
        p.jvp_E0 + p.E > p.jvp_Etot || p.jvp_n < 0 || p.jvp_n > 16 || (!p.jvp_ydot && !p.jvp_xf) ||
        (p.jvp_ydot && (p.jvp_n < 1 || !p.jvp_O)) || !p.jvp_xdot || !p.props || !p.ops || (long long)p.K * p.N > 0x7fffff00ll)
        return hipErrorInvalidConfiguration;
    if (p.traj_exact) {
        // the exact derivative mode: E_t = DF_t[V_t] per (member, slice) into traj_w, then the instance that consumes it
        if (!p.traj_w || !p.traj_x)
            return hipErrorInvalidConfiguration;
        const hipError_t e = run_traj_frechet(N, true, p, stream);
        if (e != hipSuccess)
            return e;
        GRAPE_LAUNCH_AS("trajectory_jvp_exact_kernel", (trajectory_jvp_kernel<N, M, MAXT, true>), dim3(p.E), dim3(threads), 0, stream,
                        p.ops, p.jvp_O, p.jvp_xdot, p);
        return hipGetLastError();
    }
    GRAPE_LAUNCH_AS("trajectory_jvp_kernel", (trajectory_jvp_kernel<N, M, MAXT>), dim3(p.E), dim3(threads), 0, stream, p.ops, p.jvp_O,
                    p.jvp_xdot, p);
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

// grape_eval_jvp_multi: p.jvp_ndir directions in blocks of DB through trajectory_jvp_multi_kernel, or (no instance for this
// launch, or not asked for) one behind the other through trajectory_jvp_kernel -- the same bits either way
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
    if (threads > RcTraits<N>::MAXT || p.jvp_CH < 1 || (long long)p.S * p.jvp_CH < p.N || p.N < 1 || p.E < 1 || p.K < 1 || p.jvp_E0 < 0 ||
        p.jvp_E0 + p.E > p.jvp_Etot || p.jvp_n < 0 || p.jvp_n > 16 || (!p.jvp_ydot && !p.jvp_xf) ||
        (p.jvp_ydot && (p.jvp_n < 1 || !p.jvp_O)) || !p.props || !p.ops || (long long)p.K * p.N > 0x7fffff00ll)
        return hipErrorInvalidConfiguration;
    if (p.traj_exact && (!p.traj_w || !p.traj_x))
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
            GRAPE_LAUNCH_AS("trajectory_jvp_multi_exact_kernel", (trajectory_jvp_multi_kernel<N, M, MAXT, DB, true>), dim3(q.E),
                            dim3(threads), 0, stream, q.ops, q.jvp_O, q.jvp_xdot, q);
        } else {
            GRAPE_LAUNCH_AS("trajectory_jvp_multi_kernel", (trajectory_jvp_multi_kernel<N, M, MAXT, DB>), dim3(q.E), dim3(threads), 0,
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
    if (p.jvp_ndir > 0) {
        switch (n * 8 + p.jvp_m) {
        case 2 * 8 + 1: return jvp_launch_multi_nm<2, 1>(p, stream);
        case 2 * 8 + 2: return jvp_launch_multi_nm<2, 2>(p, stream);
        case 3 * 8 + 1: return jvp_launch_multi_nm<3, 1>(p, stream);
        case 3 * 8 + 2: return jvp_launch_multi_nm<3, 2>(p, stream);
        case 3 * 8 + 3: return jvp_launch_multi_nm<3, 3>(p, stream);
        case 4 * 8 + 1: return jvp_launch_multi_nm<4, 1>(p, stream);
        case 4 * 8 + 2: return jvp_launch_multi_nm<4, 2>(p, stream);
        case 4 * 8 + 3: return jvp_launch_multi_nm<4, 3>(p, stream);
        case 4 * 8 + 4: return jvp_launch_multi_nm<4, 4>(p, stream);
        default: return hipErrorInvalidValue;
        }
    }
    switch (n * 8 + p.jvp_m) {
    case 2 * 8 + 1: return jvp_launch_nm<2, 1>(p, stream);
    case 2 * 8 + 2: return jvp_launch_nm<2, 2>(p, stream);
    case 3 * 8 + 1: return jvp_launch_nm<3, 1>(p, stream);
    case 3 * 8 + 2: return jvp_launch_nm<3, 2>(p, stream);
    case 3 * 8 + 3: return jvp_launch_nm<3, 3>(p, stream);
    case 4 * 8 + 1: return jvp_launch_nm<4, 1>(p, stream);
    case 4 * 8 + 2: return jvp_launch_nm<4, 2>(p, stream);
    case 4 * 8 + 3: return jvp_launch_nm<4, 3>(p, stream);
    case 4 * 8 + 4: return jvp_launch_nm<4, 4>(p, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace grape
