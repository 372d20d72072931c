// running_cost.hip -- running costs on the intermediate states (grape_set_running_cost; the reference's C5 / C6 / C7,
// src/cost_functions.jl:44-61) for the small-n family (n = 2, 3, 4; n x m states under left multiplication) on gfx950.
//
//   J      = sum_k w_k sum_j sum_{s=1..N} rho[s-1,j] |y_{k,j,s}|^2 ,   y_{k,j,s} = tr(R_{k,j}' X_{k,s})
//   dJ/dx[c,t] ~ sum_k w_k sum_j 2 Re tr(Lam_{k,j,t+1}' B'_{k,c} X_{k,t+1}) ,   B' = -i dt B  (first order in dt, as grad_func!)
//   Lam_{j,N} = rho[N-1,j] y_{j,N} R_j ,   Lam_{j,s} = P_s' Lam_{j,s+1} + rho[s-1,j] y_{j,s} R_j
//
// It runs behind the sweep of the same launch and reads the propagators P_t that sweep left in the workspace (chunk-major:
// element e of slice t = c S + jj of member k at ((k S + jj) n^2 + e) CH + c).  One workgroup per (control array, member),
// one lane per time chunk of S consecutive slices -- the sweep's own decomposition, so every workspace access is
// lane-contiguous; the decomposition and the steps marked * are traj_chunk.hpp's, shared with observe.hip, vjp.hip and jvp.hip:
//   1* chunk product Q_c = P_hi-1 ... P_lo                                   (P read once)
//   2* inclusive/exclusive prefix scan of the Q_c over lanes (wave shuffles, wave totals through LDS): X at the chunk start
//   3  the states of the chunk: unitary flow (every generator Hermitian): only X at the chunk END = Q_c X_start is kept and
//      the walks below step back with X_s = P_s' X_s+1; general flow: a forward walk* stores X_s+1 per slice in a scratch
//      array of the chunk-major layout (there is no P' to walk back with)
//   then per term j (the recurrences of different terms share nothing but P and X):
//   4  backward walk from Lam = 0: b_c, the chunk's own contribution to the costate that leaves it on the left
//   5* suffix scan of the affine maps z -> Q_c' z + b_c over lanes, composition (Q1' Q2', Q1' b2 + b1) in a fixed tree
//      (shuffles inside a wave, wave totals through LDS, combined last wave first)
//   6  the same backward walk from the true incoming costate: Lam_t+1 at every slice, M = X_t+1 Lam_t+1', and the K traces
//      2 Re tr(B'_c M) weighted by w_k -- stored to (term 0) or added to (later terms; same lane, program order) the
//      member's row
// The traces above are the FIRST-ORDER rule.  grape_set_running_cost_derivative(GRAPE_TRAJ_EXACT) replaces them with
//   dJ/dx[c,t] = sum_k w_k 2 Re tr( DF_t[W_{k,t}] B'_kc ) ,   W_{k,t} = X_{k,t} sum_j Lam_{k,j,t+1}'
// DF_t the Frechet derivative of the map the sweep evaluated (frechet.hpp): the EXACT instance below + traj_frechet.hip.
// Ragged decompositions: a lane whose chunk starts at or behind N owns no slice (Q = 1, b = 0), the last chunk may be short.
// No atomics, plain vector stores; the fold kernel below adds the members' rows to the sweep's per-workgroup rows in member
// order, so the ensemble sum that follows is the one it always was and results are bitwise reproducible.
#include "cmat.hpp"
#include "grape_kernels.hpp"
#include "rc_mat.hpp"
#include "traj_chunk.hpp"

namespace grape {

// ops_all / r_all / rho / wts_all are separate `const __restrict__` arguments so that the wave-uniform operator, probe and
// weight entries can be fetched with scalar loads (as in sweep_small.hip).  UNI: every propagator is unitary.
// EXACT (grape_set_running_cost_derivative, GRAPE_TRAJ_EXACT; reported as running_cost_exact_kernel): walk 6 stores
// W_t = X_t Lam_{t+1}' (n x n whatever m is; X_t the state BEFORE slice t) chunk-major into SweepParams::traj_w instead of
// forming the K traces -- term 0 stores, later terms add (same lane, program order), so one block per slice carries the sum
// over the terms and ONE Frechet derivative per (member, slice) serves all controls and all terms (the running-cost instance
// of traj_frechet_rows_kernel, behind this kernel, writes the K N gradient entries of the row).  The per-term walks stay:
// J's chain of FMAs is the first-order instance's, bit for bit.  Unitary flow: X_t is at hand after the step back
// X_t = P_t' X_{t+1}; general flow: the forward walk stores the state BEFORE every slice (slot jj: X_{lo+jj}, slot 0 the
// chunk's start state) and the walks carry X_{t+1} = slot jj + 1 (the chunk's end state for the last slice) in registers.
template <int N, int M, bool UNI, int MAXT, bool EXACT = false>
__global__ __launch_bounds__(MAXT) void running_cost_kernel(const double2 *__restrict__ ops_all,
                                                            const double2 *__restrict__ r_all,
                                                            const double *__restrict__ rho,
                                                            const double *__restrict__ wts_all, const SweepParams p)
{
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    __shared__ double2 s_q[MAXW][NN];              // wave totals: prefix products, then the affine maps' matrices ...
    __shared__ double2 s_v[MAXW][NM];              // ... and their offsets
    __shared__ double s_j[MAXW];

    const int K = p.K, Nsl = p.N;
    const int k = blockIdx.x;                        // row of the workspace and of the output: (control array, member)
    const int kl = k % p.E;                          // member within the launch
    const TrajLane<N> ln = traj_lane<N>(p.rc_CH, p.S, Nsl, p.props, k);
    const int L = ln.L, lane = ln.lane, wave = ln.wave, W = ln.W, lo = ln.lo, cnt = ln.cnt;
    const size_t stride = ln.stride;
    double2 *__restrict__ Xw = UNI ? nullptr : ln.template ws<NM>(p.rc_xs);
    const TrajOps op = traj_ops<N>(ops_all, kl, K);
    const double2 *__restrict__ opB = op.opB;
    double *__restrict__ row = p.rc_rows + (size_t)k * ((size_t)K * Nsl + 1);
    const double wk = (EXACT && p.rc_unweighted) ? 1.0 : wts_all[kl];

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

    double jpart = 0.0;
    for (int j = 0; j < p.rc_terms; ++j) {
        CRect<N, M> R;
        rload_uniform(R, r_all + ((size_t)j * p.rc_Etot + kl) * NM);
        const double *__restrict__ rho_j = rho + (size_t)j * Nsl;
        // one backward walk over the chunk from the costate Lam that enters it on the right; EMIT: with the gradient traces
        auto walk = [&](CRect<N, M> &Lam, const bool emit) {
            CRect<N, M> X = Xhi, Tm;
            for (int jj = cnt - 1; jj >= 0; --jj) {
                const int t = lo + jj;               // slice index; the state behind it is X_{t+1}, weighted by rho[t]
                if constexpr (!EXACT) {
                    if (!UNI)
                        rload_ws(X, Xw + (size_t)jj * NM * stride, stride);
                }
                rc_load_mat(P, ln.P(jj), stride);
                double yr = 0.0, yi = 0.0;           // y = tr(R' X)
#pragma unroll
                for (int e = 0; e < NM; ++e) {
                    yr = fma(R.re[e], X.re[e], yr);
                    yr = fma(R.im[e], X.im[e], yr);
                    yi = fma(R.re[e], X.im[e], yi);
                    yi = fma(-R.im[e], X.re[e], yi);
                }
                const double r = rho_j[t];
                const double cr = r * yr, ci = r * yi;
                if (!emit)
                    jpart = fma(r, fma(yr, yr, yi * yi), jpart);
#pragma unroll
                for (int e = 0; e < NM; ++e) {       // Lam_{t+1} = (what came from the right) + rho y R
                    Lam.re[e] = fma(cr, R.re[e], fma(-ci, R.im[e], Lam.re[e]));
                    Lam.im[e] = fma(cr, R.im[e], fma(ci, R.re[e], Lam.im[e]));
                }
                if constexpr (EXACT) {
                    if (UNI) {
                        rmul_ah(Tm, P, X);           // X_t = P_t' X_{t+1}
                        X = Tm;
                    } else {
                        rload_ws(X, Xw + (size_t)jj * NM * stride, stride);
                    }
                    if (emit) {
                        // W_t = X_t Lam_{t+1}' of this term, column by column (rmul_a_bh's sums): a column is stored
                        // (term 0) or added to the block (later terms) before the next one is formed -- the scheduling
                        // barriers keep the whole block and its n^2 loads from being live at once
                        double2 *__restrict__ wp = ln.template slot<NN>(p.traj_w, jj);
#pragma unroll
                        for (int b2 = 0; b2 < N; ++b2) {
                            double wr[N], wi[N];
#pragma unroll
                            for (int a2 = 0; a2 < N; ++a2) {
                                double sr = 0.0, si = 0.0;
#pragma unroll
                                for (int q = 0; q < M; ++q) {
                                    const double ar = X.re[a2 + q * N], ai = X.im[a2 + q * N];
                                    const double br = Lam.re[b2 + q * N], bi = -Lam.im[b2 + q * N];
                                    sr = fma(ar, br, sr);
                                    sr = fma(-ai, bi, sr);
                                    si = fma(ar, bi, si);
                                    si = fma(ai, br, si);
                                }
                                wr[a2] = sr;
                                wi[a2] = si;
                            }
                            if (j == 0) {
#pragma unroll
                                for (int a2 = 0; a2 < N; ++a2)
                                    wp[(a2 + b2 * N) * stride] = make_double2(wr[a2], wi[a2]);
                            } else {
#pragma unroll
                                for (int a2 = 0; a2 < N; ++a2) {
                                    const double2 v = wp[(a2 + b2 * N) * stride];
                                    wp[(a2 + b2 * N) * stride] = make_double2(v.x + wr[a2], v.y + wi[a2]);
                                }
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                } else if (emit) {
                    CMat<N> Mx;
                    rmul_a_bh(Mx, X, Lam);           // X Lam'
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
                        const double g = 2.0 * wk * re;
                        double *dst = row + (size_t)t * K + c;
                        *dst = (j == 0) ? g : *dst + g;
                    }
                }
                rmul_ah(Tm, P, Lam);                 // pull the costate back over slice t
                Lam = Tm;
                if constexpr (!EXACT) {
                    if (UNI) {
                        rmul_ah(Tm, P, X);
                        X = Tm;
                    }
                }
            }
        };
        // ------------------------------------------------------------ 4: the chunk's affine map
        CRect<N, M> bvec;
        rzero(bvec);
        walk(bvec, false);
        // ------------------------------------------------------------ 5: suffix scan of (Q', b)
        CRect<N, M> Lin;
        traj_affine_suffix(Lin, Q, bvec, ln, s_q, s_v);
        // ------------------------------------------------------------ 6: the true costates, the traces
        walk(Lin, true);
    }

    // J of this member: lanes in a fixed butterfly, waves in order
    for (int d = 32; d >= 1; d >>= 1)
        jpart += __shfl_xor(jpart, d, 64);
    if (W > 1)
        __syncthreads();
    if (lane == 0)
        s_j[wave] = jpart;
    __syncthreads();
    if (L == 0) {
        double tot = 0.0;
        for (int w = 0; w < W; ++w)
            tot += s_j[w];
        row[(size_t)K * Nsl] = wk * tot;
    }
}

// block_out[b][q] += sum over the members m of sweep workgroup b, ascending, of rows[member][q]: the running cost joins the
// sweep's weighted per-workgroup rows, and the ensemble reduction behind them stays what it was
__global__ __launch_bounds__(256) void running_cost_fold_kernel(const double *__restrict__ rows, double *__restrict__ block_out,
                                                                int MPB, int E, int BPX, int Q)
{
    const int q = blockIdx.y * 256 + threadIdx.x;
    if (q >= Q)
        return;
    const int xi = blockIdx.x / BPX, bi = blockIdx.x - xi * BPX;
    const int m0 = bi * MPB, nmem = min(MPB, E - m0);
    double acc = block_out[(size_t)blockIdx.x * Q + q];
    for (int m = 0; m < nmem; ++m)
        acc += rows[((size_t)xi * E + m0 + m) * Q + q];
    block_out[(size_t)blockIdx.x * Q + q] = acc;
}

// gradient = exact contexts: rows[i] = member_rows[i] + rows[i] over the (K N + 1) entries of the launch's members -- the
// unweighted [dJ_k/dx, J_k] join a private copy of the exact gradient's member rows, one addition per number; the weighted
// ensemble reduction behind sums that copy in its own fixed order, and the context's member rows stay without J
__global__ __launch_bounds__(256) void running_cost_join_kernel(const double *__restrict__ member_rows, double *__restrict__ rows,
                                                                size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total)
        rows[i] = member_rows[i] + rows[i];
}

static hipError_t rc_launch_join(const SweepParams &p, hipStream_t stream)
{
    const size_t total = (size_t)p.E * ((size_t)p.K * p.N + 1);
    if (!p.member_out || !p.rc_rows || p.E < 1 || p.K < 1 || p.N < 1 || p.n_x != 1 || (total + 255) / 256 > 0x7fffffffull)
        return hipErrorInvalidConfiguration;
    GRAPE_LAUNCH(running_cost_join_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p.member_out, p.rc_rows,
                 total);
    return hipGetLastError();
}

template <int N, int M>
static hipError_t rc_launch_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = RcTraits<N>::MAXT;
    const int threads = (p.rc_CH + 63) & ~63;
    if (threads > MAXT || p.rc_CH < 1 || (long long)p.S * p.rc_CH < p.N || !p.rc_rows || !p.rc_R || !p.rc_rho ||
        (!p.rc_unitary && !p.rc_xs) || p.rc_terms < 1)
        return hipErrorInvalidConfiguration;
    const dim3 grid(p.E * p.n_x), block(threads);
    hipError_t e = hipSuccess;
    if (p.rc_exact) {
        // the exact derivative mode: W_t into traj_w, then one Frechet derivative per (member, slice) into the rows
        if (!p.traj_w || !p.x || !p.wts || (p.rc_unweighted && p.n_x != 1))
            return hipErrorInvalidConfiguration;
        if (p.rc_unitary)
            GRAPE_LAUNCH_AS("running_cost_exact_kernel", (running_cost_kernel<N, M, true, MAXT, true>), grid, block, 0, stream, p.ops,
                            p.rc_R, p.rc_rho, p.wts, p);
        else
            GRAPE_LAUNCH_AS("running_cost_exact_kernel", (running_cost_kernel<N, M, false, MAXT, true>), grid, block, 0, stream, p.ops,
                            p.rc_R, p.rc_rho, p.wts, p);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
        e = run_traj_frechet(N, false, p, stream);
        if (e != hipSuccess || p.rc_unweighted)          // (gradient = exact contexts: the join follows the exact gradient)
            return e;
    } else {
        if (p.rc_unitary)
            GRAPE_LAUNCH_AS("running_cost_kernel", (running_cost_kernel<N, M, true, MAXT>), grid, block, 0, stream, p.ops, p.rc_R,
                            p.rc_rho, p.wts, p);
        else
            GRAPE_LAUNCH_AS("running_cost_kernel", (running_cost_kernel<N, M, false, MAXT>), grid, block, 0, stream, p.ops, p.rc_R,
                            p.rc_rho, p.wts, p);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    const int Qr = p.K * p.N + 1;
    GRAPE_LAUNCH(running_cost_fold_kernel, dim3(p.BPX * p.n_x, (Qr + 255) / 256), dim3(256), 0, stream, p.rc_rows, p.block_out,
                 p.MPB, p.E, p.BPX, Qr);
    return hipGetLastError();
}

hipError_t run_running_cost(int n, const SweepParams &p, hipStream_t stream)
{
    if (p.rc_only == 2)
        return rc_launch_join(p, stream);
    return dispatch_nm(n, p.rc_m, [&](auto N, auto M) {
        return rc_launch_nm<decltype(N)::value, decltype(M)::value>(p, stream);
    });
}

}  // namespace grape
