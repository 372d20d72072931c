// sweep_small.hip -- the GRAPE hot path for small operators (n = 2, 3, 4) on gfx950.
//
// One workgroup per ensemble member, W wavefronts per workgroup; every lane owns S consecutive
// time slices and whole n x n ComplexF64 matrices in VGPRs (cmat.hpp).  The time axis, serial
// in the reference (src/GRAPE.jl:53-75), is cut into 64*W lane chunks and stitched with a
// wavefront-shuffle prefix/suffix product scan, so all lanes work for the whole kernel:
//
//   phase A  pw_prop_save!  (src/timeevolution.jl:98-110): H_t = sum_j B_j x[j,t] + A,
//            P_t = exp(-i dt H_t) (expm_t8), P_t -> HBM, chunk product Q = P_last ... P_first
//   phase B  scan over lanes/waves: U_L = Q_{L-1}...Q_0 (exclusive prefix), V_L = Q_last...Q_{L+1}
//            (exclusive suffix); X at chunk start = U Xi [U'], L at chunk end = V' Xt [V]
//   phase C  evolve_func! forward (src/GRAPE.jl:226 / :245-246) inside the chunk, X_t -> HBM
//   phase D  evolve_func! backward (:228 / :248-249) fused with grad_func! (:261-287) and
//            fom_func (src/cost_functions.jl:99-111): the costates never leave registers;
//            tr(L' B_c X) = sum_ij B_c[i,j] (X L')[j,i]  (the trace_matmul identity,
//            src/grape_tools.jl:66-68), so one product per slice serves all K controls.
//
// Two data flows share phases A and B:
//   MODE_GENERAL (any generator, e.g. non-Hermitian Liouvillians): the reference's flow -- forward
//     states X_t, costates L_t pulled back, M_t = X_t L_t' per slice -- with one change of
//     bookkeeping: phase A also stores the running in-chunk product Q_j = P_j ... P_first, and the
//     backward sweep rebuilds X_t = Q_{j-1} Xs [Q_{j-1}'] from it, so there is no separate forward
//     sweep (no phase C) and P_t is read once instead of twice.  HBM traffic = "model S" of
//     two matrices per slice make one round trip (64 n^2 N bytes per member).
//   MODE_GENERAL_KEEPL (debug, GRAPE_FLAG_KEEP_COSTATES): the literal reference flow with the
//     forward sweep (phase C) storing X_t and every L_t stored, for grape_get_trajectory.
//   MODE_UNITARY (every A_k, B_jk Hermitian, checked on the host, so every P_t is unitary):
//     M_t = X_t L_t' (UnitaryGate) or [X_t, L_t'] (State/CoherenceTransfer) obeys
//     M_t = P_t' M_{t+1} P_t, so the backward sweep carries ONE matrix, no forward state is
//     stored and phase C disappears: only P_t makes the HBM round trip (32 n^2 N bytes per
//     member) and the sweep needs 2 products per slice instead of 3-6.  tr(X_t' L_t), which
//     the UnitaryGate gradient and both figures of merit use, is conj(tr M_t) (UnitaryGate) or
//     t-invariant (taken at the chunk end that owns slice N).
// All workspace accesses are lane-contiguous 16-byte accesses (1 KiB per wave instruction).
#include "cmat.hpp"
#include "grape_kernels.hpp"

namespace grape {

template <int N>
GRAPE_DEV void load_uniform(CMat<N> &m, const double2 *__restrict__ src)
{
#pragma unroll
    for (int e = 0; e < N * N; ++e) {
        const double2 v = src[e];
        m.re[e] = v.x;
        m.im[e] = v.y;
    }
}

template <int N>
GRAPE_DEV void store_ws(double2 *__restrict__ base, size_t stride, const CMat<N> &m)
{
#pragma unroll
    for (int e = 0; e < N * N; ++e)
        base[e * stride] = make_double2(m.re[e], m.im[e]);
}

template <int N>
GRAPE_DEV void load_ws(CMat<N> &m, const double2 *__restrict__ base, size_t stride)
{
#pragma unroll
    for (int e = 0; e < N * N; ++e) {
        const double2 v = base[e * stride];
        m.re[e] = v.x;
        m.im[e] = v.y;
    }
}

// diagnostic phase stamps (GRAPE_FLAG_PHASE_STAMPS): lane 0 of every wave stores the shader
// clock at the phase boundaries into a buffer nothing else reads.  p.stamps is NULL in
// production, so no stamp executes there.
GRAPE_DEV void stamp(unsigned long long *__restrict__ st, int slot)
{
    if (st) {
        const unsigned long long t = __builtin_readcyclecounter();
        if ((threadIdx.x & 63) == 0)
            st[slot] = t;
    }
}

enum { MODE_GENERAL = 0, MODE_GENERAL_KEEPL = 1, MODE_UNITARY = 2 };

// sum_ij B[i,j] M[j,i] for the K control operators of this member -> gradient entries
template <int N, int SAND>
GRAPE_DEV void write_gradient(double *out, const double2 *__restrict__ opB, int K, const CMat<N> &M, double zr,
                              double zi, double gs)
{
    constexpr int NN = N * N;
    // opB holds B' = -i dt B, so w' = tr(B' M) = -i dt w and the reference's entries are
    //   sandwich:     dt Im(w)   = Re(w')
    //   UnitaryGate:  dt Im(w z) = Re(w' z) = Re(tr(B' (z M)))
    // Only a REAL part is needed: fold z into M once, then 2 FMAs per operator entry instead of 4.
    CMat<N> Z;
#pragma unroll
    for (int e = 0; e < NN; ++e) {
        if (SAND) {
            Z.re[e] = M.re[e];
            Z.im[e] = M.im[e];
        } else {
            Z.re[e] = fma(M.re[e], zr, -M.im[e] * zi);
            Z.im[e] = fma(M.re[e], zi, M.im[e] * zr);
        }
    }
    for (int c = 0; c < K; ++c) {
        double re = 0.0;
#pragma unroll
        for (int jj = 0; jj < N; ++jj)
#pragma unroll
            for (int ii = 0; ii < N; ++ii) {
                const double2 b = opB[c * NN + ii + jj * N];
                re = fma(b.x, Z.re[jj + ii * N], re);
                re = fma(-b.y, Z.im[jj + ii * N], re);
            }
        out[c] = gs * re;
    }
}

template <int N, int SAND>
GRAPE_DEV double figure_of_merit(double zr, double zi)
{
    if (SAND) {                                  // 1 - |tr(L'X)/D|^2, cost_functions.jl:13-17
        const double inv = 1.0 / (double)N;
        const double ar = zr * inv, ai = zi * inv;
        return 1.0 - (ar * ar + ai * ai);
    }
    return zr * zr - zi * zi;                    // Re(z^2), cost_functions.jl:99-101
}

// ops_all / x_all are separate `const __restrict__` kernel arguments (not members of the
// parameter struct) so that the compiler can prove them read-only and fetch the wave-uniform
// operator entries with scalar loads (s_load_dwordx16 -> SGPR operands of v_fma_f64).
// XGLDS: the controls/gradient staging buffer lives in LDS (normal case); false: it lives in a
// global scratch buffer (very long pulses, where K*N doubles per member no longer fit in LDS).
template <int N, int SAND, int MODE, int MAXT, bool XGLDS>
__global__ __launch_bounds__(MAXT) void sweep_small_kernel(const double2 *__restrict__ ops_all,
                                                           const double *__restrict__ x_all,
                                                           const double *__restrict__ wts_all,
                                                           const SweepParams p)
{
    constexpr int NN = N * N;
    constexpr int MAXW = MAXT / 64;
    constexpr bool UNI = (MODE == MODE_UNITARY);
    constexpr bool KEEPL = (MODE == MODE_GENERAL_KEEPL);
    // One dynamic LDS array (16-byte aligned carve, nothing static in front of it):
    //   s_tot  2*MAXW*NN double2   wave totals of the two scans
    //   s_xg   MPB*LT*(S*K+1) double  per member: controls x[., t] of its slices on the way in,
    //                              the gradient g[., t] on the way out; lane stride S*K+1 is odd,
    //                              so the per-lane reads/writes are bank-conflict free
    //   s_F    MPB double          figures of merit of the block's members
    // A workgroup holds MPB members (W waves each): their weighted results are summed in LDS
    // before leaving the chip (first level of src/solve.jl:171-191), so the ensemble reduction
    // that follows reads E/MPB rows instead of E.
    extern __shared__ double2 s_dyn[];
    double2(*s_tot)[MAXW][NN] = reinterpret_cast<double2(*)[MAXW][NN]>(s_dyn);

    const int LT = p.LT, W = LT >> 6;
    // LT is a multiple of 64, so mb is the same in every lane of a wave: say so, or the
    // operator loads below stop being scalar loads
    const int mb = __builtin_amdgcn_readfirstlane(threadIdx.x / LT);   // member within the block
    const int L = threadIdx.x - mb * LT;             // lane within the member
    const int lane = L & 63, wave = L >> 6;
    const int wbase_tot = mb * W;                    // this member's rows of s_tot
    // batched evaluation (grape_eval_batch): the grid is n_x copies of the ensemble's BPX
    // workgroups, copy xi evaluates control array xi; a workgroup never straddles two copies
    const int xi = blockIdx.x / p.BPX;               // which control array
    const int bi = blockIdx.x - xi * p.BPX;          // workgroup within the ensemble
    int kl = bi * p.MPB + mb;                        // member within the ensemble
    const bool valid = kl < p.E;
    if (!valid)
        kl = p.E - 1;                                // surplus waves repeat the last member (never stored)
    const int k = xi * p.E + kl;                     // row of the workspace / per-member output
    const int K = p.K, Nsl = p.N, S = p.S;
    const size_t stride = (size_t)LT;

    const int SK = S * K;
    double *s_xg_all = XGLDS ? reinterpret_cast<double *>(s_dyn + 2 * MAXW * NN)
                             : p.xg_scratch + (size_t)blockIdx.x * ((size_t)p.MPB * LT * (SK + 1) + p.MPB);
    double *s_xg = s_xg_all + (size_t)mb * LT * (SK + 1);
    double *s_F = s_xg_all + (size_t)p.MPB * LT * (SK + 1);
    const unsigned magic = p.sk_magic;               // q / SK == __umulhi(q, magic) for q * SK < 2^32
    auto chunk_of = [&](int q) { return SK == 1 ? q : (int)__umulhi((unsigned)q, magic); };
    {
        const double *__restrict__ xsrc = x_all + (size_t)xi * K * Nsl;
        for (int q = L; q < K * Nsl; q += LT)
            s_xg[q + chunk_of(q)] = xsrc[q];         // lq*(SK+1) + (q - lq*SK) = q + lq
    }
    __syncthreads();
    const double2 *__restrict__ ops = ops_all + (size_t)kl * (K + 3) * NN;
    const double2 *__restrict__ opB = ops + NN;
    const double2 *__restrict__ opXi = ops + (size_t)(1 + K) * NN;
    const double2 *__restrict__ opXt = opXi + NN;
    double *xg = s_xg + L * (SK + 1);            // this lane's x / g slots: [j*K + c]
    const size_t wbase = (size_t)k * S * NN * stride + L;
    double2 *__restrict__ Pw = p.props + wbase;
    double2 *__restrict__ Xw = p.states + wbase;
    double *__restrict__ out = p.member_out + (size_t)k * ((size_t)K * Nsl + 1);
    const int t0 = L * S;
    unsigned long long *__restrict__ st =
        p.stamps ? p.stamps + ((size_t)k * W + wave) * kStampSlots : nullptr;
    if (st && lane == 0)
        st[5] = __builtin_amdgcn_s_memrealtime();
    stamp(st, 0);

    // ---------------------------------------------------------------- phase A
    // Q accumulates the chunk product P_last ... P_first; two buffers alternate so that the
    // product never needs a register copy (Qout = P * Qin).
    CMat<N> Q, Q2;
    set_identity(Q);
    // generators of TWO consecutive slices are assembled in one pass over the member's operators:
    // every scalar-loaded operator entry feeds both slices, halving the scalar-load round trips
    auto build2 = [&](int j, int j1, CMat<N> &G0, CMat<N> &G1) {
        if (p.variant == 0) {
#pragma unroll
            for (int e = 0; e < NN; ++e) { G0.re[e] = 0.0; G0.im[e] = 0.0; G1.re[e] = 0.0; G1.im[e] = 0.0; }
        } else {
            load_uniform(G0, ops);
            G1 = G0;
        }
        for (int c = 0; c < K; ++c) {
            const double x0 = xg[j * K + c], x1 = xg[j1 * K + c];
#pragma unroll
            for (int e = 0; e < NN; ++e) {
                const double2 b = opB[c * NN + e];
                G0.re[e] = fma(b.x, x0, G0.re[e]);
                G0.im[e] = fma(b.y, x0, G0.im[e]);
                G1.re[e] = fma(b.x, x1, G1.re[e]);
                G1.im[e] = fma(b.y, x1, G1.im[e]);
            }
        }
        if (p.variant == 0) {
#pragma unroll
            for (int e = 0; e < NN; ++e) {
                const double2 a = ops[e];
                G0.re[e] += a.x;
                G0.im[e] += a.y;
                G1.re[e] += a.x;
                G1.im[e] += a.y;
            }
        }
    };
    // (the operators were multiplied by -i dt on the host: G already is -i dt H)
    auto finish = [&](int j, CMat<N> &G, const CMat<N> &Qin, CMat<N> &Qout) {
        if (t0 + j < Nsl) {
            CMat<N> P;
            expm_t8<N, UNI>(P, G, p.s_forced);
            store_ws(Pw + (size_t)j * NN * stride, stride, P);
            mul(Qout, P, Qin);
            if (MODE == MODE_GENERAL)                // in-chunk prefix product, read back in phase D
                store_ws(Xw + (size_t)j * NN * stride, stride, Qout);
        } else {
            Qout = Qin;
        }
    };
    {
        CMat<N> G0, G1;
        int j = 0;
        for (; j + 1 < S; j += 2) {
            build2(j, j + 1, G0, G1);
            finish(j, G0, Q, Q2);
            finish(j + 1, G1, Q2, Q);
        }
        if (j < S) {                                // odd S: the last slice alone
            build2(j, j, G0, G1);
            finish(j, G0, Q, Q2);
            Q = Q2;
        }
    }

    // unitary flow: the first propagator the backward sweep needs (the chunk's last slice) is
    // requested now, so its latency hides under the scan
    CMat<N> P0;
    if (UNI)
        load_ws(P0, Pw + (size_t)(S - 1) * NN * stride, stride);

    stamp(st, 1);
    // ---------------------------------------------------------------- phase B
    // General flow: Xs = state at the chunk start, Le = costate at the chunk end.
    // Unitary flow: M = M at the chunk end, from the forward scan alone: with U the inclusive
    // prefix product of this lane and T the product of ALL propagators of the member, the
    // exclusive suffix is V = T U' (U unitary), hence
    //   UnitaryGate:  M_end = X L' = U (Xi Xt' T) U'
    //   sandwich:     M_end = [X, L'] = U [Xi, E'] U',  E = T' Xt T,  tr(X' L) = tr(Xi' E).
    CMat<N> Xs, Le;
    double zr = 0.0, zi = 0.0;
    {
        CMat<N> inc = Q, oth, tmp;
        for (int d = 1; d < 64; d <<= 1) {
            shfl_up(oth, inc, d);
            if (lane >= d) {
                mul(tmp, inc, oth);
                inc = tmp;
            }
        }
        if (!UNI) {                                  // exclusive prefix
            shfl_up(oth, inc, 1);
            if (lane == 0)
                set_identity(oth);
        }
        if (W > 1) {
            if (lane == 63) {
#pragma unroll
                for (int e = 0; e < NN; ++e)
                    s_tot[0][wbase_tot + wave][e] = make_double2(inc.re[e], inc.im[e]);
            }
            __syncthreads();
            CMat<N> pre, wt;
            set_identity(pre);
            for (int w = 0; w < wave; ++w) {
                load_uniform(wt, &s_tot[0][wbase_tot + w][0]);
                mul(tmp, wt, pre);
                pre = tmp;
            }
            if (UNI) {
                mul(tmp, inc, pre);
                inc = tmp;
            } else {
                mul(tmp, oth, pre);
                oth = tmp;
            }
        }
        if (UNI) {
            if (L == LT - 1) {
#pragma unroll
                for (int e = 0; e < NN; ++e)
                    s_tot[1][wbase_tot][e] = make_double2(inc.re[e], inc.im[e]);
            }
            __syncthreads();
            CMat<N> T, C0, xi, xt;
            load_uniform(T, &s_tot[1][wbase_tot][0]);
            load_uniform(xi, opXi);
            load_uniform(xt, opXt);
            if (SAND) {
                mul(tmp, xt, T);
                mul_ah_b(oth, T, tmp);               // E = T' Xt T
                trace_ah_b(zr, zi, xi, oth);         // tr(Xi' E) = tr(X_t' L_t) for every t
                mul_a_bh(C0, xi, oth);               // Xi E'
                mul_ah_b(tmp, oth, xi);              // E' Xi
#pragma unroll
                for (int e = 0; e < NN; ++e) {
                    C0.re[e] -= tmp.re[e];
                    C0.im[e] -= tmp.im[e];
                }
            } else {
                mul_a_bh(tmp, xi, xt);               // Xi Xt'
                mul(C0, tmp, T);
            }
            mul(tmp, inc, C0);
            mul_a_bh(Xs, tmp, inc);                  // Xs := M at the chunk end
        } else {
            CMat<N> xi;
            load_uniform(xi, opXi);
            if (SAND) {
                mul(tmp, oth, xi);
                mul_a_bh(Xs, tmp, oth);
            } else {
                mul(Xs, oth, xi);
            }
        }
    }
    if (!UNI) {
        CMat<N> inc = Q, oth, tmp;
        for (int d = 1; d < 64; d <<= 1) {
            shfl_down(oth, inc, d);
            if (lane + d < 64) {
                mul(tmp, oth, inc);
                inc = tmp;
            }
        }
        shfl_down(oth, inc, 1);
        if (lane == 63)
            set_identity(oth);
        if (W > 1) {
            if (lane == 0) {
#pragma unroll
                for (int e = 0; e < NN; ++e)
                    s_tot[1][wbase_tot + wave][e] = make_double2(inc.re[e], inc.im[e]);
            }
            __syncthreads();
            CMat<N> post;
            set_identity(post);
            for (int w = wave + 1; w < W; ++w) {
                load_uniform(inc, &s_tot[1][wbase_tot + w][0]);
                mul(tmp, inc, post);
                post = tmp;
            }
            mul(tmp, post, oth);
            oth = tmp;
        }
        load_uniform(inc, opXt);
        if (SAND) {
            mul_ah_b(tmp, oth, inc);
            mul(Le, tmp, oth);
        } else {
            mul_ah_b(Le, oth, inc);
        }
    }

    const double gs = SAND ? -1.0 : (p.variant == 0 ? -2.0 : 2.0);

    if (UNI) {
        stamp(st, 2);
        stamp(st, 3);
        // ------------------------------------------------------------ phase D, unitary flow
        CMat<N> M = Xs, tmp;
        CMat<N> P1;
        // software pipeline: P of slice j-1 is in flight while slice j is processed
        auto step = [&](int j, const CMat<N> &P) {
            const int t = t0 + j;
            if (t < Nsl) {
                mul(tmp, M, P);
                mul_ah_b(M, P, tmp);                 // M_t = P' M_{t+1} P
                if (!SAND) {                         // z_t = tr(X_t' L_t) = conj(tr M_t)
                    double tr_r = 0.0, tr_i = 0.0;
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        tr_r += M.re[i + i * N];
                        tr_i += M.im[i + i * N];
                    }
                    zr = tr_r;
                    zi = -tr_i;
                }
                write_gradient<N, SAND>(xg + j * K, opB, K, M, zr, zi, gs);
                if (t == Nsl - 1)
                    s_F[mb] = figure_of_merit<N, SAND>(zr, zi);
            }
        };
        int j = S - 1;
        for (; j >= 1; j -= 2) {
            load_ws(P1, Pw + (size_t)(j - 1) * NN * stride, stride);
            step(j, P0);
            if (j >= 2)
                load_ws(P0, Pw + (size_t)(j - 2) * NN * stride, stride);
            step(j - 1, P1);
        }
        if (j == 0)
            step(0, P0);
    } else {
        stamp(st, 2);
        // ------------------------------------------------------------ phase C (debug flow only)
        if (KEEPL) {
            CMat<N> X = Xs, P, tmp;
            for (int j = 0; j < S; ++j) {
                const int t = t0 + j;
                if (t < Nsl) {
                    store_ws(Xw + (size_t)j * NN * stride, stride, X);
                    if (j + 1 < S) {                   // the chunk's last state is never read
                        load_ws(P, Pw + (size_t)j * NN * stride, stride);
                        if (SAND) {
                            mul_a_bh(tmp, X, P);
                            mul(X, P, tmp);
                        } else {
                            mul(tmp, P, X);
                            X = tmp;
                        }
                    }
                }
            }
        }

        stamp(st, 3);
        // ------------------------------------------------------------ phase D, general flow
        CMat<N> Lc = Le, P, X, M, tmp;
        for (int j = S - 1; j >= 0; --j) {
            const int t = t0 + j;
            if (t < Nsl) {
                load_ws(P, Pw + (size_t)j * NN * stride, stride);
                if (KEEPL) {
                    load_ws(X, Xw + (size_t)j * NN * stride, stride);
                } else if (j > 0) {
                    load_ws(M, Xw + (size_t)(j - 1) * NN * stride, stride);   // Q_{j-1}
                }
                if (SAND) {
                    mul(tmp, Lc, P);
                    mul_ah_b(Lc, P, tmp);
                } else {
                    mul_ah_b(tmp, P, Lc);
                    Lc = tmp;
                }
                if (!KEEPL) {                        // X_t = Q_{j-1} Xs [Q_{j-1}'] ; X at the chunk start is Xs
                    if (j > 0) {
                        if (SAND) {
                            mul(tmp, M, Xs);
                            mul_a_bh(X, tmp, M);
                        } else {
                            mul(X, M, Xs);
                        }
                    } else {
                        X = Xs;
                    }
                }
                if (KEEPL)
                    store_ws(p.costates + wbase + (size_t)j * NN * stride, stride, Lc);
                double zr, zi;
                trace_ah_b(zr, zi, X, Lc);           // tr(X' L)
                mul_a_bh(M, X, Lc);                  // X L'
                if (SAND) {
                    mul_ah_b(tmp, Lc, X);            // L' X
#pragma unroll
                    for (int e = 0; e < NN; ++e) {
                        M.re[e] -= tmp.re[e];
                        M.im[e] -= tmp.im[e];
                    }
                }
                write_gradient<N, SAND>(xg + j * K, opB, K, M, zr, zi, gs);
                if (t == Nsl - 1)
                    s_F[mb] = figure_of_merit<N, SAND>(zr, zi);
            }
        }
    }
    // results: LDS -> HBM, lane-contiguous.  (1) this member's unweighted row (the reference's
    // gradient[k,:,:] and F_k: parity/debug accessor), (2) the block's weighted partial sum.
    __syncthreads();
    const int KN = K * Nsl;
    if (p.member_out && valid) {
        for (int q = L; q < KN; q += LT)
            out[q] = s_xg[q + chunk_of(q)];
        if (L == 0)
            out[KN] = s_F[mb];
    }
    {
        const int nmem = min(p.MPB, p.E - bi * p.MPB);
        const double *__restrict__ wb = wts_all + (size_t)bi * p.MPB;
        double *__restrict__ bout = p.block_out + (size_t)blockIdx.x * (KN + 1);
        const int mstride = LT * (SK + 1);
        for (int q = threadIdx.x; q <= KN; q += blockDim.x) {
            const int off = q + chunk_of(q);
            double acc = 0.0;
            for (int m = 0; m < nmem; ++m) {
                const double v = (q < KN) ? s_xg_all[m * mstride + off] : s_F[m];
                acc = fma(v, wb[m], acc);
            }
            bout[q] = acc;
            if (p.direct_dst)
                p.direct_dst[q] = acc;
        }
    }
    if (p.direct_flag) {               // one workgroup: the result is complete, tell the host (reduce.hip: signal_done)
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_store(p.direct_flag, p.direct_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    stamp(st, 4);
    if (st && lane == 0) {
        st[6] = __builtin_amdgcn_s_memrealtime();
        // where the wave ran: HW_REG_XCC_ID (hwreg 20) in the high word, HW_REG_HW_ID (hwreg 4) in the low
        st[7] = ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32) |
                (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11));
    }
}

template <int N>
struct SmallTraits;
template <> struct SmallTraits<2> { static constexpr int MAXT = 1024; };
template <> struct SmallTraits<3> { static constexpr int MAXT = 512; };
template <> struct SmallTraits<4> { static constexpr int MAXT = 256; };

int sweep_small_max_waves(int n)
{
    switch (n) {
    case 2: return SmallTraits<2>::MAXT / 64;
    case 3: return SmallTraits<3>::MAXT / 64;
    case 4: return SmallTraits<4>::MAXT / 64;
    default: return 0;
    }
}

size_t sweep_small_lds_bytes(int n, int MPB, int LT, int S, int K, bool xg_in_lds)
{
    const int maxt = n == 2 ? SmallTraits<2>::MAXT : (n == 3 ? SmallTraits<3>::MAXT : SmallTraits<4>::MAXT);
    size_t b = sizeof(double2) * (2 * (size_t)(maxt / 64) * n * n);
    if (xg_in_lds)
        b += sizeof(double) * ((size_t)MPB * LT * ((size_t)S * K + 1) + MPB);
    return b;
}

template <int N, int SAND, int MODE, bool XGLDS>
static hipError_t launch_one(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = SmallTraits<N>::MAXT;
    const dim3 grid(p.BPX * p.n_x), block(p.LT * p.MPB);
    const size_t lds = sweep_small_lds_bytes(N, p.MPB, p.LT, p.S, p.K, XGLDS);
    if (lds > 160 * 1024)
        return hipErrorInvalidConfiguration;
    auto kern = sweep_small_kernel<N, SAND, MODE, MAXT, XGLDS>;
    if (lds > 64 * 1024) {                       // above the default dynamic-LDS cap: opt in
        hipError_t e = ensure_dynamic_lds((const void *)kern, lds);
        if (e != hipSuccess)
            return e;
    }
    GRAPE_LAUNCH_AS("sweep_small_kernel", kern, grid, block, lds, stream, p.ops, p.x, p.wts, p);
    return hipGetLastError();
}

template <int N, int SAND>
static hipError_t launch_ns(int mode, const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = SmallTraits<N>::MAXT;
    if (p.MPB < 1 || p.LT * p.MPB > MAXT || (p.LT & 63) || (long long)p.S * p.LT < p.N)
        return hipErrorInvalidConfiguration;
    const bool lds = p.xg_scratch == nullptr;
    switch (mode) {
    case MODE_GENERAL:
        return lds ? launch_one<N, SAND, MODE_GENERAL, true>(p, stream) : launch_one<N, SAND, MODE_GENERAL, false>(p, stream);
    case MODE_GENERAL_KEEPL:
        return lds ? launch_one<N, SAND, MODE_GENERAL_KEEPL, true>(p, stream)
                   : launch_one<N, SAND, MODE_GENERAL_KEEPL, false>(p, stream);
    case MODE_UNITARY:
        return lds ? launch_one<N, SAND, MODE_UNITARY, true>(p, stream) : launch_one<N, SAND, MODE_UNITARY, false>(p, stream);
    default:
        return hipErrorInvalidValue;
    }
}

hipError_t launch_sweep_small(int n, int sandwich, int mode, const SweepParams &p, hipStream_t stream)
{
    if (p.fom_only)                                  // grape_eval_fom: the forward-only kernel (fom_small.hip)
        return launch_fom_small(n, sandwich, mode, false, p, stream);
    if (p.rc_only)                                   // grape_set_running_cost: the kernels behind the sweep (running_cost.hip)
        return run_running_cost(n, p, stream);
    if (p.obs_only)                                  // grape_eval_observables: the kernel behind the sweep (observe.hip)
        return run_observe(n, sandwich, p, stream);
    if (p.vjp_only)                                  // grape_eval_vjp: the kernels behind the sweep (vjp.hip)
        return run_trajectory_vjp(n, p, stream);
    if (p.jvp_only)                                  // grape_eval_jvp: the kernel behind the sweep (jvp.hip)
        return run_trajectory_jvp(n, p, stream);
    if (p.hvp_only)                                  // grape_eval_hvp: the kernels behind the sweep (hvp.hip)
        return run_trajectory_hvp(n, p, stream);
    if (p.gnvp_only)                                 // grape_eval_gnvp: the kernels behind the sweep (gnvp.hip)
        return run_trajectory_gnvp(n, p, stream);
    if (p.gn)                                        // grape_gn_step: the kernels of the call's record (gn_step.hip)
        return run_gn_step(n, p, stream);
    switch (n * 2 + (sandwich ? 1 : 0)) {
    case 4: return launch_ns<2, 0>(mode, p, stream);
    case 5: return launch_ns<2, 1>(mode, p, stream);
    case 6: return launch_ns<3, 0>(mode, p, stream);
    case 7: return launch_ns<3, 1>(mode, p, stream);
    case 8: return launch_ns<4, 0>(mode, p, stream);
    case 9: return launch_ns<4, 1>(mode, p, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace grape
