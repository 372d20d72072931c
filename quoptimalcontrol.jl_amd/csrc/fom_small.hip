// fom_small.hip -- the figure of merit WITHOUT the gradient for small operators (n = 2, 3, 4) on gfx950:
// grape_eval_fom's fast path (pw_evolve, src/timeevolution.jl:28-39, followed by fom_func, src/cost_functions.jl:99-111,
// or the ADGRAPE functional C1(Xt, U Xi [U']), src/solve.jl:268-361).
//
// Phase A of sweep_small.hip / sweep_pair.hip and nothing behind it.  A lane (fom_lane_kernel: cmat.hpp, any n) or a pair
// of adjacent lanes (fom_pair_kernel: cmatp.hpp, n = 2, 4) owns S consecutive time slices, forms P_t = exp(-i dt H_t) in
// registers (expm_t8, the H build in the reference's association for both variants) and multiplies it onto its running
// chunk product C = P_last ... P_first.  No P_t, no in-chunk prefix and no gradient staging buffer exists: the kernel
// reads the operators and the controls and writes ONE double per member.
//
// The chunk products of a member are combined IN TIME ORDER into U_k = C_last ... C_first.  Only the total is needed,
// so this is a reduction tree, not phase B's prefix scan: inside a wave log2(chunks) shuffle steps (chunk c takes
// chunk c + d's product on the left, d = 1, 2, 4, ...), the wave totals through LDS, multiplied in wave order by the
// member's first lane (pair).  The tree's shape depends on the decomposition (S, W) alone: bitwise reproducible.
// Then X_N = U_k Xi_k (UnitaryGate; n x m states are zero padded) or U_k Xi_k U_k' (State / CoherenceTransfer),
// z = tr(X_N' Xt_k) -- the t-invariant trace the sweeps take at their last slice -- and
//   objective 0:  Re z^2 (UnitaryGate) or 1 - |z / n|^2 (sandwich)          (figure_of_merit of sweep_small.hip)
//   objective 1:  1 - |z / n|^2 for every system type                       (exact_grad.hip)
// Nothing assumes Hermitian generators (UNI only selects expm_t8's anti-Hermitian square): dissipative Liouvillians take
// the same kernels.
//
// Output: fom_member[array][member] = F_k (unweighted), fom_rows[array][workgroup] = sum over the workgroup's members of
// w_k F_k in member order; launch_reduce_rows sums the rows (Q = 1).  One workgroup (single problems): the kernel
// publishes its row itself (SweepParams::direct_dst / direct_flag), as the sweeps do.
//
// The controls are shared by every member of a workgroup: ONE image of x in LDS (the sweeps' chunk-strided layout:
// lane stride S K + 1 doubles, odd, bank-conflict free), or -- pulses too long for LDS -- read from memory in place.
#include "cmatp.hpp"
#include "grape_kernels.hpp"

namespace grape {

constexpr int kFomParityPad = 8;       // double2 slots between a member's two parity images (half an LDS row: see sweep_pair.hip)

// parity image of one matrix in LDS: NE = n*n/2 consecutive double2 (as sweep_pair.hip)
template <int N>
GRAPE_DEV void pload_lds(PMat<N> &m, const double2 *s)
{
#pragma unroll
    for (int e = 0; e < N * (N / 2); ++e) {
        const double2 v = s[e];
        m.re[e] = v.x;
        m.im[e] = v.y;
    }
}

template <int N>
GRAPE_DEV void pstore_lds(double2 *s, const PMat<N> &m)
{
#pragma unroll
    for (int e = 0; e < N * (N / 2); ++e)
        s[e] = make_double2(m.re[e], m.im[e]);
}

template <int N, int SAND>
GRAPE_DEV double fom_value(double zr, double zi, int objective)
{
    if (SAND || objective == 1) {                // 1 - |tr(L'X) / D|^2, src/cost_functions.jl:13-17
        const double inv = 1.0 / (double)N;
        const double ar = zr * inv, ai = zi * inv;
        return 1.0 - (ar * ar + ai * ai);
    }
    return zr * zr - zi * zi;                    // Re(z^2), src/cost_functions.jl:99-101
}

// the workgroup's image of control array `xsrc` (K N doubles): element q = c + K t at q + q / (S K)
GRAPE_DEV void fom_stage_x(double *s_x, const double *__restrict__ xsrc, int KNs, int SK, unsigned magic)
{
    for (int q = threadIdx.x; q < KNs; q += blockDim.x)
        s_x[q + (SK == 1 ? q : (int)__umulhi((unsigned)q, magic))] = xsrc[q];
}

// member results and the workgroup's weighted row; one workgroup: the publication
GRAPE_DEV void fom_write(const SweepParams &p, const double *s_F, const double *__restrict__ wts_all, int xi, int bi)
{
    const int nmem = min(p.MPB, p.E - bi * p.MPB);
    if ((int)threadIdx.x < nmem)
        p.fom_member[(size_t)xi * p.E + (size_t)bi * p.MPB + threadIdx.x] = s_F[threadIdx.x];
    if (threadIdx.x == 0) {
        const double *__restrict__ wb = wts_all + (size_t)bi * p.MPB;
        double acc = 0.0;
        for (int m = 0; m < nmem; ++m)
            acc = fma(s_F[m], wb[m], acc);
        p.fom_rows[blockIdx.x] = acc;
        if (p.direct_dst)
            p.direct_dst[0] = acc;
        if (p.direct_flag) {                     // (reduce.hip: signal_done)
            __threadfence_system();
            __hip_atomic_store(p.direct_flag, p.direct_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---------------------------------------------------------------------------------------------- lane pairs, n = 2, 4
template <int N, int SAND, bool UNI, int MAXT>
__global__ __launch_bounds__(MAXT) void fom_pair_kernel(const double2 *__restrict__ ops_all, const double *__restrict__ x_all,
                                                        const double *__restrict__ wts_all, const SweepParams p, const int xlds)
{
    constexpr int NN = N * N, NC = N / 2, NE = N * NC;
    constexpr int MAXW = MAXT / 64;
    // dynamic LDS:  s_tot  MAXW*NN double2          wave totals (both parity halves)
    //               s_ops  MPB * 2 * PS double2     parity images of the members' [A' | B'_c | Xi | Xt]
    //               s_nrm  MPB * (K+1) double       1-norm bounds of A', B'_c
    //               s_F    MPB double
    //               s_x    K N + CH double          the control array (xlds)
    extern __shared__ double2 s_dyn[];
    double2(*s_tot)[NN] = reinterpret_cast<double2(*)[NN]>(s_dyn);

    const int LT = p.LT, W = LT >> 6;
    const int mb = __builtin_amdgcn_readfirstlane(threadIdx.x / LT);   // member within the block
    const int L = threadIdx.x - mb * LT;             // lane within the member
    const int lane = L & 63, wave = L >> 6;
    const int par = L & 1;                           // parity within the pair
    const int ch = L >> 1;                           // time chunk of the pair
    const int cw = lane >> 1;                        // chunk within the wave (0..31)
    const int wbase_tot = mb * W;
    const int xi = blockIdx.x / p.BPX;               // which control array (batched call)
    const int bi = blockIdx.x - xi * p.BPX;
    int kl = bi * p.MPB + mb;
    if (kl >= p.E)
        kl = p.E - 1;                                // surplus waves repeat the last member (never stored)
    const int K = p.K, Nsl = p.N, S = p.S;
    const int NM = K + 3;                            // images: A', B'_c, Xi, Xt
    const int PS = NM * NE + kFomParityPad;
    double2 *s_ops_all = s_dyn + MAXW * NN;
    double2 *s_ops = s_ops_all + (size_t)mb * 2 * PS;
    const size_t nrm_d2 = ((size_t)p.MPB * (K + 1) + 1) / 2;
    double *s_nrm = reinterpret_cast<double *>(s_ops_all + (size_t)p.MPB * 2 * PS) + (size_t)mb * (K + 1);
    double *s_F = reinterpret_cast<double *>(s_ops_all + (size_t)p.MPB * 2 * PS + nrm_d2);
    double *s_x = s_F + ((p.MPB + 1) & ~1);
    const int SK = S * K;
    const double *__restrict__ xsrc = x_all + (size_t)xi * K * Nsl;
    if (xlds)
        fom_stage_x(s_x, xsrc, K * Nsl, SK, p.sk_magic);
    {
        // parity images of this member's operators: image element (q, mat, e = r + jl n)
        const double2 *__restrict__ ops = ops_all + (size_t)kl * (K + 3) * NN;
        for (int idx = L; idx < 2 * NM * NE; idx += LT) {
            const int q = idx / (NM * NE), rem = idx - q * NM * NE;
            const int mat = rem / NE, e = rem - mat * NE;
            const int r = e % N, jl = e / N;
            const int i = (((r / NC) ^ q) * NC) + (r % NC), j = q * NC + jl;
            s_ops[(size_t)q * PS + rem] = ops[mat * NN + i + j * N];
        }
    }
    __syncthreads();
    if (L <= K) {                                    // one lane per generator: max column sum of |re| + |im|
        double best = 0.0;
        for (int q = 0; q < 2; ++q)
            for (int jl = 0; jl < NC; ++jl) {
                double cs = 0.0;
                for (int r = 0; r < N; ++r) {
                    const double2 v = s_ops[(size_t)q * PS + (size_t)L * NE + r + jl * N];
                    cs += fabs(v.x) + fabs(v.y);
                }
                best = fmax(best, cs);
            }
        s_nrm[L] = best;
    }
    __syncthreads();
    const double2 *sA = s_ops + (size_t)par * PS;               // my parity's images
    const double2 *sB = sA + NE;
    const double2 *sXi = sA + (size_t)(1 + K) * NE;
    const double2 *sXt = sXi + NE;
    const int t0 = ch * S;
    const double *xg_l = s_x + ch * (SK + 1);        // this chunk's controls [j*K + c] ...
    const double *__restrict__ xg_g = xsrc + (size_t)t0 * K;   // ... or where they lie in memory
    auto xval = [&](int j, int c) { return xlds ? xg_l[j * K + c] : xg_g[j * K + c]; };

    // G = -i dt H_t (the operators were multiplied by -i dt on the host) in the reference's association:
    // variant 0  (0 + B_1 x_1 + ...) + A, timeevolution.jl:101-108; variant 1  A + B_1 x_1 + ...
    // returns an upper bound of |G|_1 from the members' operator norms
    auto build = [&](int j, PMat<N> &G) -> double {
        double nb = s_nrm[0];
        if (p.variant != 0)
            pload_lds(G, sA);
        for (int c = 0; c < K; ++c) {
            const double xv = xval(j, c);
            nb = fma(fabs(xv), s_nrm[1 + c], nb);
            if (c == 0 && p.variant == 0) {
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const double2 b = sB[e];
                    G.re[e] = b.x * xv;
                    G.im[e] = b.y * xv;
                }
            } else {
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const double2 b = sB[c * NE + e];
                    G.re[e] = fma(b.x, xv, G.re[e]);
                    G.im[e] = fma(b.y, xv, G.im[e]);
                }
            }
        }
        if (p.variant == 0) {
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const double2 a = sA[e];
                G.re[e] += a.x;
                G.im[e] += a.y;
            }
        }
        return nb;
    };

    // ---------------------------------------------------------------- the chunk product (both lanes of a pair share t0)
    PMat<N> Q, tmp, opar;
    pset_identity(Q);
    {
        bool first = true;
        for (int j = 0; j < S; ++j) {
            if (t0 + j < Nsl) {
                PMat<N> G, P;
                const double nb = build(j, G);
                __builtin_amdgcn_sched_barrier(0);
                pexpm_t8<N, UNI>(P, G, p.s_forced, nb);
                __builtin_amdgcn_sched_barrier(0);
                if (first) {
                    Q = P;
                } else {
                    fetch_partner(opar, P);
                    pmul(tmp, P, opar, Q);
                    Q = tmp;
                }
                first = false;
            }
        }
    }
    // ---------------------------------------------------------------- the member's total, in time order
    {
        PMat<N> oth;
        for (int d = 1; d < 32; d <<= 1) {
            pshfl_down(oth, Q, 2 * d);               // chunk cw + d's product (same parity)
            fetch_partner(opar, oth);
            pmul(tmp, oth, opar, Q);
            if (cw + d < 32)
                Q = tmp;
        }
    }
    if (cw == 0)
        pstore_lds(&s_tot[wbase_tot + wave][par * NE], Q);
    __syncthreads();
    if (L < 2) {                                     // the member's first pair
        PMat<N> T = Q, wt, wtp;
        for (int w = 1; w < W; ++w) {
            pload_lds(wt, &s_tot[wbase_tot + w][par * NE]);
            pload_lds(wtp, &s_tot[wbase_tot + w][(1 - par) * NE]);
            pmul(tmp, wt, wtp, T);
            T = tmp;
        }
        PMat<N> Tp, X, xm;
        fetch_partner(Tp, T);
        pload_lds(xm, sXi);
        pmul(X, T, Tp, xm);                          // U Xi
        if (SAND) {
            fetch_partner(opar, X);
            pmul_a_bh(tmp, X, opar, T, Tp);          // U Xi U'
            X = tmp;
        }
        pload_lds(xm, sXt);
        double zr, zi;
        ptrace_ah_b(zr, zi, X, xm);                  // tr(X_N' Xt)
        if (par == 0)
            s_F[mb] = fom_value<N, SAND>(zr, zi, p.fom_objective);
    }
    __syncthreads();
    fom_write(p, s_F, wts_all, xi, bi);
}

// ---------------------------------------------------------------------------------------------- whole matrices per lane
// ops_all / x_all are separate `const __restrict__` kernel arguments so that the wave-uniform operator entries come
// through scalar loads (see sweep_small.hip)
template <int N, int SAND, bool UNI, int MAXT>
__global__ __launch_bounds__(MAXT) void fom_lane_kernel(const double2 *__restrict__ ops_all, const double *__restrict__ x_all,
                                                        const double *__restrict__ wts_all, const SweepParams p, const int xlds)
{
    constexpr int NN = N * N;
    constexpr int MAXW = MAXT / 64;
    // dynamic LDS:  s_tot  MAXW*NN double2 wave totals;  s_F  MPB double;  s_x  K N + LT double (xlds)
    extern __shared__ double2 s_dyn[];
    double2(*s_tot)[NN] = reinterpret_cast<double2(*)[NN]>(s_dyn);

    const int LT = p.LT, W = LT >> 6;
    const int mb = __builtin_amdgcn_readfirstlane(threadIdx.x / LT);
    const int L = threadIdx.x - mb * LT;
    const int lane = L & 63, wave = L >> 6;
    const int wbase_tot = mb * W;
    const int xi = blockIdx.x / p.BPX;
    const int bi = blockIdx.x - xi * p.BPX;
    int kl = bi * p.MPB + mb;
    if (kl >= p.E)
        kl = p.E - 1;
    const int K = p.K, Nsl = p.N, S = p.S;
    const int SK = S * K;
    double *s_F = reinterpret_cast<double *>(s_dyn + MAXW * NN);
    double *s_x = s_F + ((p.MPB + 1) & ~1);
    const double *__restrict__ xsrc = x_all + (size_t)xi * K * Nsl;
    if (xlds) {
        fom_stage_x(s_x, xsrc, K * Nsl, SK, p.sk_magic);
        __syncthreads();
    }
    const double2 *__restrict__ ops = ops_all + (size_t)kl * (K + 3) * NN;
    const double2 *__restrict__ opB = ops + NN;
    const double2 *__restrict__ opXi = ops + (size_t)(1 + K) * NN;
    const double2 *__restrict__ opXt = opXi + NN;
    const int t0 = L * S;
    const double *xg_l = s_x + L * (SK + 1);
    const double *__restrict__ xg_g = xsrc + (size_t)t0 * K;
    auto xval = [&](int j, int c) { return xlds ? xg_l[j * K + c] : xg_g[j * K + c]; };
    auto load_uniform = [&](CMat<N> &m, const double2 *__restrict__ src) {
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            const double2 v = src[e];
            m.re[e] = v.x;
            m.im[e] = v.y;
        }
    };

    CMat<N> Q, tmp;
    set_identity(Q);
    for (int j = 0; j < S; ++j) {
        if (t0 + j < Nsl) {
            CMat<N> G, P;
            if (p.variant == 0) {
#pragma unroll
                for (int e = 0; e < NN; ++e) { G.re[e] = 0.0; G.im[e] = 0.0; }
            } else {
                load_uniform(G, ops);
            }
            for (int c = 0; c < K; ++c) {
                const double xv = xval(j, c);
#pragma unroll
                for (int e = 0; e < NN; ++e) {
                    const double2 b = opB[c * NN + e];
                    G.re[e] = fma(b.x, xv, G.re[e]);
                    G.im[e] = fma(b.y, xv, G.im[e]);
                }
            }
            if (p.variant == 0) {
#pragma unroll
                for (int e = 0; e < NN; ++e) {
                    const double2 a = ops[e];
                    G.re[e] += a.x;
                    G.im[e] += a.y;
                }
            }
            expm_t8<N, UNI>(P, G, p.s_forced);
            mul(tmp, P, Q);
            Q = tmp;
        }
    }
    {
        CMat<N> oth;
        for (int d = 1; d < 64; d <<= 1) {
            shfl_down(oth, Q, d);                    // chunk lane + d's product
            mul(tmp, oth, Q);
            if (lane + d < 64)
                Q = tmp;
        }
    }
    if (W > 1) {
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < NN; ++e)
                s_tot[wbase_tot + wave][e] = make_double2(Q.re[e], Q.im[e]);
        }
        __syncthreads();
    }
    if (L == 0) {
        CMat<N> T = Q, wt, X;
        for (int w = 1; w < W; ++w) {
            load_uniform(wt, &s_tot[wbase_tot + w][0]);
            mul(tmp, wt, T);
            T = tmp;
        }
        load_uniform(wt, opXi);
        mul(X, T, wt);                               // U Xi
        if (SAND) {
            mul_a_bh(tmp, X, T);                     // U Xi U'
            X = tmp;
        }
        load_uniform(wt, opXt);
        double zr, zi;
        trace_ah_b(zr, zi, X, wt);                   // tr(X_N' Xt)
        s_F[mb] = fom_value<N, SAND>(zr, zi, p.fom_objective);
    }
    __syncthreads();
    fom_write(p, s_F, wts_all, xi, bi);
}

// the sweeps' workgroup limits: the planner's decomposition (LT, MPB) fits both
template <int N> struct FomPairTraits;
template <> struct FomPairTraits<2> { static constexpr int MAXT = 1024; };
template <> struct FomPairTraits<4> { static constexpr int MAXT = 512; };
template <int N> struct FomLaneTraits;
template <> struct FomLaneTraits<2> { static constexpr int MAXT = 1024; };
template <> struct FomLaneTraits<3> { static constexpr int MAXT = 512; };
template <> struct FomLaneTraits<4> { static constexpr int MAXT = 256; };

constexpr size_t kFomLdsCap = 150 * 1024;

template <int N, int SAND, bool UNI>
static hipError_t fom_launch_pair(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = FomPairTraits<N>::MAXT;
    if (p.MPB < 1 || p.LT * p.MPB > MAXT || (p.LT & 63) || (long long)p.S * (p.LT / 2) < p.N)
        return hipErrorInvalidConfiguration;
    const int K = p.K, NE = N * (N / 2);
    size_t lds = sizeof(double2) * ((size_t)(MAXT / 64) * N * N + (size_t)p.MPB * 2 * ((K + 3) * NE + kFomParityPad) +
                                    ((size_t)p.MPB * (K + 1) + 1) / 2) +
                 sizeof(double) * ((p.MPB + 1) & ~1);
    const size_t xb = sizeof(double) * ((size_t)K * p.N + p.LT / 2 + 1);
    const int xlds = lds + xb <= kFomLdsCap ? 1 : 0;
    if (xlds)
        lds += xb;
    if (lds > kFomLdsCap)
        return hipErrorInvalidConfiguration;
    auto kern = fom_pair_kernel<N, SAND, UNI, MAXT>;
    if (lds > 64 * 1024) {
        hipError_t e = ensure_dynamic_lds((const void *)kern, lds);
        if (e != hipSuccess)
            return e;
    }
    GRAPE_LAUNCH_AS("fom_pair_kernel", kern, dim3(p.BPX * p.n_x), dim3(p.LT * p.MPB), lds, stream, p.ops, p.x, p.wts, p, xlds);
    return hipGetLastError();
}

template <int N, int SAND, bool UNI>
static hipError_t fom_launch_lane(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = FomLaneTraits<N>::MAXT;
    if (p.MPB < 1 || p.LT * p.MPB > MAXT || (p.LT & 63) || (long long)p.S * p.LT < p.N)
        return hipErrorInvalidConfiguration;
    size_t lds = sizeof(double2) * ((size_t)(MAXT / 64) * N * N) + sizeof(double) * ((p.MPB + 1) & ~1);
    const size_t xb = sizeof(double) * ((size_t)p.K * p.N + p.LT + 1);
    const int xlds = lds + xb <= kFomLdsCap ? 1 : 0;
    if (xlds)
        lds += xb;
    auto kern = fom_lane_kernel<N, SAND, UNI, MAXT>;
    if (lds > 64 * 1024) {
        hipError_t e = ensure_dynamic_lds((const void *)kern, lds);
        if (e != hipSuccess)
            return e;
    }
    GRAPE_LAUNCH_AS("fom_lane_kernel", kern, dim3(p.BPX * p.n_x), dim3(p.LT * p.MPB), lds, stream, p.ops, p.x, p.wts, p, xlds);
    return hipGetLastError();
}

hipError_t launch_fom_small(int n, int sandwich, int mode, bool pair, const SweepParams &p, hipStream_t stream)
{
    if (!p.fom_member || !p.fom_rows)
        return hipErrorInvalidValue;
    const int uni = mode == 2 ? 1 : 0;
    const int key = n * 4 + (sandwich ? 2 : 0) + uni;
    if (pair) {
        switch (key) {
        case 8: return fom_launch_pair<2, 0, false>(p, stream);
        case 9: return fom_launch_pair<2, 0, true>(p, stream);
        case 10: return fom_launch_pair<2, 1, false>(p, stream);
        case 11: return fom_launch_pair<2, 1, true>(p, stream);
        case 16: return fom_launch_pair<4, 0, false>(p, stream);
        case 17: return fom_launch_pair<4, 0, true>(p, stream);
        case 18: return fom_launch_pair<4, 1, false>(p, stream);
        case 19: return fom_launch_pair<4, 1, true>(p, stream);
        default: return hipErrorInvalidValue;
        }
    }
    switch (key) {
    case 8: return fom_launch_lane<2, 0, false>(p, stream);
    case 9: return fom_launch_lane<2, 0, true>(p, stream);
    case 10: return fom_launch_lane<2, 1, false>(p, stream);
    case 11: return fom_launch_lane<2, 1, true>(p, stream);
    case 12: return fom_launch_lane<3, 0, false>(p, stream);
    case 13: return fom_launch_lane<3, 0, true>(p, stream);
    case 14: return fom_launch_lane<3, 1, false>(p, stream);
    case 15: return fom_launch_lane<3, 1, true>(p, stream);
    case 16: return fom_launch_lane<4, 0, false>(p, stream);
    case 17: return fom_launch_lane<4, 0, true>(p, stream);
    case 18: return fom_launch_lane<4, 1, false>(p, stream);
    case 19: return fom_launch_lane<4, 1, true>(p, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace grape
