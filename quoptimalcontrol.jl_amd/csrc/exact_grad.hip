// exact_grad.hip -- exact control gradient for small operators (n <= 4): the functional path of the reference.
//
// The reference's GRAPE gradient (grad_func!, src/GRAPE.jl:261-287) is first order in dt.  Its ADGRAPE path
// (src/solve.jl:268-361 with pw_evolve, src/timeevolution.jl:28-39) differentiates the functional
//     F(x) = sum_k w_k C1(Xt_k, U_k Xi_k [U_k'])         U_k = prod_t exp(-i dt H_t)
// exactly with Zygote, and src/grape_tools.jl:26-57 (eig_factors / expm_exact_gradient, unused) sketches the
// exact derivative of the propagator.  This kernel gives that exact gradient without an AD tape:
//     dPhi/dx[c,t] = tr( L_{t+1}' dP_t[c] X_t )                                  (UnitaryGate)
//                  = tr( L_{t+1}' (dP_t[c] X_t P_t' + P_t X_t dP_t[c]') )        (State/CoherenceTransfer)
// with X_t the state before slice t, L_{t+1} the costate after it (both left in HBM by the sweep's debug flow,
// GRAPE_FLAG_KEEP_COSTATES), and dP_t[c] the Frechet derivative of exp at G_t = -i dt H_t in direction
// B'_c = -i dt B_c, obtained by differentiating the sweep's own Taylor-8 + scaling/squaring evaluation
// (cmat.hpp: expm_t8) operation by operation -- exact to the rounding of P_t itself.
//     C1-type objectives (1 - |Phi/D|^2):   dF = -(2/D^2) Re( conj(Phi) dPhi )
//     GRAPE UnitaryGate objective Re(z^2), z = conj(Phi):   dF = 2 Re( z conj(dPhi) )
// One lane per (member, slice); a wave covers 64 slices of one member, so the member's operators are wave
// uniform.  The register footprint (a dozen 4 x 4 complex matrices) spills to scratch: this is the optional
// accuracy path, not the throughput path.
#include <cstdlib>

#include "cmat.hpp"
#include "cmatp.hpp"
#include "frechet.hpp"
#include "grape_kernels.hpp"

namespace grape {

template <int N, int SAND>
__global__ __launch_bounds__(64) void exact_grad_kernel(const double2 *__restrict__ ops_all, const double *__restrict__ x_all,
                                                        const ExactParams p)
{
    constexpr int NN = N * N;
    const int k = blockIdx.y;
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int K = p.K, Nsl = p.N;
    const bool live = t < Nsl;
    const int tt = live ? t : Nsl - 1;                   // surplus lanes repeat the last slice (never stored)
    const double2 *__restrict__ ops = ops_all + (size_t)k * (K + 3) * NN;
    const double2 *__restrict__ opB = ops + NN;
    const double2 *__restrict__ opXt = ops + (size_t)(2 + K) * NN;
    auto ws_load = [&](CMat<N> &m, const double2 *__restrict__ ws, int slice) {
        const int L = slice / p.S, j = slice - L * p.S;
        const double2 *__restrict__ base = ws + ((size_t)k * p.S + j) * NN * p.CH + L;
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            const double2 v = base[(size_t)e * p.CH];
            m.re[e] = v.x;
            m.im[e] = v.y;
        }
    };
    CMat<N> P, X, Ln;
    ws_load(P, p.props, tt);
    ws_load(X, p.states, tt);
    if (tt + 1 < Nsl) {
        ws_load(Ln, p.costates, tt + 1);                 // costate after slice t
    } else {
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            const double2 v = opXt[e];
            Ln.re[e] = v.x;
            Ln.im[e] = v.y;
        }
    }
    // W: dPhi = tr(dP W1) [+ conj(tr(dP W2))] ;  Phi = tr(L_{t+1}' X_{t+1})
    CMat<N> W1, W2, tmp;
    double phr, phi;
    if (SAND) {
        CMat<N> Y;
        mul_a_bh(Y, X, P);                               // X P'
        mul_a_bh(W1, Y, Ln);                             // X P' L'
        mul(tmp, P, Y);                                  // X_{t+1} = P X P'
        trace_ah_b(phr, phi, Ln, tmp);
        mul_ah_b(Y, P, Ln);                              // P' L
        mul_ah_b(W2, X, Y);                              // X' P' L
    } else {
        mul_a_bh(W1, X, Ln);                             // X L'
        mul(tmp, P, X);                                  // X_{t+1} = P X
        trace_ah_b(phr, phi, Ln, tmp);
    }
    // generator of this slice and the shared part of the Taylor-8 evaluation (frechet.hpp)
    FrechetLane<N> fr;
    build_generator(fr.G, ops, opB, x_all + (size_t)tt * K, K, p.variant);
    fr.prepare(p.s_forced);

    double *__restrict__ out = p.member_out + (size_t)k * ((size_t)K * Nsl + 1);
    const double D2 = 1.0 / ((double)N * (double)N);
    // ONE derivative in the direction W1 (and one in W2 where the sandwich needs it) serves all K controls (frechet.hpp)
    CMat<N> D1, D2m;
    fr.apply(D1, W1);
    const bool second = SAND && !p.herm_states;          // Hermitian X, L: W2 == W1
    if (second)
        fr.apply(D2m, W2);
    for (int c = 0; c < K; ++c) {
        CMat<N> Bc;
#pragma unroll
        for (int e = 0; e < NN; ++e) { const double2 b = opB[c * NN + e]; Bc.re[e] = b.x; Bc.im[e] = b.y; }
        double ar, ai, dr, di;
        trace_ab(ar, ai, D1, Bc);                        // tr(L' dP_c X [P']) = tr(DF[W1] B'_c)
        dr = ar;
        di = ai;
        if (SAND) {
            if (second)
                trace_ab(ar, ai, D2m, Bc);               // + conj(tr(dP_c X' P' L))
            dr += ar;
            di -= ai;
        }
        double g;
        if (SAND || p.objective == 1)
            g = -2.0 * D2 * (phr * dr + phi * di);       // -(2/D^2) Re(conj(Phi) dPhi)
        else
            g = 2.0 * (phr * dr - phi * di);             // F = Re(z^2), z = conj(Phi): dF = 2 Re(z dz) = 2 Re(Phi dPhi)
        if (live)
            out[c + (size_t)t * K] = g;
    }
    if (live && t == Nsl - 1) {
        double F;
        if (SAND || p.objective == 1)
            F = 1.0 - D2 * (phr * phr + phi * phi);      // C1, src/cost_functions.jl:13-17
        else
            F = phr * phr - phi * phi;                   // Re(z^2), z = conj(Phi): src/cost_functions.jl:99-101
        out[(size_t)K * Nsl] = F;
    }
}

// ---- n = 2, 4: the same evaluation on LANE PAIRS (frechet.hpp: FrechetPair)
// W1IN (UnitaryGate, Hermitian generators -- round 4): the backward sweep of the unitary flow has left W_t = X_t L_{t+1}' in
// `states` and Phi = tr(L' X) per member in `zphi` (SweepParams::dump_w1): no P_t / X_t / L_{t+1} loads, two products less,
// and a sweep of 0.09 instead of 0.16 ms in front of this kernel.
template <int N, int SAND, bool W1IN = false>
__global__ __launch_bounds__(64) void exact_pair_kernel(const double2 *__restrict__ ops_all, const double *__restrict__ x_all,
                                                        const ExactParams p)
{
    constexpr int NN = N * N, NC = N / 2, NE = N * NC;
    const int k = blockIdx.y, lane = threadIdx.x, par = lane & 1;
    const int t = blockIdx.x * 32 + (lane >> 1);
    const int K = p.K, Nsl = p.N;
    const bool live = t < Nsl;
    const int tt = live ? t : Nsl - 1;                   // surplus pairs repeat the last slice (never stored)
    const double2 *__restrict__ ops = ops_all + (size_t)k * (K + 3) * NN;
    const double2 *__restrict__ opB = ops + NN;
    const double2 *__restrict__ opXt = ops + (size_t)(2 + K) * NN;
    int gidx[NE], gidx_t[NE];
    pair_indices<N>(par, gidx, gidx_t);
    auto ws_load = [&](PMat<N> &m, const double2 *__restrict__ ws, int slice) {
        const int L = slice / p.S, j = slice - L * p.S;
        const double2 *__restrict__ base = ws + ((size_t)k * p.S + j) * NN * p.CH + L;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const double2 v = base[(size_t)gidx[e] * p.CH];
            m.re[e] = v.x;
            m.im[e] = v.y;
        }
    };
    PMat<N> W1, W2;
    double phr, phi;
    if (W1IN) {
        ws_load(W1, p.states, tt);
        phr = p.zphi[2 * (size_t)k];
        phi = p.zphi[2 * (size_t)k + 1];
    } else {
        PMat<N> P, X, Ln, Lp, tmp, tp;
        ws_load(P, p.props, tt);
        ws_load(X, p.states, tt);
        if (tt + 1 < Nsl)
            ws_load(Ln, p.costates, tt + 1);             // costate after slice t
        else
            pair_op_load(Ln, opXt, gidx);
        fetch_partner(Lp, Ln);
        if (SAND) {
            PMat<N> Y, Pp, Xp;
            fetch_partner(Pp, P);
            fetch_partner(Xp, X);
            pmul_a_bh(Y, X, Xp, P, Pp);                  // X P'
            fetch_partner(tp, Y);
            pmul_a_bh(W1, Y, tp, Ln, Lp);                // X P' L'
            pmul(tmp, P, Pp, Y);                         // X_{t+1} = P X P'
            ptrace_ah_b(phr, phi, Ln, tmp);
            if (!p.herm_states) {
                pmul_ah_b(Y, P, Pp, Ln);                 // P' L
                pmul_ah_b(W2, X, Xp, Y);                 // X' P' L
            }
        } else {
            PMat<N> Xp;
            fetch_partner(Xp, X);
            pmul_a_bh(W1, X, Xp, Ln, Lp);                // X L'
            pmul_f(tmp, P, X);                           // X_{t+1} = P X
            ptrace_ah_b(phr, phi, Ln, tmp);
        }
    }
    // generator of this slice (the sweep's order of the sum) and the shared part of the Taylor-8 evaluation (frechet.hpp)
    FrechetPair<N> fr;
    build_generator_pair(fr.G, ops, opB, x_all + (size_t)tt * K, K, p.variant, gidx);
    fr.prepare(p.s_forced);
    double *__restrict__ out = p.member_out + (size_t)k * ((size_t)K * Nsl + 1);
    const double D2 = 1.0 / ((double)N * (double)N);
    PMat<N> D1, D2m;
    fr.apply(D1, W1);
    const bool second = SAND && !p.herm_states;          // Hermitian X, L: W2 == W1
    if (second)
        fr.apply(D2m, W2);
    for (int c = 0; c < K; ++c) {
        PMat<N> BT;                                      // B'_c transposed, in the pair layout: tr(D B) = sum D .* B^T
        pair_op_load(BT, opB + c * NN, gidx_t);
        double ar, ai, dr, di;
        ptrace_elem(ar, ai, D1, BT);
        dr = ar;
        di = ai;
        if (SAND) {
            if (second)
                ptrace_elem(ar, ai, D2m, BT);
            dr += ar;
            di -= ai;
        }
        double g;
        if (SAND || p.objective == 1)
            g = -2.0 * D2 * (phr * dr + phi * di);       // -(2/D^2) Re(conj(Phi) dPhi)
        else
            g = 2.0 * (phr * dr - phi * di);             // F = Re(z^2), z = conj(Phi): dF = 2 Re(Phi dPhi)
        if (live && par == 0)
            out[c + (size_t)t * K] = g;
    }
    if (live && par == 0 && t == Nsl - 1) {
        double F;
        if (SAND || p.objective == 1)
            F = 1.0 - D2 * (phr * phr + phi * phi);      // C1, src/cost_functions.jl:13-17
        else
            F = phr * phr - phi * phi;                   // Re(z^2), z = conj(Phi): src/cost_functions.jl:99-101
        out[(size_t)K * Nsl] = F;
    }
}

template <int N>
static hipError_t launch_exact_pair(int sandwich, const ExactParams &p, hipStream_t stream)
{
    const dim3 grid((p.N + 31) / 32, p.E), block(64);
    if (p.w1_in && sandwich) return hipErrorInvalidConfiguration;
    if (p.w1_in)       GRAPE_LAUNCH_AS("exact_pair_kernel", (exact_pair_kernel<N, 0, true>), grid, block, 0, stream, p.ops, p.x, p);
    else if (sandwich) GRAPE_LAUNCH((exact_pair_kernel<N, 1>), grid, block, 0, stream, p.ops, p.x, p);
    else               GRAPE_LAUNCH((exact_pair_kernel<N, 0>), grid, block, 0, stream, p.ops, p.x, p);
    return hipGetLastError();
}

template <int N>
static hipError_t launch_exact_n(int sandwich, const ExactParams &p, hipStream_t stream)
{
    const dim3 grid((p.N + 63) / 64, p.E), block(64);
    if (sandwich) GRAPE_LAUNCH((exact_grad_kernel<N, 1>), grid, block, 0, stream, p.ops, p.x, p);
    else          GRAPE_LAUNCH((exact_grad_kernel<N, 0>), grid, block, 0, stream, p.ops, p.x, p);
    return hipGetLastError();
}

hipError_t launch_exact_grad(int n, int sandwich, const ExactParams &p, hipStream_t stream)
{
    static const bool lane_env = std::getenv("GRAPE_EXACT_LANE") != nullptr;          // (the round-2 mapping, for comparison)
    const bool lane_kernel = lane_env && !p.w1_in;
    if (p.w1_in && n != 2 && n != 4) return hipErrorInvalidConfiguration;
    switch (n) {
    case 2: return lane_kernel ? launch_exact_n<2>(sandwich, p, stream) : launch_exact_pair<2>(sandwich, p, stream);
    case 3: return launch_exact_n<3>(sandwich, p, stream);
    case 4: return lane_kernel ? launch_exact_n<4>(sandwich, p, stream) : launch_exact_pair<4>(sandwich, p, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace grape
