// observe.hip -- expectation values along the trajectory (grape_eval_observables; what the reference names and leaves
// undone: test_pulse, src/tools.jl:32-36, and visualise_expt_val(s), src/visualisation.jl:13-51) for the small-n family
// (n = 2, 3, 4) on gfx950.
//
//   y[s, j, k] = tr(O_kj' X_{k,s}) ,  s = 0..N ,  X_{k,0} = Xi_k
//   UnitaryGate (n x m states, kets included):  X_{s+1} = P_s X_s          StateTransfer / CoherenceTransfer:  X_{s+1} = P_s X_s P_s'
//
// It runs behind the sweep of the same launch (and behind the running-cost kernels, if any) and reads the propagators P_t
// that sweep left in the workspace (chunk-major: element e of slice t = c S + jj of member k at ((k S + jj) n^2 + e) CH + c).
// The decomposition and the steps marked * are traj_chunk.hpp's: one workgroup per member of the launch, one lane per time
// chunk of S consecutive slices, so every workspace access is lane-contiguous:
//   1* chunk product Q_c = P_hi-1 ... P_lo
//   2* exclusive prefix scan of the Q_c over lanes (wave shuffles in a fixed tree, wave totals through LDS, combined in wave
//      order): U_start, the cumulative propagator at the chunk start
//   3  X = U_start Xi [U_start'], then the walk X <- P_t X [P_t'] over the chunk (P read a second time)
//   4  behind every slice the n_obs traces*, one probe at a time (the probes are wave-uniform: scalar loads), stored to y
//   5  lane 0 also stores the s = 0 entry, the lane that owns slice N - 1 stores X_N
// Ragged decompositions: a lane whose chunk starts at or behind N, and the padding lanes behind chunk CH - 1, own no slice
// (Q = 1, nothing stored); the last chunk may be short.  Plain vector stores, no atomics; every number has one fixed
// evaluation order, so results are bitwise reproducible and a member-chunked launch gives the bits of an unchunked one.
//
// STAGED (observe_staged_kernel; the device forms, SweepParams::obs_staged): a member's y block is ONE contiguous run of
// n_obs (N + 1) entries in the caller's layout, but lane c stores at s = c S + jj: neighbouring lanes are S 16 B apart within a
// probe row, every wave store touches 64 sectors.  The staged instance writes the same values into an LDS image of the block
// at [j][s] (lane 0's s = 0 entries included), and behind ONE barrier behind the walk -- reached by every lane, whatever its
// cnt -- the workgroup streams the image out with lane-contiguous 16 B stores.  Same arithmetic, same order, same bits.
#include "cmat.hpp"
#include "grape_kernels.hpp"
#include "rc_mat.hpp"
#include "traj_chunk.hpp"

namespace grape {

// C = X P^H  (the right half of the sandwich; all n x n)
template <int N>
GRAPE_DEV void rmul_x_ph(CRect<N, N> &c, const CRect<N, N> &x, const CMat<N> &p)
{
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double ar = x.re[i + k * N], ai = x.im[i + k * N];
                const double br = p.re[j + k * N], bi = -p.im[j + k * N];
                sr = fma(ar, br, sr);
                sr = fma(-ai, bi, sr);
                si = fma(ar, bi, si);
                si = fma(ai, br, si);
            }
            c.re[i + j * N] = sr;
            c.im[i + j * N] = si;
        }
}

// X <- U X (UnitaryGate) or U X U' (sandwich; M == N)
template <int N, int M, bool SAND>
GRAPE_DEV void obs_apply(CRect<N, M> &X, const CMat<N> &U)
{
    CRect<N, M> Tm;
    rmul(Tm, U, X);
    if constexpr (SAND)
        rmul_x_ph(X, Tm, U);
    else
        X = Tm;
}

// ops_all / o_all are separate `const __restrict__` arguments so that the wave-uniform operator and probe entries can be
// fetched with scalar loads (as in sweep_small.hip and running_cost.hip)
template <int N, int M, bool SAND, int MAXT, bool STAGED>
__global__ __launch_bounds__(MAXT) void observe_kernel(const double2 *__restrict__ ops_all, const double2 *__restrict__ o_all,
                                                       const SweepParams p)
{
    static_assert(!SAND || M == N, "the sandwich acts on n x n states");
    constexpr int NN = N * N, NM = N * M, MAXW = MAXT / 64;
    __shared__ double2 s_q[MAXW][NN];              // wave totals of the prefix scan
    extern __shared__ double2 s_img[];             // STAGED: the member's y block, [j][s] as the caller lays it out

    const int Nsl = p.N, n_obs = p.obs_n;
    const int k = blockIdx.x;                        // member within the launch: row of the workspace
    const int kg = k + p.obs_E0;                     // member of the ensemble: row of the probes and of the outputs
    const TrajLane<N> ln = traj_lane<N>(p.obs_CH, p.S, Nsl, p.props, k);
    const int L = ln.L, lo = ln.lo, hi = ln.hi, cnt = ln.cnt;
    const TrajProbes pr = traj_probes<N, M>(o_all, p.obs_per_member, p.obs_Etot, kg, Nsl);
    double2 *__restrict__ yk = p.obs_y ? p.obs_y + (size_t)kg * n_obs * pr.y_step : nullptr;

    // ---------------------------------------------------------------- 1, 2: chunk product, U at the chunk start
    CMat<N> P, U;
    {
        CMat<N> Q;
        traj_chunk_product(Q, ln);
        traj_prefix_start(U, Q, ln, s_q);
    }
    // ---------------------------------------------------------------- 3: the state at the chunk start
    CRect<N, M> X;
    rload_uniform(X, traj_ops<N>(ops_all, k, p.K).opXi);
    obs_apply<N, M, SAND>(X, U);

    // the n_obs traces y_j = tr(O_j' X) of the state behind s slices, one probe at a time
    auto emit = [&](int s) {
        for (int j = 0; j < n_obs; ++j) {
            const double2 y = traj_probe_trace(pr.probe(j), X);
            if constexpr (STAGED)
                s_img[s + j * (Nsl + 1)] = y;
            else
                yk[(size_t)s + (size_t)j * pr.y_step] = y;
        }
    };
    if (yk && L == 0)
        emit(0);                                     // (U_start = 1: X is Xi)
    // ---------------------------------------------------------------- 4: the walk
    for (int jj = 0; jj < cnt; ++jj) {
        rc_load_mat(P, ln.P(jj), ln.stride);
        obs_apply<N, M, SAND>(X, P);
        if (yk)
            emit(lo + jj + 1);
    }
    if constexpr (STAGED) {                          // the image -> y, lane-contiguous (every lane reaches the barrier)
        __syncthreads();
        if (yk) {
            const int tot = n_obs * (Nsl + 1);
            for (int i = L; i < tot; i += (int)blockDim.x)
                yk[i] = s_img[i];
        }
    }
    // ---------------------------------------------------------------- 5: X_N
    if (p.obs_xf && cnt > 0 && hi == Nsl) {
        double2 *__restrict__ xf = p.obs_xf + (size_t)kg * NM;
#pragma unroll
        for (int e = 0; e < NM; ++e)
            xf[e] = make_double2(X.re[e], X.im[e]);
    }
}

template <int N, int M, bool SAND>
static hipError_t obs_launch_nm(const SweepParams &p, hipStream_t stream)
{
    constexpr int MAXT = RcTraits<N>::MAXT;
    const int threads = (p.obs_CH + 63) & ~63;
    if (threads > MAXT || p.obs_CH < 1 || (long long)p.S * p.obs_CH < p.N || p.N < 1 || p.E < 1 || p.obs_E0 < 0 ||
        p.obs_E0 + p.E > p.obs_Etot || p.obs_n < 0 || p.obs_n > 16 || (!p.obs_y && !p.obs_xf) ||
        (p.obs_y && p.obs_n > 0 && !p.obs_O) || !p.props || !p.ops)
        return hipErrorInvalidConfiguration;
    if (p.obs_staged) {
        // the image is exactly the member's block, and static + dynamic LDS fit a workgroup of this device
        const auto kern = observe_kernel<N, M, SAND, MAXT, true>;
        const size_t lds = (size_t)p.obs_staged;
        if (!p.obs_y || p.obs_n < 1 || lds != sizeof(double2) * (size_t)p.obs_n * ((size_t)p.N + 1))
            return hipErrorInvalidConfiguration;
        int dev = 0, cap = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        if (e != hipSuccess) return e;
        if (lds + traj_static_lds(N, M, false) > (size_t)cap) return hipErrorInvalidConfiguration;
        e = ensure_dynamic_lds((const void *)kern, lds);
        if (e != hipSuccess) return e;
        GRAPE_LAUNCH_AS("observe_staged_kernel", kern, dim3(p.E), dim3(threads), lds, stream, p.ops, p.obs_O, p);
        return hipGetLastError();
    }
    GRAPE_LAUNCH_AS("observe_kernel", (observe_kernel<N, M, SAND, MAXT, false>), dim3(p.E), dim3(threads), 0, stream, p.ops, p.obs_O, p);
    return hipGetLastError();
}

hipError_t run_observe(int n, int sandwich, const SweepParams &p, hipStream_t stream)
{
    if (sandwich) {
        if (p.obs_m != n)
            return hipErrorInvalidValue;
        switch (n) {
        case 2: return obs_launch_nm<2, 2, true>(p, stream);
        case 3: return obs_launch_nm<3, 3, true>(p, stream);
        case 4: return obs_launch_nm<4, 4, true>(p, stream);
        default: return hipErrorInvalidValue;
        }
    }
    return dispatch_nm(n, p.obs_m, [&](auto N, auto M) {
        return obs_launch_nm<decltype(N)::value, decltype(M)::value, false>(p, stream);
    });
}

}  // namespace grape
