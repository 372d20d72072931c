// The two kernels of the ensemble-averaged trajectory calls (csrc/traj_mean.hip) alone, from HIP events: the member reduction
// (traj_mean_reduce_kernel + traj_mean_combine_kernel) and the cotangent broadcast (traj_mean_broadcast_kernel) at the headline
// shape -- N = 500, E = 1024, n x m = 4 x 4 -- for 1, 4 and 16 probes, through the launcher the library uses.  Both are
// memory-bound: they touch 16 (N + 1) n_obs E bytes once (plus the final states), so bytes / time is printed next to the time.
// Blocks of back-to-back launches behind a warm-up block; per variant the median of the block means and half the 10 .. 90 %
// range between blocks.  tools/traj_mean_time.py runs this program and copies its lines.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-fast-math -ffp-contract=on traj_mean_rate.hip -o traj_mean_rate
#include "../../quoptimalcontrol.jl_amd/csrc/traj_mean.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace grape {
void log_kernel(const char *) {}
}  // namespace grape

#define CHECK(call)                                                                   \
    do {                                                                              \
        hipError_t e__ = (call);                                                      \
        if (e__ != hipSuccess) {                                                      \
            std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e__));          \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static void stats(std::vector<double> t, double &med, double &spread)
{
    std::sort(t.begin(), t.end());
    const size_t n = t.size();
    med = n % 2 ? t[n / 2] : 0.5 * (t[n / 2 - 1] + t[n / 2]);
    spread = 0.5 * (t[(size_t)(0.9 * (n - 1) + 0.5)] - t[(size_t)(0.1 * (n - 1) + 0.5)]);
}

int main(int argc, char **argv)
{
    const int blocks = argc > 1 ? std::atoi(argv[1]) : 15, calls = argc > 2 ? std::atoi(argv[2]) : 50;
    const int N = 500, E = 1024, nm = 16;
    const int probes[3] = {1, 4, 16};
    const size_t Lmax = (size_t)(N + 1) * 16, nseg = (E + grape::kMeanSeg - 1) / grape::kMeanSeg;
    double2 *y, *xf, *io, *part;
    double *v;
    CHECK(hipMalloc((void **)&y, sizeof(double2) * Lmax * E));
    CHECK(hipMalloc((void **)&xf, sizeof(double2) * nm * E));
    CHECK(hipMalloc((void **)&io, sizeof(double2) * (Lmax + nm)));
    CHECK(hipMalloc((void **)&part, sizeof(double2) * (Lmax + nm) * nseg));
    CHECK(hipMalloc((void **)&v, sizeof(double) * E));
    {
        std::vector<double> h(2 * Lmax * E);
        for (size_t i = 0; i < h.size(); ++i) h[i] = 1e-3 * (double)(i % 1009) - 0.5;
        CHECK(hipMemcpy(y, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(xf, h.data(), sizeof(double2) * nm * E, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(io, h.data(), sizeof(double2) * (Lmax + nm), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(v, h.data(), sizeof(double) * E, hipMemcpyHostToDevice));
    }
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::printf("# tools/ubench/traj_mean_rate: N=%d E=%d n x m=%d, %d blocks of %d launches behind a warm-up block, HIP events; us: median of "
                "the block means +- half the 10..90 %% range between blocks\n", N, E, nm, blocks, calls);
    for (int pi = 0; pi < 3; ++pi) {
        grape::MeanOp red, bc;
        red.E = bc.E = E;
        red.v = bc.v = v;
        red.L[0] = bc.L[0] = (long long)(N + 1) * probes[pi];
        red.L[1] = bc.L[1] = nm;
        red.src[0] = y;
        red.src[1] = xf;
        red.out = io;
        red.part = part;
        bc.broadcast = 1;
        bc.in = io;
        bc.dst[0] = y;
        bc.dst[1] = xf;
        const double bytes = 16.0 * (double)(red.L[0] + red.L[1]) * E;
        std::vector<double> t[2];
        for (int b = 0; b <= blocks; ++b)
            for (int which = 0; which < 2; ++which) {            // alternating
                const grape::MeanOp &op = which ? bc : red;
                CHECK(grape::run_traj_mean(op, nullptr));
                CHECK(hipDeviceSynchronize());
                CHECK(hipEventRecord(e0, nullptr));
                for (int c = 0; c < calls; ++c)
                    CHECK(grape::run_traj_mean(op, nullptr));
                CHECK(hipEventRecord(e1, nullptr));
                CHECK(hipEventSynchronize(e1));
                float ms = 0.f;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (b)
                    t[which].push_back(1e3 * ms / calls);
            }
        for (int which = 0; which < 2; ++which) {
            double med, sp;
            stats(t[which], med, sp);
            std::printf("kernels alone n_obs=%-2d %-42s %7.2f +- %5.2f us   %6.1f MB touched once   %6.2f TB/s\n", probes[pi],
                        which ? "broadcast (traj_mean_broadcast_kernel):" : "reduction (traj_mean_reduce + _combine):", med, sp,
                        bytes / 1e6, bytes / (med * 1e-6) / 1e12);
        }
    }
    return 0;
}
