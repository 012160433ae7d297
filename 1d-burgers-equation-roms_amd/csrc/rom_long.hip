// rom_long.hip -- the whole POD-PROM time loop of one sample on one compute unit for LONG meshes, 513 <= N <= 1024, with
// bases of up to 40 modes (bg_rom_run_long).  reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785.
//
// bg_rom_run (rom_fused.hip) keeps the basis in registers, 2 (N / 64) (r / 4) of them per lane: 160 at N = 512, 320 at
// N = 1024.  Here the basis streams through LDS: the loop is rom_stream_device.hpp's, from the padded copy PhiP
// [NPAD + 2][40] (one pass over it per Picard iteration, L2-resident: 328 KB at N = 1024; Galerkin 110 items: 28 per wave;
// LSPG 75: 19 per wave; five 16-byte reads per row).  What is this kernel's own is the description LongPod:
// the reduced system is parked WHOLE in LDS over the dead slabs (LSPG: the lower block pairs mirrored on the way) and
// solved by rom_fused_device.hpp's routines: the guarded pivot-free Gauss-Jordan of all four waves in the fast kernel; a
// sample in which a multiplier below the diagonal exceeds 1 or a pivot is 0 (np.linalg.solve would have exchanged rows)
// is marked and redone from u0 by the repair instantiation (PIV: one-wave partial pivoting) launched behind the fast one,
// as in bg_rom_run.
// The layout, the solve and the kernel body are rom_long_device.hpp's (shared with the local POD loop, rom_local_long.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rom_long_device.hpp"

namespace {

using namespace bg;

struct LongPod : LongLayout {
    using Args = StreamRunArgs;
    static constexpr bool local = false;
};

// The repair kernel (PIV) keeps one workgroup per CU: its one-wave pivoted solve holds a 41-double row per lane.
template <bool GAL, bool PIV>
__global__ __launch_bounds__(256, PIV ? 1 : LWG_PER_CU) void rom_long_kernel(StreamRunArgs a)
{
    BG_LONG_KERNEL_BODY(LongPod, 0);
}

}  // namespace

extern "C" {

int bg_rom_run_long_max_n(void) { return LNMAX; }
int bg_rom_run_long_max_r(void) { return LR; }
int bg_rom_run_long_workgroups_per_cu(void) { return LWG_PER_CU; }

// doubles of the padded basis copy bg_rom_run_long reads: (NPAD + 2) rows of 40, NPAD = N rounded up to 64 (any r <= 40)
long long bg_rom_run_long_phi_elems(int N, int r)
{
    if (N < 3 || N > LNMAX || r < 1 || r > LR) return 0;
    return (long long)(((N + SRS - 1) / SRS) * SRS + 2) * LR;
}

int bg_rom_run_long(int N, int B, int r, int nsteps, int projection, const double* x, const double* PhiP, const double* u0,
                    const double* mu1, const double* mu2, double dt, double E, double tol, int max_it, int options,
                    double* hist, int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    StreamRunArgs a;
    const int rc = stream_run_args(a, 3, LNMAX, LR, N, B, r, nsteps, projection, x, PhiP, u0, mu1, mu2, dt, E, tol, max_it, options,
                                   hist, iters, flags, info, order);
    if (rc != BG_OK || B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        return launch_fast_then_repair(B, LWG_PER_CU, a.force_pivoted != 0, [&](auto piv, int grid) {
            hipLaunchKernelGGL((rom_long_kernel<decltype(p)::galerkin, decltype(piv)::value>), dim3(grid), dim3(256), 0, st, a);
        });
    });
}

}  // extern "C"
