// rom_local_long.hip -- the whole local POD-PROM time loop of one sample on one compute unit for LONG meshes,
// 513 <= N <= 1024, with local bases of up to 40 modes (bg_local_rom_run_long).  reference: FEMBurgers.local_prom_burgers,
// FEM/fem_burgers.py:979-1079.
//
// bg_local_rom_run (rom_fused.hip, LOCAL) keeps the step's basis in registers and reloads it when the cluster changes; it
// stops at N = 512.  Here the basis streams through LDS as in bg_rom_run_long: the loop is rom_stream_device.hpp's with the
// description LongLocal = rom_long_device.hpp's layout plus `local`: at the top of every time step the nearest centre to
// q_g = U_g^T u^n (the arithmetic of bg_local_rom_run) picks a block of the stack
// bases [C][NPAD + 2][40] and a width, and every sweep of that step streams that block.  The sweep re-reads the basis from L2
// on every pass anyway, so a switch costs nothing beyond the pick, and it forms q = Phi^T u + dq, which is what the first
// iteration after a switch needs (u^n is not in the new span).  The solves give the unknowns at and beyond the width a zero
// correction (LongLayout::solve_update).  Fast and repair instantiations as in rom_long.hip; the repair kernel redoes a
// marked sample from u0 and so follows the same cluster path.
// LDS: rom_long_device.hpp's 77.7 KB + 64 doubles for q_g: two workgroups per compute unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rom_long_device.hpp"

namespace {

using namespace bg;

constexpr int LMAXM = 64;              // global modes of the cluster pick: the length of q_g in LDS
constexpr int LMAXC = 64;              // centres: one lane each in the nearest-centre pick

struct LongLocal : LongLayout {
    using Args = LocalStreamRunArgs;
    static constexpr bool local = true;
};

// The repair kernel (PIV) keeps one workgroup per CU: its one-wave pivoted solve holds a 41-double row per lane.
template <bool GAL, bool PIV>
__global__ __launch_bounds__(256, PIV ? 1 : LWG_PER_CU) void rom_local_long_kernel(LocalStreamRunArgs a)
{
    BG_LONG_KERNEL_BODY(LongLocal, LMAXM);
}

}  // namespace

extern "C" {

int bg_local_rom_run_long_limits(int* max_n, int* max_r, int* max_m, int* max_clusters)
{
    if (max_n) *max_n = LNMAX;
    if (max_r) *max_r = LR;
    if (max_m) *max_m = LMAXM;
    if (max_clusters) *max_clusters = LMAXC;
    return BG_OK;
}

// doubles of the stack bg_local_rom_run_long reads: C blocks of (NPAD + 2) rows of 40, NPAD = N rounded up to 64
long long bg_local_rom_run_long_bases_elems(int N, int C)
{
    if (N < 3 || N > LNMAX || C < 1 || C > LMAXC) return 0;
    return (long long)C * (((N + SRS - 1) / SRS) * SRS + 2) * LR;
}

int bg_local_rom_run_long(int N, int B, int C, int rmax, int m, int nsteps, int projection, const double* x,
                          const double* bases, const int32_t* widths, const double* UgT, const double* centres,
                          const double* u0, const double* mu1, const double* mu2, double dt, double E, double tol,
                          int max_it, int options, double* hist, int32_t* iters, int32_t* flags, int32_t* info,
                          int32_t* clusters, const int32_t* order, void* stream)
{
    if (C < 1 || m < 1) return BG_ERR_BAD_ARG;
    LocalStreamRunArgs a;
    const int rc = stream_run_args(a, 3, LNMAX, LR, N, B, rmax, nsteps, projection, x, bases, u0, mu1, mu2, dt, E, tol, max_it,
                                   options, hist, iters, flags, info, order);
    if (rc != BG_OK) return rc;
    if (m > LMAXM || C > LMAXC) return BG_ERR_UNSUPPORTED_R;
    if (B == 0) return BG_OK;
    if (!widths || !UgT || !centres) return BG_ERR_BAD_ARG;
    a.widths = widths; a.UgT = UgT; a.centres = centres; a.clusters = clusters; a.C = C; a.m = m;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        return launch_fast_then_repair(B, LWG_PER_CU, a.force_pivoted != 0, [&](auto piv, int grid) {
            hipLaunchKernelGGL((rom_local_long_kernel<decltype(p)::galerkin, decltype(piv)::value>), dim3(grid), dim3(256), 0, st, a);
        });
    });
}

}  // extern "C"
