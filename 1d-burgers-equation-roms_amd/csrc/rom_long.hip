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
// LDS: 8 B per mesh row for each of u, g, h_f, dt F (32 KB at 1024 rows), the coefficients of ONE slab (2 KB), two slabs
// of 66 x 42 doubles (43.3 KB) -- 77.7 KB, so two workgroups share a compute unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rom_fused_device.hpp"
#include "rom_stream_device.hpp"

namespace {

using namespace bg;

constexpr int LNMAX = 1024;            // mesh rows
constexpr int LR = 40;                 // padded reduced dimension: column 10 t + c  <->  (lane index t, block c)
constexpr int LNB = 10;                // 4-column blocks
constexpr int LPS = 42;                // doubles per row of the LDS slabs (16-byte aligned rows)
constexpr int LSW = LR + 4;            // doubles per row of the parked system: Ar | br | Phi^T u
#ifndef BG_LONG_WG_PER_CU
#define BG_LONG_WG_PER_CU 2
#endif
constexpr int LWG_PER_CU = BG_LONG_WG_PER_CU;

struct LongPod {
    static constexpr int NB = LNB, PS = LPS, SW = LSW, NMAX = LNMAX;
    static constexpr bool cf_by_mesh_row = false;       // lo, di, up, R of the slab at hand only: 2 KB instead of 32
    static constexpr bool mirror_lspg = true;           // the solves read the system through a plain accessor
    static constexpr bool has_repair = true;
    static constexpr bool timing = false;

    // solve(Ar, -br) (:767) by rom_fused_device.hpp's routines, one value of dq and q per lane.  BG_OPT_FORCE_PIVOTED: the
    // entry point skips the fast launch and the repair kernel takes every sample.
    template <bool GAL, bool PIV, int W, class Lap>
    static __device__ __forceinline__ void solve_update(const StreamRunArgs& a, const StreamLds& L, int lane, bool& aborted, int& info_out,
                                                        double& nd, double& nq, const Lap&)
    {
        const double* S = L.slab;
        const int r = a.r;
        const double wtu = (lane < r) ? S[lane * LSW + LR + 1] : 0.0;            // Phi^T u
        auto entry = [&](int i, int j) -> double { return S[i * LSW + j]; };      // (Ar | br)[i][j]
        double xout;
        if constexpr (PIV) {
            if (W == 0) fused::pivoted_solve_of<LNB>(entry, L.x, &L.bad[4], lane, r);
            __syncthreads();
            xout = (lane < LR) ? L.x[lane] : 0.0;
            if (L.bad[4] != 0 && info_out == 0) info_out = L.bad[4];
        } else {
            bool tripped;
            xout = fused::coop_gj_solve_of<LNB>(entry, reinterpret_cast<double (*)[4][64]>(L.m), L.diag, L.y, L.bad, W, lane, r, tripped);
            if (tripped) aborted = true;
        }
        const double dq = (lane < r) ? xout : 0.0;
        const double qn = wtu + dq;
        wave_sum2(dq * dq, qn * qn, nd, nq);
        if (W == 0 && lane < LR) L.q[lane] = qn;
    }
};

// The repair kernel (PIV) keeps one workgroup per CU: its one-wave pivoted solve holds a 41-double row per lane.
template <bool GAL, bool PIV>
__global__ __launch_bounds__(256, PIV ? 1 : LWG_PER_CU) void rom_long_kernel(StreamRunArgs a)
{
    constexpr int SLAB = StreamDims<LongPod>::SLAB;
    __shared__ __attribute__((aligned(16))) double s_slab[2 * SLAB];              // two slab buffers; later the system
    __shared__ __attribute__((aligned(16))) double s_u[LNMAX + 4];                // u at offset 2, zero halo on each side
    __shared__ double s_g[LNMAX], s_h[LNMAX], s_fdt[LNMAX];
    __shared__ __attribute__((aligned(16))) double s_cf[SRS][4];                  // lo, di, up, R per row of the slab
    __shared__ __attribute__((aligned(16))) double s_q[LR];
    __shared__ int s_bad[8];                                                      // [4] guard of each wave, [4] info of the pivoted solve
    static_assert(sizeof(double) * (2 * SLAB + LNMAX + 4 + 3 * LNMAX + 4 * SRS + LR) + 32 <= 160 * 1024 / LWG_PER_CU, "LDS per workgroup");
    // over the dead slabs: the system [LR][LSW], then the multipliers of two panels, the diagonal, y and x
    double* const s_m = s_slab + LR * LSW;
    double* const s_diag = s_m + 512;
    static_assert(LR * LSW + 512 + 3 * 64 <= 2 * SLAB, "the solve's arrays fit over the slabs");
    rom_stream_waves<LongPod, GAL, PIV>(a, StreamLds{s_slab, s_u, s_g, s_h, s_fdt, s_cf, s_q, s_m, s_diag, s_diag + 64, s_diag + 128, s_bad});
}

template <bool PIV>
void launch_long(int projection, int grid, hipStream_t st, const StreamRunArgs& a)
{
    if (projection == BG_PROJ_GALERKIN)
        hipLaunchKernelGGL((rom_long_kernel<true, PIV>), dim3(grid), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((rom_long_kernel<false, PIV>), dim3(grid), dim3(256), 0, st, a);
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
    const int cus = device_cu_count();
    const int grid = B < LWG_PER_CU * cus ? B : LWG_PER_CU * cus;
    const int grid_repair = B < cus ? B : cus;
    hipStream_t st = (hipStream_t)stream;
    if (!a.force_pivoted) {
        launch_long<false>(projection, grid, st, a);
        const int rc_fast = check_launch();
        if (rc_fast != BG_OK) return rc_fast;
    }
    launch_long<true>(projection, grid_repair, st, a);         // every workgroup leaves at once unless a sample is marked
    return check_launch();
}

}  // extern "C"
