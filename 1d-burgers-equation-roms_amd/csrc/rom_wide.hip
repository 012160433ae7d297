// rom_wide.hip -- the whole POD-PROM time loop of one sample on one compute unit for the thesis' LARGER bases, 40 < r <= 96
// (bg_rom_run_wide).  reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785; the bases are
// POD/modes/U_modes_tol_1e-04.npy (r = 96) and smaller, driven by POD/Results_thesis/prom_pod.py:35-58.
//
// The loop is rom_stream_device.hpp's (the basis streams through LDS, the accumulators of the reduced system stay in
// registers: LSPG 348 items, 87 per wave; Galerkin 600, 150 per wave; one pass over Phi per Picard iteration, L2-resident:
// 393 KB at r = 96; twelve 16-byte reads per row and 24 blocks).  What is this kernel's own is the description WidePod and
// the 96 x 96 solve by all four waves -- bg_rom_run's guarded pivot-free Gauss-Jordan on two row tiles (rows 0-63 and
// 64-95 of a column live in two registers of lane = row mod 64; wave w owns the 4-column blocks b = w mod 4), one panel
// of four columns at a time.  A sample whose elimination meets a multiplier above 1 (np.linalg.solve would have exchanged rows)
// is marked BG_INFO_NEEDS_PIVOTING and redone by the caller through the library path (burgers_hip/rom.py does).
// The solve and the description are rom_wide_device.hpp's (shared with the loop for long meshes, rom_long_wide.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rom_wide_device.hpp"

namespace {

using namespace bg;

template <bool GAL>
__global__ __launch_bounds__(256, 1) void rom_wide_kernel(StreamRunArgs a)
{
    constexpr int SLAB = StreamDims<WidePod>::SLAB;
    __shared__ __attribute__((aligned(16))) double s_slab[2 * SLAB + 128];       // two slab buffers (+ slack of the last DMA piece); later the system
    __shared__ __attribute__((aligned(16))) double s_u[WNMAX + 4];                // u at offset 2, zero halo on each side
    __shared__ double s_g[WNMAX], s_h[WNMAX], s_fdt[WNMAX];
    __shared__ __attribute__((aligned(16))) double s_cf[WNMAX][4];                // lo, di, up, R per mesh row
    __shared__ __attribute__((aligned(16))) double s_q[WR];
    __shared__ double s_m[8][WR];                                                 // multipliers of the current and the next panel
    __shared__ double s_diag[WR], s_y[WR];
    __shared__ int s_bad[4];
    rom_stream_waves<WidePod, GAL, false>(a, StreamLds{s_slab, s_u, s_g, s_h, s_fdt, s_cf, s_q, &s_m[0][0], s_diag, s_y, nullptr, s_bad});
}

}  // namespace

extern "C" {

int bg_rom_run_wide_max_r(void) { return WR; }

// doubles of the padded basis copy bg_rom_run_wide reads: (NPAD + 2) rows of 96, NPAD = N rounded up to 64
long long bg_rom_run_wide_phi_elems(int N) { return N < 2 ? 0 : (long long)(((N + 63) / 64) * 64 + 2) * WR; }

int bg_rom_run_wide(int N, int B, int r, int nsteps, int projection, const double* x, const double* PhiP, const double* u0,
                    const double* mu1, const double* mu2, double dt, double E, double tol, int max_it, int options,
                    double* hist, int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    StreamRunArgs a;
    const int rc = stream_run_args(a, 2, WNMAX, WR, N, B, r, nsteps, projection, x, PhiP, u0, mu1, mu2, dt, E, tol, max_it, options,
                                   hist, iters, flags, info, order);
    if (rc != BG_OK || B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        hipLaunchKernelGGL((rom_wide_kernel<decltype(p)::galerkin>), dim3(persistent_grid(B, 1)), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
