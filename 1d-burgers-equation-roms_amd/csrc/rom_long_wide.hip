// rom_long_wide.hip -- the whole POD-PROM time loop of one sample on one compute unit for LONG meshes, 513 <= N <= 1024,
// with the thesis' LARGER bases, 40 < r <= 96 (bg_rom_run_long_wide).  reference: FEMBurgers.pod_prom_burgers,
// FEM/fem_burgers.py:709-785.
//
// The loop is rom_stream_device.hpp's, the 96 x 96 solve and the hand-back of marked samples are rom_wide_device.hpp's
// (bg_rom_run_wide's: guarded pivot-free Gauss-Jordan by all four waves; a sample whose elimination meets a multiplier
// above 1 or a zero pivot is marked BG_INFO_NEEDS_PIVOTING and redone by the caller; there is no repair kernel).  What is
// this kernel's own is the description LongWidePod: WidePod with bg_rom_run_long's length -- 1024 mesh rows of u, g, h_f and
// dt F in LDS and the coefficients lo, di, up, R of ONE slab (2 KB) instead of every mesh row's (which would be 32 KB).
// One pass over PhiP [NPAD + 2][96] per Picard iteration, L2-resident: 788 KB at N = 1024.
// LDS: two slabs of 66 x 98 doubles + 1 KB slack (104 512 B), u (8 224 B), g, h_f, dt F (24 576 B), the slab's coefficients
// (2 048 B), q (768 B), the multipliers of two panels (6 144 B), the diagonal and y (1 536 B), the guards (16 B):
// 147 824 B of 163 840 B, one workgroup per compute unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rom_wide_device.hpp"

namespace {

using namespace bg;

constexpr int LWNMAX = 1024;           // mesh rows

struct LongWidePod : WidePod {
    static constexpr int NMAX = LWNMAX;
    static constexpr bool cf_by_mesh_row = false;       // lo, di, up, R of the slab at hand only: 2 KB instead of 32
};

template <bool GAL>
__global__ __launch_bounds__(256, 1) void rom_long_wide_kernel(StreamRunArgs a)
{
    constexpr int SLAB = StreamDims<LongWidePod>::SLAB;
    __shared__ __attribute__((aligned(16))) double s_slab[2 * SLAB + 128];       // two slab buffers (+ slack of the last DMA piece); later the system
    __shared__ __attribute__((aligned(16))) double s_u[LWNMAX + 4];               // u at offset 2, zero halo on each side
    __shared__ double s_g[LWNMAX], s_h[LWNMAX], s_fdt[LWNMAX];
    __shared__ __attribute__((aligned(16))) double s_cf[SRS][4];                  // lo, di, up, R per row of the slab
    __shared__ __attribute__((aligned(16))) double s_q[WR];
    __shared__ double s_m[8][WR];                                                 // multipliers of the current and the next panel
    __shared__ double s_diag[WR], s_y[WR];
    __shared__ int s_bad[4];
    static_assert(sizeof(double) * (2 * SLAB + 128 + LWNMAX + 4 + 3 * LWNMAX + 4 * SRS + WR + 8 * WR + 2 * WR) + 16 <= 160 * 1024,
                  "LDS per workgroup");
    static_assert(WR * WPS <= 2 * SLAB, "the parked system fits over the slabs");
    rom_stream_waves<LongWidePod, GAL, false>(a, StreamLds{s_slab, s_u, s_g, s_h, s_fdt, s_cf, s_q, &s_m[0][0], s_diag, s_y, nullptr, s_bad});
}

}  // namespace

extern "C" {

int bg_rom_run_long_wide_max_n(void) { return LWNMAX; }
int bg_rom_run_long_wide_max_r(void) { return WR; }

// doubles of the padded basis copy bg_rom_run_long_wide reads: (NPAD + 2) rows of 96, NPAD = N rounded up to 64
long long bg_rom_run_long_wide_phi_elems(int N)
{
    if (N < 3 || N > LWNMAX) return 0;
    return (long long)(((N + SRS - 1) / SRS) * SRS + 2) * WR;
}

int bg_rom_run_long_wide(int N, int B, int r, int nsteps, int projection, const double* x, const double* PhiP, const double* u0,
                         const double* mu1, const double* mu2, double dt, double E, double tol, int max_it, int options,
                         double* hist, int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    StreamRunArgs a;
    const int rc = stream_run_args(a, 3, LWNMAX, WR, N, B, r, nsteps, projection, x, PhiP, u0, mu1, mu2, dt, E, tol, max_it, options,
                                   hist, iters, flags, info, order);
    if (rc != BG_OK || B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        hipLaunchKernelGGL((rom_long_wide_kernel<decltype(p)::galerkin>), dim3(persistent_grid(B, 1)), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
