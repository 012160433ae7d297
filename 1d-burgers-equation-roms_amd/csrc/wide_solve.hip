// wide_solve.hip -- bg_wide_solve_pivoted: a batch of dense systems of up to 96 unknowns, each solved by one workgroup of four
// waves with rom_wide_device.hpp's wide_solve_pivoted (Gauss-Jordan with partial pivoting as an implicit permutation), the
// repair solve of bg_hyper_rom_run_wide.  The entry point pins that routine on inputs a time loop cannot be steered to, and is
// the batched pivoted solve for 65 <= n <= 96.
//
// A system is parked in LDS as the loops park theirs: row i of (A | -b) at S[98 i], the right-hand side in column 96 with its
// sign turned, since the routine solves for the loops' solve(Ar, -br).  Rows and columns at and beyond n are never written:
// the routine reads them as identity.  LDS: the system (75 264 B), the multipliers of two panels (6 144 B), the diagonal and
// y (1 536 B), pivot rows, info and the permutation (448 B): 83 392 B, one workgroup per compute unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "abi_common.hpp"
#include "rom_device.hpp"
#include "rom_wide_device.hpp"

namespace {

using namespace bg;

__global__ __launch_bounds__(256, 1) void wide_solve_pivoted_kernel(int B, int n, const double* A, const double* b, double* x, int32_t* piv,
                                                                    int32_t* info)
{
    __shared__ __attribute__((aligned(16))) double s_S[WR * WPS];
    __shared__ double s_m[8][WR];
    __shared__ double s_diag[WR], s_y[WR];
    __shared__ int s_piv[WPIV_INTS];
    static_assert(sizeof(double) * (WR * WPS + 8 * WR + 2 * WR) + 4 * WPIV_INTS <= 160 * 1024, "LDS per workgroup");
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform by construction
    for (int sys = blockIdx.x; sys < B; sys += gridDim.x) {
        const double* As = A + (size_t)sys * (size_t)n * (size_t)n;
        for (int e = tid; e < n * n; e += 256) {
            const int i = e / n, j = e - i * n;
            s_S[i * WPS + j] = As[e];
        }
        for (int i = tid; i < n; i += 256) s_S[i * WPS + WR] = -b[(size_t)sys * n + i];
        __syncthreads();
        wide_solve_pivoted<true>((lds_double_t*)s_S, (lds_double_t*)&s_m[0][0], (lds_double_t*)s_diag, (lds_double_t*)s_y, (lds_int_t*)s_piv, w,
                                 lane, n);
        if (tid < n) {
            x[(size_t)sys * n + tid] = s_y[tid] * rcp(s_diag[tid]);
            if (piv) piv[(size_t)sys * n + tid] = s_piv[WPIV_PERM + tid];
        }
        if (tid == 0) info[sys] = s_piv[WPIV_INFO];
        __syncthreads();                                             // the outputs are read: the next system may be parked and solved
    }
}

}  // namespace

extern "C" {

int bg_wide_solve_pivoted(int B, int n, const double* A, const double* b, double* x, int32_t* piv, int32_t* info, void* stream)
{
    if (n < 1 || n > WR) return BG_ERR_UNSUPPORTED_R;
    if (B < 0) return BG_ERR_BAD_ARG;
    if (B == 0) return BG_OK;
    if (!A || !b || !x || !info) return BG_ERR_BAD_ARG;
    hipLaunchKernelGGL(wide_solve_pivoted_kernel, dim3(persistent_grid(B, 1)), dim3(256), 0, (hipStream_t)stream, B, n, A, b, x, piv, info);
    return check_launch();
}

}  // extern "C"
