// rom_hyper_wide.hip -- bg_hyper_rom_run_wide: the HYPER-REDUCED POD-PROM time loop of one sample on one compute unit for the
// thesis' LARGER bases, 40 < r <= 96, on up to 512 sampled mesh rows.  reference: FEMBurgers.pod_prom_burgers,
// FEM/fem_burgers.py:709-785, with the sums over mesh rows restricted to m sampled rows and weighted.
//
// The loop is rom_hyper.hip's hyper_body (included with BG_ROM_HYPER_WIDE_TU defined, as rom_hyper_local.hip includes it: the
// kernels of bg_hyper_rom_run and bg_hyper_local_rom_run stay exactly what they were) with the description HyperWidePod in the
// place of LongLayout: rom_wide_device.hpp's WidePod -- 24 four-column blocks, 98-double LDS rows, the upper block pairs only for
// LSPG, the guarded pivot-free 96 x 96 Gauss-Jordan by all four waves (wide_solve) -- with a solve_add that adds dq to q itself.
// By default there is no repair: a sample whose elimination meets a multiplier above 1 or a zero pivot (or every sample under
// BG_OPT_FORCE_PIVOTED) is marked BG_INFO_NEEDS_PIVOTING and handed back to the caller, as in bg_rom_run_wide.  With
// BG_OPT_PIVOT_ON_DEVICE the repair kernel (PIV) follows the fast one, as in bg_hyper_rom_run, and redoes those samples with
// rom_wide_device.hpp's wide_solve_pivoted; its pivot rows, info and permutation are 448 B of LDS in the guards' place.
// Nothing here touches a vector of mesh length: 3 <= N <= bg_fom_max_n().
//
// The table is PhiS [MPAD][3][98], MPAD = m rounded up to 16: a slab of 16 sampled rows is one contiguous piece of 37 632 B.
// LDS: 32 rows per slab would make 2 x 75 264 B of slab buffers and leave no room for the per-row arrays at m = 512; with 16
// the two buffers are 75 264 B, which is exactly the parked 96 x 98 system.  With the five per-row double arrays and the row
// index at m = 512 (22 528 B), the slab's coefficients (512 B), q (768 B), the multipliers of two panels (6 144 B), the
// diagonal and y (1 536 B) and the guards (16 B): 106 768 B of 163 840 B, one workgroup per compute unit.
#define BG_ROM_HYPER_WIDE_TU
#include "rom_hyper.hip"
#include "rom_wide_device.hpp"

namespace {

constexpr int HWS = 16;                // sampled rows per slab
constexpr int HWMMAX = 512;            // sampled rows held

struct HyperWidePod : WidePod {
    // solve(Ar, -br) (:767) by wide_solve, q = base + dq into L.q, |dq|^2 and |q|^2: WidePod::solve_update with the base given
    // by the caller (this lane's q at rows lane and 64 + lane, 0 at and beyond r, read before the solve's first barrier)
    // where the streaming loops take the parked Phi^T u.  `force`: BG_OPT_FORCE_PIVOTED, every sample is handed back.
    template <bool GAL, int W>
    static __device__ __forceinline__ void solve_add(const StreamLds& L, int r, int lane, double base0, double base1, bool force,
                                                     bool& aborted, double& nd, double& nq)
    {
        wide_solve<GAL>((lds_double_t*)L.slab, (lds_double_t*)L.m, (lds_double_t*)L.diag, (lds_double_t*)L.y, (lds_int_t*)L.bad, W, lane, r);
        const bool tripped = ((L.bad[0] | L.bad[1] | L.bad[2] | L.bad[3]) != 0) || force;      // workgroup-uniform
        if (tripped) aborted = true;
        add_dq<W>(L, r, lane, base0, base1, nd, nq);
    }

    // The repair kernel's (PIV): wide_solve_pivoted, whose L.bad holds WPIV_INTS ints.  Nothing is handed back; an exactly
    // singular system leaves LAPACK's info in info_out and the sample stops.  (A routine of its own and not a parameter of
    // solve_add: with info_out passed through the fast kernels' call, their register allocation changed.)
    template <bool GAL, int W>
    static __device__ __forceinline__ void solve_add_pivoted(const StreamLds& L, int r, int lane, double base0, double base1, int& info_out,
                                                             double& nd, double& nq)
    {
        wide_solve_pivoted<GAL>((lds_double_t*)L.slab, (lds_double_t*)L.m, (lds_double_t*)L.diag, (lds_double_t*)L.y, (lds_int_t*)L.bad, W, lane, r);
        const int singular = L.bad[WPIV_INFO];                                                 // workgroup-uniform
        if (singular != 0 && info_out == 0) info_out = singular;
        add_dq<W>(L, r, lane, base0, base1, nd, nq);
    }

    // x_k = y_k / d_k of either solve, q = base + dq, the two norms
    template <int W>
    static __device__ __forceinline__ void add_dq(const StreamLds& L, int r, int lane, double base0, double base1, double& nd, double& nq)
    {
        const double dq0 = (lane < r) ? L.y[lane] * rcp(L.diag[lane]) : 0.0;
        const double dq1 = (64 + lane < r) ? L.y[64 + lane] * rcp(L.diag[64 + lane]) : 0.0;
        const double q0 = base0 + dq0, q1 = base1 + dq1;
        wave_sum2(dq0 * dq0 + dq1 * dq1, q0 * q0 + q1 * q1, nd, nq);
        if (W == 0) {
            L.q[lane] = q0;
            if (lane < WR - 64) L.q[64 + lane] = q1;
        }
    }
};

template <>
struct HyperDims<HyperWidePod> {
    static constexpr int HS = HWS, per_lane = 2;
};

constexpr int HWSLAB = hyper_slab<HyperWidePod>;

// PIV: the repair kernel behind BG_OPT_PIVOT_ON_DEVICE, which redoes the marked samples (every sample under
// BG_OPT_FORCE_PIVOTED) from u0 with wide_solve_pivoted in every iteration.
template <bool GAL, bool PIV>
__global__ __launch_bounds__(256, 1) void rom_hyper_wide_kernel(HyperRunArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_slab[2 * HWSLAB];            // two slab buffers; later the system
    __shared__ double s_g[HWMMAX], s_fdt[HWMMAX], s_hl[HWMMAX], s_hr[HWMMAX], s_w[HWMMAX];
    __shared__ int s_row[HWMMAX];
    __shared__ __attribute__((aligned(16))) double s_cf[HWS][4];                  // weighted lo, di, up, R per row of the slab
    __shared__ __attribute__((aligned(16))) double s_q[WR];
    __shared__ double s_m[8][WR];                                                 // multipliers of the current and the next panel
    __shared__ double s_diag[WR], s_y[WR];
    __shared__ int s_bad[PIV ? WPIV_INTS : 4];                                    // the guards; PIV: pivot rows, info, permutation
    static_assert(sizeof(double) * (2 * HWSLAB + 5 * HWMMAX + 4 * HWS + WR + 8 * WR + 2 * WR) + 4 * HWMMAX + 4 * WPIV_INTS <= 160 * 1024,
                  "LDS per workgroup");
    static_assert(HWMMAX % HWS == 0 && HWS % 16 == 0 && HWS <= 64, "whole slabs of whole 16-row steps, at most one row per quad");
    static_assert(WR * WPS <= 2 * HWSLAB, "the parked system fits over the slabs");
    static_assert((HWSLAB * 8) % 16 == 0, "a slab is whole 16-byte DMA lanes");
    const StreamLds L{s_slab, nullptr, nullptr, nullptr, nullptr, s_cf, s_q, &s_m[0][0], s_diag, s_y, nullptr, s_bad, nullptr};
    const HyperLds H{s_g, s_fdt, s_hl, s_hr, s_w, s_row, nullptr, nullptr, nullptr};
    switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {       // wave-uniform by construction
        case 0: hyper_body<GAL, PIV, 0, false, HyperRunArgs, HyperWidePod>(a, L, H); break;
        case 1: hyper_body<GAL, PIV, 1, false, HyperRunArgs, HyperWidePod>(a, L, H); break;
        case 2: hyper_body<GAL, PIV, 2, false, HyperRunArgs, HyperWidePod>(a, L, H); break;
        default: hyper_body<GAL, PIV, 3, false, HyperRunArgs, HyperWidePod>(a, L, H); break;
    }
}

}  // namespace

extern "C" {

int bg_hyper_rom_wide_limits(int* max_r, int* max_m)
{
    if (!max_r || !max_m) return BG_ERR_BAD_ARG;
    *max_r = WR;
    *max_m = HWMMAX;
    return BG_OK;
}

// doubles of the packed stencil table bg_hyper_rom_run_wide reads: three rows of 98 per sampled row, m rounded up to 16 (any r <= 96)
long long bg_hyper_rom_wide_table_elems(int m, int r)
{
    if (m < 1 || m > HWMMAX || r < 1 || r > WR) return 0;
    return (long long)((m + HWS - 1) / HWS) * HWSLAB;
}

int bg_hyper_rom_run_wide(int N, int B, int r, int m, int nsteps, int projection, const int32_t* rows, const double* xi, const double* xs,
                          const double* PhiS, const double* q0, const double* u0s, const double* mu1, const double* mu2, double dt,
                          double E, double tol, int max_it, int options, double* qhist, int32_t* iters, int32_t* flags, int32_t* info,
                          const int32_t* order, void* stream)
{
    HyperRunArgs a;
    const int rc = hyper_run_args(a, WR, HWMMAX, N, B, r, m, nsteps, projection, rows, xi, xs, PhiS, q0, u0s, mu1, mu2, dt, E, tol, max_it,
                                  options, qhist, iters, flags, info, order);
    if (rc != BG_OK || B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        if (options & BG_OPT_PIVOT_ON_DEVICE)
            return launch_fast_then_repair(B, 1, a.force_pivoted != 0, [&](auto piv, int grid) {
                hipLaunchKernelGGL((rom_hyper_wide_kernel<decltype(p)::galerkin, decltype(piv)::value>), dim3(grid), dim3(256), 0, st, a);
            });
        hipLaunchKernelGGL((rom_hyper_wide_kernel<decltype(p)::galerkin, false>), dim3(persistent_grid(B, 1)), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
