// rom_hyper_local.hip -- bg_hyper_local_rom_run: the HYPER-REDUCED local POD-PROM time loop of one sample on one compute
// unit.  reference: FEMBurgers.local_prom_burgers, FEM/fem_burgers.py:979-1079, with the sums over mesh rows restricted to m
// sampled rows and weighted, one sampling for all clusters.
//
// The LOCAL instantiations of rom_hyper.hip's hyper_body, which holds the loop and says what LOCAL adds (HyperLocalRunArgs:
// the pick from reduced coordinates, the lift-only sweep over the old table and q <- Phi_c^T Phi_p q at a switch).  They are
// compiled in a translation unit of their own so that the four kernels of bg_hyper_rom_run stay exactly what they were, as
// rom_local_fused.hip does for bg_local_rom_run.
// Nothing here touches a vector of mesh length: 3 <= N <= bg_fom_max_n(), widths <= 40, m <= 256, mg <= 64, C <= 64.
// LDS: rom_hyper.hip's 77 136 B + u^n at two stencil nodes per sampled row after a switch (4096 B; the third lies in g until
// the first iteration turns it into g) + 64 doubles for q_g = 81 744 B: two workgroups per compute unit (81 920 B each).
#define BG_ROM_HYPER_LOCAL_TU
#include "rom_hyper.hip"

namespace {

constexpr int HLMAXM = 64;             // global modes of the cluster pick: the length of q_g in LDS, four lanes each
constexpr int HLMAXC = 64;             // centres: one lane each in the nearest-centre pick

// The repair kernel (PIV) keeps one workgroup per CU: its one-wave pivoted solve holds a 41-double row per lane.
template <bool GAL, bool PIV>
__global__ __launch_bounds__(256, PIV ? 1 : HWG_PER_CU) void rom_hyper_local_kernel(HyperLocalRunArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_slab[2 * HSLAB];             // two slab buffers; later the system
    __shared__ double s_g[HMMAX], s_fdt[HMMAX], s_hl[HMMAX], s_hr[HMMAX], s_w[HMMAX];
    __shared__ double s_u0[HMMAX], s_ur[HMMAX];                                   // u^n at nodes i, i + 1 after a switch
    __shared__ double s_qg[HLMAXM];
    __shared__ int s_row[HMMAX];
    __shared__ __attribute__((aligned(16))) double s_cf[HS][4];                   // weighted lo, di, up, R per row of the slab
    __shared__ __attribute__((aligned(16))) double s_q[LR];
    __shared__ int s_bad[8];                                                      // [4] guard of each wave, [4] info of the pivoted solve
    static_assert(sizeof(double) * (2 * HSLAB + 7 * HMMAX + HLMAXM + 4 * HS + LR) + 4 * HMMAX + 32 <= 160 * 1024 / HWG_PER_CU, "LDS per workgroup");
    static_assert(HLMAXM * 4 <= 256 && LR * 4 <= 256 && HLMAXC <= 64, "four lanes per global mode and per row of trans, one lane per centre");
    // over the dead slabs: the system [LR][LSW], then the multipliers of two panels, the diagonal, y and x
    double* const s_m = s_slab + LR * LSW;
    double* const s_diag = s_m + 512;
    static_assert(LR * LSW + 512 + 3 * 64 <= 2 * HSLAB, "the solve's arrays fit over the slabs");
    const StreamLds L{s_slab, nullptr, nullptr, nullptr, nullptr, s_cf, s_q, s_m, s_diag, s_diag + 64, s_diag + 128, s_bad, nullptr};
    const HyperLds H{s_g, s_fdt, s_hl, s_hr, s_w, s_row, s_u0, s_ur, s_qg};
    switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {       // wave-uniform by construction
        case 0: hyper_body<GAL, PIV, 0, true>(a, L, H); break;
        case 1: hyper_body<GAL, PIV, 1, true>(a, L, H); break;
        case 2: hyper_body<GAL, PIV, 2, true>(a, L, H); break;
        default: hyper_body<GAL, PIV, 3, true>(a, L, H); break;
    }
}

}  // namespace

extern "C" {

int bg_hyper_local_rom_limits(int* max_r, int* max_m, int* max_mg, int* max_clusters)
{
    if (max_r) *max_r = LR;
    if (max_m) *max_m = HMMAX;
    if (max_mg) *max_mg = HLMAXM;
    if (max_clusters) *max_clusters = HLMAXC;
    return BG_OK;
}

// doubles of the stack of stencil tables bg_hyper_local_rom_run reads: per cluster three rows of 42 per sampled row, m rounded up to 32
long long bg_hyper_local_rom_table_elems(int C, int m)
{
    if (C < 1 || C > HLMAXC || m < 1 || m > HMMAX) return 0;
    return (long long)C * ((m + HS - 1) / HS) * HSLAB;
}

int bg_hyper_local_rom_run(int N, int B, int C, int rmax, int mg, int m, int nsteps, int projection, const int32_t* rows,
                           const double* xi, const double* xs, const double* PhiS, const int32_t* widths, const double* trans,
                           const double* pick, const double* centres, const double* qg0, const double* pu0, const double* u0s,
                           const double* mu1, const double* mu2, double dt, double E, double tol, int max_it, int options,
                           double* qhist, int32_t* iters, int32_t* flags, int32_t* info, int32_t* clusters, const int32_t* order,
                           void* stream)
{
    if (N < 3 || B < 0 || C < 1 || rmax < 1 || mg < 1 || m < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > bg_fom_max_n()) return BG_ERR_UNSUPPORTED_N;
    if (rmax > LR || m > HMMAX || mg > HLMAXM || C > HLMAXC) return BG_ERR_UNSUPPORTED_R;
    if (m > N) return BG_ERR_BAD_ARG;
    if (B == 0) return BG_OK;
    if (!rows || !xi || !xs || !PhiS || !widths || !trans || !pick || !centres || !qg0 || !pu0 || !u0s || !mu1 || !mu2 || !qhist ||
        !flags || !info || (nsteps > 0 && !iters))
        return BG_ERR_BAD_ARG;
    if ((uintptr_t)PhiS & 15) return BG_ERR_BAD_ARG;
    HyperLocalRunArgs a;
    a.rows = rows; a.xi = xi; a.xs = xs; a.PhiS = PhiS; a.q0 = pu0; a.u0s = u0s; a.mu1 = mu1; a.mu2 = mu2; a.qhist = qhist;
    a.iters = iters; a.flags = flags; a.info = info; a.order = order;
    a.dt = dt; a.E = E; a.tol = tol; a.N = N; a.B = B; a.r = rmax; a.m = m; a.nsteps = nsteps; a.max_it = max_it;
    a.supg = options & BG_OPT_SUPG; a.nonuniform = (options & BG_OPT_NONUNIFORM) ? 1 : 0;
    a.force_pivoted = (options & BG_OPT_FORCE_PIVOTED) ? 1 : 0;
    a.widths = widths; a.trans = trans; a.pick = pick; a.centres = centres; a.qg0 = qg0; a.clusters = clusters;
    a.table = (long long)((m + HS - 1) / HS) * HSLAB; a.C = C; a.mg = mg;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        return launch_fast_then_repair(B, HWG_PER_CU, a.force_pivoted != 0, [&](auto piv, int grid) {
            hipLaunchKernelGGL((rom_hyper_local_kernel<decltype(p)::galerkin, decltype(piv)::value>), dim3(grid), dim3(256), 0, st, a);
        });
    });
}

}  // extern "C"
