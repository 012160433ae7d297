// rom_hyper_ann_wide.hip -- the whole HYPER-REDUCED POD-ANN PROM time loop of one sample on one compute unit for up to 20
// primary modes (bg_hyper_ann_rom_run_wide): both projections of pod_ann_prom (reference FEM/fem_burgers.py:1177-1251,
// compute_ann_jacobian :1254-1275) are assembled from m sampled mesh rows with weights xi >= 0,
//   Ar = sum_j xi_j w_j^T y_j,  br = sum_j xi_j w_j^T R_j  with W = U_p + U_s dN(q_p),
// y_j = (A W)[i_j] and w_j = W[i_j] (Galerkin) or y_j (LSPG), so the mesh side of an iteration (tangent, projection, decode)
// costs what the at most 3 m stencil nodes of those rows cost whatever the mesh size; the closure evaluation is the full
// loop's.  The kernel never touches a vector of mesh length.  bg_hyper_ann_rom_run (rom_hyper_ann.hip) stops at n <= 8.
//
// The loop is bg_ann_rom_run_wide's own body (rom_ann_wide_loop_device.hpp; rom_hyper_table_device.hpp describes the
// hyper-reduced form) on the compacted mesh of the stencil nodes: the closure MLP, tangent_fragments, mfma_passes,
// pivoted_solve and decode_u are unchanged.  This file keeps the three instantiations and the entry points, all on four
// waves (ann_layers is written for 256 threads):
//   nodes <= 256   S = 4    two workgroups per CU   UTn row stride 512
//   nodes <= 512   S = 8    two workgroups per CU   UTn row stride 512
//   nodes <= 768   S = 12   one workgroup per CU    UTn row stride 768 (the 512-register budget, 96 KB of LDS)
#include "rom_ann_wide_loop_device.hpp"

namespace {

constexpr int HAW_MAX_ROWS = 256;                // sampled rows
constexpr int HAW_MAX_NODES = 3 * HAW_MAX_ROWS;  // table nodes: every sampling of HAW_MAX_ROWS rows runs
constexpr int HAW_LONG_UT_LD = 768;              // row stride of UTn beyond 512 nodes

constexpr int haw_workgroups_per_cu(int nodes) { return nodes <= AW_UT_LD ? 2 : 1; }
constexpr int haw_ut_ld(int nodes) { return nodes <= AW_UT_LD ? AW_UT_LD : HAW_LONG_UT_LD; }

}  // namespace

extern "C" {

int bg_hyper_ann_rom_wide_limits(int* max_n, int* max_nbar, int* max_width, int* max_layers, int* max_m, int* max_nodes)
{
    if (max_n) *max_n = AW_MAX_N;
    if (max_nbar) *max_nbar = ANN_MAX_NBAR;
    if (max_width) *max_width = ANN_MAX_WIDTH;
    if (max_layers) *max_layers = ANN_MAX_LAYERS;
    if (max_m) *max_m = HAW_MAX_ROWS;
    if (max_nodes) *max_nodes = HAW_MAX_NODES;
    return BG_OK;
}

// persistent workgroups per compute unit of the instantiation that runs a table of `nodes` nodes (0: no such table)
int bg_hyper_ann_rom_wide_workgroups_per_cu(int nodes)
{
    return (nodes < 1 || nodes > HAW_MAX_NODES) ? 0 : haw_workgroups_per_cu(nodes);
}

// row stride of UTn for a table of `nodes` nodes (0: no such table)
int bg_hyper_ann_rom_wide_ut_ld(int nodes)
{
    return (nodes < 1 || nodes > HAW_MAX_NODES) ? 0 : haw_ut_ld(nodes);
}

int bg_hyper_ann_rom_run_wide(int N, int B, int n, int nbar, int m, int nodes, int nsteps, int projection,
                              const int32_t* node, const double* xn, const int32_t* pos, const double* xi, const double* UTn,
                              const double* q0, const double* u0n, const double* mu1, const double* mu2, int n_layers,
                              const int* widths, const float* const* wt, const float* const* bias, const int* acts,
                              const float* alphas, double dt, double E, double tol, int max_it, int options, double* qhist,
                              double* qshist, int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    if (N < 3 || B < 0 || n < 1 || nbar < 1 || m < 1 || nodes < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0) || n_layers < 1)
        return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > bg_fom_max_n()) return BG_ERR_UNSUPPORTED_N;
    if (m > HAW_MAX_ROWS || nodes > HAW_MAX_NODES) return BG_ERR_UNSUPPORTED_R;
    if (m > N || nodes > N || nodes < m || nodes > 3 * m) return BG_ERR_BAD_ARG;
    HyperAnnWideRunArgs a;
    if (const int rc = ann_model_check(AW_MAX_N, n, nbar, n_layers, widths, wt, bias, acts, alphas, a.m)) return rc;
    if (B == 0) return BG_OK;
    if (!node || !xn || !pos || !xi || !UTn || !q0 || !u0n || !mu1 || !mu2 || !qhist || !qshist || !flags || !info ||
        (nsteps > 0 && !iters))
        return BG_ERR_BAD_ARG;
    if ((uintptr_t)UTn & 15) return BG_ERR_BAD_ARG;      // 16-byte loads
    a.x = xn; a.UT = UTn; a.u0 = u0n; a.mu1 = mu1; a.mu2 = mu2; a.hist = qhist; a.iters = iters; a.flags = flags;
    a.info = info; a.order = order; a.dt = dt; a.E = E; a.tol = tol; a.N = N; a.B = B; a.n = n; a.nbar = nbar;
    a.nsteps = nsteps; a.max_it = max_it; a.supg = options & BG_OPT_SUPG; a.nonuniform = 1;
    a.no_reuse = 0;                                      // the tangent is not kept across time steps: nothing to switch off
    a.node = node; a.pos = pos; a.xi = xi; a.q0 = q0; a.qshist = qshist; a.nodes = nodes; a.nrows = m;
    const int grid = persistent_grid(B, haw_workgroups_per_cu(nodes));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        constexpr int PROJ = decltype(p)::value;
        if (nodes <= 256)
            hipLaunchKernelGGL((rom_ann_wide_kernel<4, PROJ, 2, AW_UT_LD, HyperAnnWideRunArgs>), dim3(grid), dim3(256), 0, st, a);
        else if (nodes <= AW_UT_LD)
            hipLaunchKernelGGL((rom_ann_wide_kernel<8, PROJ, 2, AW_UT_LD, HyperAnnWideRunArgs>), dim3(grid), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL((rom_ann_wide_kernel<12, PROJ, 1, HAW_LONG_UT_LD, HyperAnnWideRunArgs>), dim3(grid), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
