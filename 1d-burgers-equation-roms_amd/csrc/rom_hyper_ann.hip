// rom_hyper_ann.hip -- the whole HYPER-REDUCED POD-ANN PROM time loop of one sample on one compute unit
// (bg_hyper_ann_rom_run): both projections of pod_ann_prom (reference FEM/fem_burgers.py:1177-1251) are assembled from m
// sampled mesh rows with weights xi >= 0,  Ar = sum_j xi_j w_j^T y_j,  br = sum_j xi_j w_j^T R_j  with W = U_p + U_s dN(q_p),
// y_j = (A W)[i_j] and w_j = W[i_j] (Galerkin) or y_j (LSPG), so an iteration costs what the at most 3 m stencil nodes of
// those rows cost whatever the mesh size, and the kernel never touches a vector of mesh length.
//
// The loop is bg_ann_rom_run's own body (rom_ann_loop_device.hpp; rom_hyper_table_device.hpp describes the hyper-reduced
// form) on the compacted mesh of the stencil nodes: the closure MLP, the sweep over [U_p | U_s] restricted to the table,
// mfma_pass and pivoted_gj8 are unchanged.  This file keeps the three instantiations and the entry points:
//   nodes <= 256   S = 4   two workgroups per CU
//   nodes <= 512   S = 8   two workgroups per CU
//   nodes <= 768   S = 12  one workgroup per CU (the tangent rows alone are 49 KB of LDS)
#include "rom_ann_loop_device.hpp"

namespace {

constexpr int HA_MAX_ROWS = 256;               // sampled rows
constexpr int HA_MAX_NODES = 3 * HA_MAX_ROWS;  // table nodes: every sampling of HA_MAX_ROWS rows runs

constexpr int ha_workgroups_per_cu(int nodes) { return nodes <= 512 ? 2 : 1; }

}  // namespace

extern "C" {

int bg_hyper_ann_rom_limits(int* max_n, int* max_nbar, int* max_width, int* max_layers, int* max_m, int* max_nodes)
{
    if (max_n) *max_n = ANN_MAX_N;
    if (max_nbar) *max_nbar = ANN_MAX_NBAR;
    if (max_width) *max_width = ANN_MAX_WIDTH;
    if (max_layers) *max_layers = ANN_MAX_LAYERS;
    if (max_m) *max_m = HA_MAX_ROWS;
    if (max_nodes) *max_nodes = HA_MAX_NODES;
    return BG_OK;
}

// persistent workgroups per compute unit of the instantiation that runs a table of `nodes` nodes (0: no such table)
int bg_hyper_ann_rom_workgroups_per_cu(int nodes)
{
    return (nodes < 1 || nodes > HA_MAX_NODES) ? 0 : ha_workgroups_per_cu(nodes);
}

int bg_hyper_ann_rom_run(int N, int B, int n, int nbar, int m, int nodes, int nsteps, int projection, const int32_t* node,
                         const double* xn, const int32_t* pos, const double* xi, const double* UTn, const double* q0,
                         const double* u0n, const double* mu1, const double* mu2, int n_layers, const int* widths,
                         const float* const* wt, const float* const* bias, const int* acts, const float* alphas, double dt,
                         double E, double tol, int max_it, int options, double* qhist, double* qshist, int32_t* iters,
                         int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    if (N < 3 || B < 0 || n < 1 || nbar < 1 || m < 1 || nodes < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0) || n_layers < 1)
        return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > bg_fom_max_n()) return BG_ERR_UNSUPPORTED_N;
    if (m > HA_MAX_ROWS || nodes > HA_MAX_NODES) return BG_ERR_UNSUPPORTED_R;
    if (m > N || nodes > N || nodes < m || nodes > 3 * m) return BG_ERR_BAD_ARG;
    HyperAnnRunArgs a;
    if (const int rc = ann_model_check(ANN_MAX_N, n, nbar, n_layers, widths, wt, bias, acts, alphas, a.m)) return rc;
    if (B == 0) return BG_OK;
    if (!node || !xn || !pos || !xi || !UTn || !q0 || !u0n || !mu1 || !mu2 || !qhist || !qshist || !flags || !info ||
        (nsteps > 0 && !iters))
        return BG_ERR_BAD_ARG;
    if ((uintptr_t)UTn & 15) return BG_ERR_BAD_ARG;
    a.x = xn; a.UT = UTn; a.u0 = u0n; a.mu1 = mu1; a.mu2 = mu2; a.hist = qhist; a.iters = iters; a.flags = flags;
    a.info = info; a.order = order; a.dt = dt; a.E = E; a.tol = tol; a.N = N; a.B = B; a.n = n; a.nbar = nbar;
    a.nsteps = nsteps; a.max_it = max_it; a.supg = options & BG_OPT_SUPG; a.nonuniform = 1;
    a.no_reuse = (options & BG_OPT_NO_TANGENT_REUSE) ? 1 : 0;
    a.node = node; a.pos = pos; a.xi = xi; a.q0 = q0; a.qshist = qshist; a.nodes = nodes; a.nrows = m;
    const int grid = persistent_grid(B, ha_workgroups_per_cu(nodes));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        constexpr int PROJ = decltype(p)::value;
        if (nodes <= 256) hipLaunchKernelGGL((ann_loop_kernel<4, PROJ, 2, HyperAnnRunArgs>), dim3(grid), dim3(256), 0, st, a);
        else if (nodes <= 512) hipLaunchKernelGGL((ann_loop_kernel<8, PROJ, 2, HyperAnnRunArgs>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((ann_loop_kernel<12, PROJ, 1, HyperAnnRunArgs>), dim3(grid), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
