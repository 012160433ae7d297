// rom_hyper_rbf.hip -- the whole HYPER-REDUCED POD-RBF PROM time loop of one sample on one compute unit
// (bg_hyper_rbf_rom_run): both projections of pod_rbf_prom (reference FEM/fem_burgers.py:1278-1398) are assembled from m
// sampled mesh rows with weights xi >= 0,  Ar = sum_j xi_j w_j^T y_j,  br = sum_j xi_j w_j^T R_j  with W = U_p + U_s J(q_p),
// y_j = (A W)[i_j] and w_j = W[i_j] (Galerkin) or y_j (LSPG), so the mesh side of an iteration (tangent, projection, decode)
// costs what the at most 3 m stencil nodes of those rows cost whatever the mesh size; the closure evaluation (Ns nbar n) is
// the full loop's.  The kernel never touches a vector of mesh length.
//
// The loop is bg_rbf_rom_run's own body (rom_rbf_loop_device.hpp; rom_hyper_table_device.hpp describes the hyper-reduced
// form) on the compacted mesh of the stencil nodes: the in-kernel fp64 closure, tangent_fragments, mfma_passes,
// pivoted_solve and decode_u are unchanged.  This file keeps the three instantiations and the entry points:
//   nodes <= 256   S = 4   four waves    two workgroups per CU   UTn row stride 512
//   nodes <= 512   S = 8   four waves    two workgroups per CU   UTn row stride 512
//   nodes <= 768   S = 8   eight waves   one workgroup per CU    UTn row stride 1024 (the profile of bg_rbf_rom_run_long)
#include "rom_rbf_loop_device.hpp"

namespace {

constexpr int HR_MAX_ROWS = 256;               // sampled rows
constexpr int HR_MAX_NODES = 3 * HR_MAX_ROWS;  // table nodes: every sampling of HR_MAX_ROWS rows runs

constexpr int hr_workgroups_per_cu(int nodes) { return nodes <= RBF_UT_LD ? 2 : 1; }
constexpr int hr_ut_ld(int nodes) { return nodes <= RBF_UT_LD ? RBF_UT_LD : RBF_LONG_UT_LD; }

}  // namespace

extern "C" {

int bg_hyper_rbf_rom_limits(int* max_n, int* max_nbar, int* max_ns, int* max_m, int* max_nodes)
{
    if (max_n) *max_n = RBF_MAX_N;
    if (max_nbar) *max_nbar = RBF_MAX_NBAR;
    if (max_ns) *max_ns = RBF_MAX_NS;
    if (max_m) *max_m = HR_MAX_ROWS;
    if (max_nodes) *max_nodes = HR_MAX_NODES;
    return BG_OK;
}

// persistent workgroups per compute unit of the instantiation that runs a table of `nodes` nodes (0: no such table)
int bg_hyper_rbf_rom_workgroups_per_cu(int nodes)
{
    return (nodes < 1 || nodes > HR_MAX_NODES) ? 0 : hr_workgroups_per_cu(nodes);
}

// row stride of UTn for a table of `nodes` nodes (0: no such table)
int bg_hyper_rbf_rom_ut_ld(int nodes)
{
    return (nodes < 1 || nodes > HR_MAX_NODES) ? 0 : hr_ut_ld(nodes);
}

int bg_hyper_rbf_rom_run(int N, int B, int n, int nbar, int Ns, int m, int nodes, int nsteps, int projection, int kind,
                         const int32_t* node, const double* xn, const int32_t* pos, const double* xi, const double* UTn,
                         const double* XtT, const double* Wd, const double* bias, const double* x_min, const double* dx,
                         double eps, const double* q0, const double* u0n, const double* mu1, const double* mu2, double dt,
                         double E, double tol, int max_it, int options, double* qhist, double* qshist, int32_t* iters,
                         int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    if (N < 3 || B < 0 || n < 1 || nbar < 1 || Ns < 1 || m < 1 || nodes < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0))
        return BG_ERR_BAD_ARG;
    if (kind != BG_RBF_GAUSSIAN && kind != BG_RBF_IMQ) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > bg_fom_max_n()) return BG_ERR_UNSUPPORTED_N;
    if (n > RBF_MAX_N || nbar > RBF_MAX_NBAR || Ns > RBF_MAX_NS || m > HR_MAX_ROWS || nodes > HR_MAX_NODES)
        return BG_ERR_UNSUPPORTED_R;
    if (m > N || nodes > N || nodes < m || nodes > 3 * m) return BG_ERR_BAD_ARG;
    if (B == 0) return BG_OK;
    if (!node || !xn || !pos || !xi || !UTn || !XtT || !Wd || !bias || !x_min || !dx || !q0 || !u0n || !mu1 || !mu2 ||
        !qhist || !qshist || !flags || !info || (nsteps > 0 && !iters))
        return BG_ERR_BAD_ARG;
    if (((uintptr_t)UTn & 15) || ((uintptr_t)Wd & 15)) return BG_ERR_BAD_ARG;    // 16-byte loads
    HyperRbfRunArgs a;
    a.x = xn; a.UT = UTn; a.XtT = XtT; a.Wd = Wd; a.bias = bias; a.x_min = x_min; a.dx = dx; a.u0 = u0n; a.mu1 = mu1;
    a.mu2 = mu2; a.hist = qhist; a.iters = iters; a.flags = flags; a.info = info; a.order = order;
    a.eps2 = eps * eps; a.dt = dt; a.E = E; a.tol = tol;
    a.N = N; a.B = B; a.n = n; a.nbar = nbar; a.Ns = Ns; a.nsteps = nsteps; a.max_it = max_it; a.kind = kind;
    a.supg = options & BG_OPT_SUPG; a.nonuniform = 1;
    a.node = node; a.pos = pos; a.xi = xi; a.q0 = q0; a.qshist = qshist; a.nodes = nodes; a.nrows = m;
    const int grid = persistent_grid(B, hr_workgroups_per_cu(nodes));
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        constexpr int PROJ = decltype(p)::value;
        if (nodes <= 256)
            hipLaunchKernelGGL((rom_rbf_fused_kernel<4, PROJ, RBF_UT_LD, 4, HyperRbfRunArgs>), dim3(grid), dim3(256), 0, st, a);
        else if (nodes <= RBF_UT_LD)
            hipLaunchKernelGGL((rom_rbf_fused_kernel<8, PROJ, RBF_UT_LD, 4, HyperRbfRunArgs>), dim3(grid), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL((rom_rbf_fused_kernel<8, PROJ, RBF_LONG_UT_LD, 8, HyperRbfRunArgs>), dim3(grid), dim3(512), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
