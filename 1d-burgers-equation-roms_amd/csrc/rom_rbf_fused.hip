// rom_rbf_fused.hip -- the whole POD-RBF PROM time loop of one sample on one compute unit, and its C-ABI entry point.
//
// Replaces FEMBurgers.pod_rbf_prom (reference FEM/fem_burgers.py:1278-1398, closure :160-260) for a batch of samples: one
// 256-thread workgroup (512 threads for meshes of 513 .. 1024 nodes, bg_rbf_rom_run_long) owns a sample for ALL time steps
// and Gauss-Newton iterations.  Per iteration, all fp64, with no
// kernel boundary (the arithmetic of the reference and of the host-driven path burgers_hip/rom.py::pod_rbf_run):
//     q_p = U_p^T U0, recomputed from the current iterate every iteration                       :1352
//     -> closure Jacobian at q_p: xs = 2 (q_p - x_min) / dx - 1, per centre the kernel value and the gradient factors
//        G[i][k] = (coef_i 2/dx_k) (xs_k - Xt_ik) as csrc/rbf.hip, staged in LDS 128 centres at a time, then contracted
//        with the output-scaled weights Wd = W dy/2 on the vector ALU: J[j][k] = sum_i Wd[i][j] G[i][k]   :238-260
//     -> tangent W = U_p + U_s J formed straight in the fragment registers of the projection (no N x n copy in LDS)
//     -> assembly with SUPG (b[0] = mu1) and the Galerkin / LSPG projection on v_mfma_f64_4x4x4_4b (mfma_passes, as
//        bg_rom_run / bg_ann_rom_run)                                                                       :1338-1361
//     -> n x n solve with partial pivoting (one wave, pivoted_solve)               np.linalg.solve :1365
//     -> q_new = q_p + dq, err = |dq| / |q_new| (|dq| when |q_new| = 0), stopping test                  :1366-1390
//     -> closure value at q_new: phi_i, f_j = sum_i phi_i Wd[i][j] + (dy/2 + y_min)_j                 :225-236
//     -> decode U1 = U_p q_new + U_s f                                                                  :1378-1381
// The centres and weights stream from L2 in tiles (any Ns), U_p and U_s are re-read from L2 every iteration; HBM sees u0
// once and one N-row history write per time step.
// The closure (scale, centre, the Jacobian and value tiles), the LDS overlay and the loop are rom_rbf_loop_device.hpp's, shared
// with rom_hyper_rbf.hip; the mesh side (q_p, tangent, halo edges, assembly, update of q_p, decode) is
// rom_closure_device.hpp's, shared with rom_ann_wide.hip.  This file keeps the entry points.
#include "rom_rbf_loop_device.hpp"

namespace {

// The two entry points: argument checks in the order the header documents, the operand frame, the launch.
// ``long_mesh``: bg_rbf_rom_run_long, 513 <= N <= 1024; otherwise bg_rbf_rom_run, N <= 512.
int rbf_run(bool long_mesh, int N, int B, int n, int nbar, int Ns, int nsteps, int projection, int kind, const double* x,
            const double* UT, const double* XtT, const double* Wd, const double* bias, const double* x_min,
            const double* dx, double eps, const double* u0, const double* mu1, const double* mu2, double dt, double E,
            double tol, int max_it, int options, double* hist, int32_t* iters, int32_t* flags, int32_t* info,
            const int32_t* order, void* stream)
{
    if ((!long_mesh && N < 3) || B < 0 || n < 1 || nbar < 1 || Ns < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0))
        return BG_ERR_BAD_ARG;
    if (kind != BG_RBF_GAUSSIAN && kind != BG_RBF_IMQ) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (long_mesh ? (N <= RBF_UT_LD || N > RBF_LONG_UT_LD) : N > RBF_UT_LD) return BG_ERR_UNSUPPORTED_N;
    if (n > RBF_MAX_N || nbar > RBF_MAX_NBAR || Ns > RBF_MAX_NS) return BG_ERR_UNSUPPORTED_R;
    if (B == 0) return BG_OK;
    if (!x || !UT || !XtT || !Wd || !bias || !x_min || !dx || !u0 || !mu1 || !mu2 || !hist || !flags || !info ||
        (nsteps > 0 && !iters))
        return BG_ERR_BAD_ARG;
    if (((uintptr_t)UT & 15) || ((uintptr_t)Wd & 15)) return BG_ERR_BAD_ARG;     // 16-byte loads
    RbfRunArgs a;
    a.x = x; a.UT = UT; a.XtT = XtT; a.Wd = Wd; a.bias = bias; a.x_min = x_min; a.dx = dx; a.u0 = u0; a.mu1 = mu1;
    a.mu2 = mu2; a.hist = hist; a.iters = iters; a.flags = flags; a.info = info; a.order = order;
    a.eps2 = eps * eps; a.dt = dt; a.E = E; a.tol = tol;
    a.N = N; a.B = B; a.n = n; a.nbar = nbar; a.Ns = Ns; a.nsteps = nsteps; a.max_it = max_it; a.kind = kind;
    a.supg = options & BG_OPT_SUPG; a.nonuniform = (options & BG_OPT_NONUNIFORM) ? 1 : 0;
    const int grid = persistent_grid(B, long_mesh ? 1 : 2);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        constexpr int PROJ = decltype(p)::value;
        if (long_mesh) hipLaunchKernelGGL((rom_rbf_fused_kernel<8, PROJ, RBF_LONG_UT_LD, 8>), dim3(grid), dim3(512), 0, st, a);
        else if (N <= 256) hipLaunchKernelGGL((rom_rbf_fused_kernel<4, PROJ>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((rom_rbf_fused_kernel<8, PROJ>), dim3(grid), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // namespace

extern "C" {

int bg_rbf_rom_limits(int* max_n, int* max_nbar, int* max_ns)
{
    if (max_n) *max_n = RBF_MAX_N;
    if (max_nbar) *max_nbar = RBF_MAX_NBAR;
    if (max_ns) *max_ns = RBF_MAX_NS;
    return BG_OK;
}

int bg_rbf_rom_run(int N, int B, int n, int nbar, int Ns, int nsteps, int projection, int kind, const double* x,
                   const double* UT, const double* XtT, const double* Wd, const double* bias, const double* x_min,
                   const double* dx, double eps, const double* u0, const double* mu1, const double* mu2, double dt,
                   double E, double tol, int max_it, int options, double* hist, int32_t* iters, int32_t* flags,
                   int32_t* info, const int32_t* order, void* stream)
{
    return rbf_run(false, N, B, n, nbar, Ns, nsteps, projection, kind, x, UT, XtT, Wd, bias, x_min, dx, eps, u0, mu1, mu2,
                   dt, E, tol, max_it, options, hist, iters, flags, info, order, stream);
}

int bg_rbf_rom_run_long_limits(int* max_n, int* max_r, int* max_nbar, int* max_ns)
{
    if (max_n) *max_n = RBF_LONG_UT_LD;
    if (max_r) *max_r = RBF_MAX_N;
    if (max_nbar) *max_nbar = RBF_MAX_NBAR;
    if (max_ns) *max_ns = RBF_MAX_NS;
    return BG_OK;
}

int bg_rbf_rom_run_long(int N, int B, int n, int nbar, int Ns, int nsteps, int projection, int kind, const double* x,
                        const double* UT, const double* XtT, const double* Wd, const double* bias, const double* x_min,
                        const double* dx, double eps, const double* u0, const double* mu1, const double* mu2, double dt,
                        double E, double tol, int max_it, int options, double* hist, int32_t* iters, int32_t* flags,
                        int32_t* info, const int32_t* order, void* stream)
{
    return rbf_run(true, N, B, n, nbar, Ns, nsteps, projection, kind, x, UT, XtT, Wd, bias, x_min, dx, eps, u0, mu1, mu2,
                   dt, E, tol, max_it, options, hist, iters, flags, info, order, stream);
}

}  // extern "C"
