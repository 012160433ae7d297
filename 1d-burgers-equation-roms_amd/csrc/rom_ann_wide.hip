// rom_ann_wide.hip -- the POD-ANN PROM time loop of one sample on one compute unit for up to 20 primary modes, and its
// C-ABI entry point (bg_ann_rom_run_wide).
//
// bg_ann_rom_run (rom_ann_fused.hip, K2a) stops at n <= 8: two 4-column MFMA blocks, the N x 8 tangent resident in LDS,
// pivoted_gj8.  The reference's second POD-ANN model has n = 17, nbar = 79 (FEM/fem_burgers.py:1177-1251,
// compute_ann_jacobian :1254-1275).  This kernel runs K2a's iteration on the mesh side of the POD-RBF loop
// (rom_rbf_fused.hip, K9), which already covers n <= 20.  Per Gauss-Newton pass of one 256-thread workgroup, no kernel boundary:
//     closure at the current q_p: the MLP value N(q_p) AND its input-Jacobian in ONE float32 forward-mode pass (the value
//        and the n tangent directions are the 1 + n rows of a small matrix in LDS; a thread owns 4 outputs of a layer and
//        a slice of its inputs, the weights stream from L2 as 16-byte loads of W^T; the slices are folded with DPP and
//        permlane swaps so that all rows of an output meet in one lane, which applies bias, activation and derivative)
//     -> decode u = U_p q_p + U_s N(q_p)  (:1242; not on the first pass of a time step: U0 stays u^n)
//     -> tangent W = U_p + U_s dN (:1224) formed straight in the projection's fragment registers from the nbar x 20 table
//        s_J (no N x n copy in LDS), assembly, projection on v_mfma_f64_4x4x4_4b (mfma_passes), as K9
//     -> n x n solve with np.linalg.solve's pivot choice (pivoted_solve, lu_pivoted_wave<20>)             :1237
//     -> q_p += dq, err = |dq| / (|q_p| + 1e-14), stopping test                                             :1238-1244
// q_p = U_p^T u^n at the start of a time step only (:1197).  The evaluation that follows the last solve of a time step
// feeds the decode alone and is a value-only one (1 row instead of 1 + n); row 0 is computed by the same operations in the
// same order in either kind.  The tangent is not kept across time steps (it is not resident during the projection), so
// BG_OPT_NO_TANGENT_REUSE is accepted and changes nothing.
// The mesh side is rom_closure_device.hpp's, shared with rom_rbf_fused.hip; the closure MLP -- its limits, its arguments
// (AnnModel in AnnRunArgs), the entry point's model check and the layer loop ann_layers -- is rom_ann_device.hpp's, shared
// with rom_ann_fused.hip: here with one 16-byte chunk of outputs per thread and the swap fold only.  The body -- the input
// set-up, the tables s_f and s_J, the LDS overlay and the loop -- is rom_ann_wide_loop_device.hpp's, shared with
// rom_hyper_ann_wide.hip (bg_hyper_ann_rom_run_wide, the same loop on a row sampling's stencil nodes); this file keeps the two
// instantiations (S = 4: N <= 256, S = 8: N <= 512, two workgroups per CU) and the entry point.
#include "rom_ann_wide_loop_device.hpp"

extern "C" {

int bg_ann_rom_run_wide_limits(int* max_n, int* max_nbar, int* max_width, int* max_layers)
{
    if (max_n) *max_n = AW_MAX_N;
    if (max_nbar) *max_nbar = ANN_MAX_NBAR;
    if (max_width) *max_width = ANN_MAX_WIDTH;
    if (max_layers) *max_layers = ANN_MAX_LAYERS;
    return BG_OK;
}

int bg_ann_rom_run_wide(int N, int B, int n, int nbar, int nsteps, int projection, const double* x, const double* UT,
                        const double* u0, const double* mu1, const double* mu2, int n_layers, const int* widths,
                        const float* const* wt, const float* const* bias, const int* acts, const float* alphas,
                        double dt, double E, double tol, int max_it, int options, double* hist, int32_t* iters,
                        int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    if (N < 2 || B < 0 || n < 1 || nbar < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0) || n_layers < 1) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > AW_UT_LD) return BG_ERR_UNSUPPORTED_N;
    AnnRunArgs a;
    if (const int rc = ann_model_check(AW_MAX_N, n, nbar, n_layers, widths, wt, bias, acts, alphas, a.m)) return rc;
    if (B == 0) return BG_OK;
    if (!x || !UT || !u0 || !mu1 || !mu2 || !hist || !flags || !info || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    if ((uintptr_t)UT & 15) return BG_ERR_BAD_ARG;       // 16-byte loads
    a.x = x; a.UT = UT; a.u0 = u0; a.mu1 = mu1; a.mu2 = mu2; a.hist = hist; a.iters = iters; a.flags = flags;
    a.info = info; a.order = order; a.dt = dt; a.E = E; a.tol = tol; a.N = N; a.B = B; a.n = n; a.nbar = nbar;
    a.nsteps = nsteps; a.max_it = max_it; a.supg = options & BG_OPT_SUPG; a.nonuniform = (options & BG_OPT_NONUNIFORM) ? 1 : 0;
    a.no_reuse = 0;                                      // the tangent is not kept across time steps: nothing to switch off
    const int grid = persistent_grid(B, 2);          // two workgroups per CU: one's closure streams while the other projects
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        constexpr int PROJ = decltype(p)::value;
        if (N <= 256) hipLaunchKernelGGL((rom_ann_wide_kernel<4, PROJ>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((rom_ann_wide_kernel<8, PROJ>), dim3(grid), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
