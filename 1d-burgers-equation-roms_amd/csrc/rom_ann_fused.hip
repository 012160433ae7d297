// rom_ann_fused.hip -- the whole POD-ANN PROM time loop of one sample on one compute unit, and its C-ABI entry point.
//
// Replaces FEMBurgers.pod_ann_prom (reference FEM/fem_burgers.py:1177-1251, compute_ann_jacobian :1254-1275) for a batch of
// samples when the closure is a plain MLP (Linear + ELU / ReLU / Tanh stacks, POD-ANN/pod_ann.py:38-56): one 256-thread
// workgroup owns a sample for ALL time steps and Gauss-Newton iterations.  Per iteration, with no kernel boundary:
//     assembly (2 rows per thread)
//     -> projection of the tangent W = U_p + U_s dN on v_mfma_f64_4x4x4_4b (mfma_pass, as bg_rom_run; W lives in LDS)
//     -> n x n solve with partial pivoting (one wave, n <= 8)              np.linalg.solve :1237
//     -> q_p += dq, err = |dq| / (|q_p| + 1e-14), stopping test            :1238-1244
//     -> closure at the new q_p: the MLP value N(q_p) AND its input-Jacobian in ONE forward-mode pass in float32 (the
//        value and the n tangent directions are the 1 + n rows of a small matrix in LDS; a thread owns 8 outputs of a
//        layer and a slice of its inputs, the weights stream from L2 as 16-byte loads of W^T) -- the reference evaluates both in float32 too
//        (:1219, :1241) -- then ONE sweep over U_s^T that forms the decode u = U_p q_p + U_s N(q_p) (:1242) and the next
//        iteration's tangent W = U_p + U_s dN (:1224) together, straight into LDS.
// HBM sees u0 once and one N-row history write per time step; the MLP weights (0.5 MB) and U_s (0.4 MB) are re-read from
// L2 every iteration.  Host-side the batched iteration of burgers_hip/rom.py needs ~40 dependent launches per iteration
// for the same work.  The closure MLP -- its limits, its arguments (AnnModel in AnnRunArgs), the entry point's model check
// and the layer loop ann_layers -- is rom_ann_device.hpp's, shared with rom_ann_wide.hip: here with two 16-byte chunks of
// outputs per thread, the two-stage fold always and the swap fold for 1 and 6 rows.  The input set-up (s_qlast), the sweep
// and its table s_dN, pivoted_gj8, the LDS overlay and the loop are rom_ann_loop_device.hpp's, shared with the hyper-reduced
// loop of rom_hyper_ann.hip; this file keeps the kernel and the entry point.
#include "rom_ann_loop_device.hpp"

namespace {

using namespace bg;
using namespace bg::fused;

// two workgroups per CU: one's memory latency hides behind the other
template <int S, int PROJ>
constexpr auto rom_ann_fused_kernel = ann_loop_kernel<S, PROJ, 2, AnnRunArgs>;

}  // namespace

extern "C" {

int bg_ann_rom_limits(int* max_n, int* max_nbar, int* max_width, int* max_layers)
{
    if (max_n) *max_n = ANN_MAX_N;
    if (max_nbar) *max_nbar = ANN_MAX_NBAR;
    if (max_width) *max_width = ANN_MAX_WIDTH;
    if (max_layers) *max_layers = ANN_MAX_LAYERS;
    return BG_OK;
}

int bg_ann_rom_run(int N, int B, int n, int nbar, int nsteps, int projection, const double* x, const double* UT,
                   const double* u0, const double* mu1, const double* mu2, int n_layers,
                   const int* widths, const float* const* wt, const float* const* bias, const int* acts,
                   const float* alphas, double dt, double E, double tol, int max_it, int options, double* hist,
                   int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    if (N < 2 || B < 0 || n < 1 || nbar < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0) || n_layers < 1) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > 512) return BG_ERR_UNSUPPORTED_N;
    AnnRunArgs a;
    if (const int rc = ann_model_check(ANN_MAX_N, n, nbar, n_layers, widths, wt, bias, acts, alphas, a.m)) return rc;
    if (B == 0) return BG_OK;
    if (!x || !UT || !u0 || !mu1 || !mu2 || !hist || !flags || !info || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    a.x = x; a.UT = UT; a.u0 = u0; a.mu1 = mu1; a.mu2 = mu2; a.hist = hist; a.iters = iters; a.flags = flags;
    a.info = info; a.order = order; a.dt = dt; a.E = E; a.tol = tol; a.N = N; a.B = B; a.n = n; a.nbar = nbar;
    a.nsteps = nsteps; a.max_it = max_it; a.supg = options & BG_OPT_SUPG; a.nonuniform = (options & BG_OPT_NONUNIFORM) ? 1 : 0;
    a.no_reuse = (options & BG_OPT_NO_TANGENT_REUSE) ? 1 : 0;
    const int grid = persistent_grid(B, 2);          // two workgroups per CU: one's memory latency hides behind the other
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        constexpr int PROJ = decltype(p)::value;
        if (N <= 256) hipLaunchKernelGGL((rom_ann_fused_kernel<4, PROJ>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((rom_ann_fused_kernel<8, PROJ>), dim3(grid), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
