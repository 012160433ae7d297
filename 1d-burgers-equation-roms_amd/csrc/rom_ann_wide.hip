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
// with rom_ann_fused.hip: here with one 16-byte chunk of outputs per thread and the swap fold only.  This file keeps the
// input set-up, the tables s_f and s_J, the LDS overlay and the loop.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "rom_ann_device.hpp"
#include "rom_closure_device.hpp"

namespace {

using namespace bg;
using namespace bg::fused;

constexpr int AW_NB = 5;                       // column blocks of the projection: n <= 20
constexpr int AW_MAX_N = 4 * AW_NB;
constexpr int AW_MAX_ROWS = 1 + AW_MAX_N;      // value + tangent directions
constexpr int AW_UT_LD = 512;                  // row stride of UT: the largest N

template <int S, int PROJ>
__global__ __launch_bounds__(256, 2) void rom_ann_wide_kernel(AnnRunArgs a)
{
    constexpr int NB = AW_NB;
    constexpr int NPAD = 64 * S;
    constexpr int NIT = NPAD / 256;              // rows per thread of the strided loops
    constexpr int RW = 4 * NB;
    constexpr bool GAL = PROJ == BG_PROJ_GALERKIN;
    constexpr int kAccBudget = GAL ? 24 : 14;    // accumulators per projection pass (see rom_rbf_fused.hip)
    __shared__ double s_u[NPAD + 4];             // u at offset 2, zero halo on each side
    __shared__ double s_g[NPAD], s_h[NPAD];
    __shared__ double s_fdt[NPAD];               // dt F
    __shared__ double s_q[RW], s_x[RW];
    __shared__ double s_part[4][RW];             // per-wave partial sums of U_p^T u
    __shared__ double s_f[ANN_MAX_NBAR];         // N(q_p) of the latest evaluation
    __shared__ int s_info;
    // The two halves of a pass never overlap in time and share one block of LDS (two workgroups per CU need <= 80 KB each):
    //   closure: s_act (two buffers of 21 rows x 256 floats); the finished table s_J takes the buffer the last layer read
    //   tangent -> assembly + projection + solve: s_J until the fragments are formed, then s_coef, s_elo, s_ehi, s_red
    constexpr int kActHalfB = AW_MAX_ROWS * ANN_MAX_WIDTH * 4, kActB = 2 * kActHalfB;
    constexpr int kJB = ANN_MAX_NBAR * RW * 8;
    static_assert(kJB <= kActHalfB && kActHalfB % 16 == 0, "s_J fits the idle activation buffer");
    constexpr int kCoefB = NPAD * 4 * 8, kEdgeB = 64 * RW * 8, kRedB = 4 * RW * (RW + 4) * 8;
    constexpr int kPhaseP = kCoefB + 2 * kEdgeB + kRedB;
    __shared__ __attribute__((aligned(16))) unsigned char s_shared[kActB > kPhaseP ? kActB : kPhaseP];
    auto& s_act = *reinterpret_cast<float (*)[2][AW_MAX_ROWS][ANN_MAX_WIDTH]>(s_shared);
    auto& s_coef = *reinterpret_cast<double (*)[NPAD][4]>(s_shared);
    auto& s_elo = *reinterpret_cast<double (*)[64][RW]>(s_shared + kCoefB);
    auto& s_ehi = *reinterpret_cast<double (*)[64][RW]>(s_shared + kCoefB + kEdgeB);
    auto& s_red = *reinterpret_cast<double (*)[4][RW][RW + 4]>(s_shared + kCoefB + 2 * kEdgeB);

    // The thread-index family is re-derived from an opaque copy at the top of every pass and of its register-heavy phases:
    // per-lane addresses are loop invariants of the whole kernel, and hoisted out of the loops they end up in scratch.
    int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform by construction
    int t = lane & 3, owner = 16 * w + (lane >> 2);
    int rowbase = owner * S;
    auto rederive = [&]() {
        int v = threadIdx.x;
        asm volatile("" : "+v"(v));
        tid = v; lane = v & 63; t = lane & 3; owner = 16 * w + (lane >> 2); rowbase = owner * S;
    };
    const int N = a.N, n = a.n, nbar = a.nbar, nr = 1 + a.n;
    const double h = (a.x[N - 1] - a.x[0]) / (double)(N - 1);
    const double* __restrict__ UT = a.UT;

    if (tid < 4) s_u[tid < 2 ? tid : NPAD + tid] = 0.0;

    // ---- N(q_p) and dN/dq_p at q_p = s_q, float32 forward mode: rows 0 = value, 1 .. n = tangent directions (ann_layers).
    // NRT = rows compiled in.  Returns the buffer of the outputs.
    auto mlp_impl = [&](auto nrt_c) __attribute__((always_inline)) -> int {
        constexpr int NRT = decltype(nrt_c)::value;
        if (tid < RW) {                                              // inputs padded with zeros to a multiple of 4
            s_act[0][0][tid] = tid < n ? (float)s_q[tid] : 0.0f;
#pragma unroll
            for (int r = 1; r < NRT; ++r) s_act[0][r][tid] = (r - 1 == tid && tid < n) ? 1.0f : 0.0f;
        }
        __syncthreads();
        PhaseClock<false, 1> clk;
        return ann_layers<NRT, 1, true, false>(a.m, s_act, tid, lane, w, clk);
    };

    __builtin_amdgcn_s_setprio(3);
    for (int slot = blockIdx.x; slot < a.B; slot += gridDim.x) {
        const int smp = a.order ? a.order[slot] : slot;
        if (smp < 0 || smp >= a.B) continue;                 // untrusted order entry: the same for the whole workgroup
        const double mu1 = a.mu1[smp], mu2 = a.mu2[smp];
        double* hist = a.hist + (size_t)smp * (size_t)(a.nsteps + 1) * (size_t)N;
        __syncthreads();
        // ---- per-sample constants (compute_forcing_vector :427-461, f_gp of :556-558) and the initial state ----------
#pragma unroll 1
        for (int ii = 0; ii < NIT; ++ii)
            sample_setup_row(tid + 256 * ii, a.x, a.u0, smp, hist, N, mu2, h, a.nonuniform, a.dt, s_u, s_fdt, s_h);
        __syncthreads();

        int flags = 0, info_out = 0;
        for (int step = 0; step < a.nsteps && info_out == 0; ++step) {
            // ---- g = M u^n + dt F (:1214) and q_p = U_p^T u^n (:1197) --------------------------------------------------
            project_q<NIT, 256, 4, AW_UT_LD, RW>(UT, s_u, n, tid, lane, w, s_part, s_q, [&](int i, double uc) {
                double g = 0.0;
                if (i < N) g = rom_mass_rhs_node(a.x, i, N, s_u[i + 1], uc, s_u[i + 3], s_fdt[i], h, a.nonuniform);
                s_g[i] = g;
            });
            int k = 0;
            bool more = true, decode = false;
            while (true) {
                rederive();
                // ---- closure at the current q_p (one call site per row count).  First pass of a time step: dN at the
                // first guess (:1219), U0 stays u^n.  Later passes: q_s = N(q_p) for the decode (:1241-1242) and dN for the
                // next projection (:1219-1224); after the last solve of the step the value alone.
                __builtin_amdgcn_s_setprio(0);
                int cur;
                if (!more) cur = mlp_impl(std::integral_constant<int, 1>{});
                else if (nr <= 10) cur = mlp_impl(std::integral_constant<int, 10>{});
                else if (nr <= 18) cur = mlp_impl(std::integral_constant<int, 18>{});
                else cur = mlp_impl(std::integral_constant<int, AW_MAX_ROWS>{});
                __builtin_amdgcn_s_setprio(3);
                const int nrt = !more ? 1 : (nr <= 10 ? 10 : (nr <= 18 ? 18 : AW_MAX_ROWS));
                // the closure table of this pass: s_f[j] = N_j, s_J[j][c] = dN_j / dq_c (zero from c = n)
                double (*__restrict__ s_J)[RW] = reinterpret_cast<double (*)[RW]>(s_shared + (cur ^ 1) * kActHalfB);
                if (tid < ANN_MAX_NBAR) s_f[tid] = tid < nbar ? (double)s_act[cur][0][tid] : 0.0;
                if (more) {
                    for (int e = tid; e < nbar * RW; e += 256) {
                        const int j = e / RW, c = e - j * RW;
                        s_J[j][c] = (c < n && 1 + c < nrt) ? (double)s_act[cur][1 + c][j] : 0.0;
                    }
                }
                __syncthreads();
                // ---- decode U1 = U_p q_p + U_s N(q_p) (:1242) ------------------------------------------------------------
                if (decode) decode_u<NIT, 256, AW_UT_LD>(s_u, UT, s_q, s_f, N, n, nbar, tid);
                if (!more) break;
                decode = true;
                // ---- tangent W = U_p + U_s dN (:1224) in this lane's projection fragments -----------------------------------
                rederive();
                double frag[NB][S];
                tangent_fragments<S, NB, AW_UT_LD>(frag, UT, s_J, n, nbar, rowbase, t);
                __syncthreads();                         // s_J consumed: the projection phase reuses its LDS
                publish_edges<S, NB>(frag, s_elo, s_ehi, owner, t);
                // ---- assembly: A(u_k), R(u_k) per row into LDS -------------------------------------------------------
                assemble_rows<NPAD, 256>(s_coef, s_u, s_g, s_h, a.x, N, h, a.dt, a.E, a.supg, a.nonuniform, mu1, tid);
                __syncthreads();
                // ---- projection (:1224-1233) -------------------------------------------------------------------------
                {
                    double (*s_wtu)[RW] = s_part;        // the Phi^T u extras of the LSPG pass: not used here
                    mfma_passes<S, NB, GAL, RW, 4, kAccBudget>(frag, HaloEdges<NB>{s_elo, s_ehi, owner, t}, s_coef, s_u,
                                                              rowbase, t, w, lane, s_red, s_wtu);
                }
                __syncthreads();
                // ---- reduced solve with partial pivoting (np.linalg.solve :1237) --------------------------------------
                if (w == 0) pivoted_solve<NB, GAL, 4>(s_red, s_x, &s_info, lane, n);
                __syncthreads();
                if (s_info != 0 && info_out == 0) info_out = s_info;
                // ---- q_p += dq, err = |dq| / (|q_p| + 1e-14)  (:1238-1244) ---------------------------------------------
                const double err = update_q<RW>(s_q, s_x, n, lane, w, [](double nd, double nq) { return nd / (nq + 1e-14); });
                ++k;
                more = (err > a.tol) && (k < a.max_it) && info_out == 0;
                if (!(err - err == 0.0)) flags |= BG_FLAG_NONFINITE;
                if (k >= a.max_it) flags |= BG_FLAG_HIT_CAP;
            }
            write_hist_row<256>(hist + (size_t)(step + 1) * N, s_u, N, tid);
            if (tid == 0) a.iters[(size_t)smp * a.nsteps + step] = k;
        }
        if (tid == 0) {
            a.flags[smp] = flags;
            a.info[smp] = info_out;
        }
    }
}

}  // namespace

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
