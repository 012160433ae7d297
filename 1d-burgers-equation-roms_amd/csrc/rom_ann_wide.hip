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
// The mesh side is rom_closure_device.hpp's, shared with rom_rbf_fused.hip; the float32 fold helpers and the activation
// arithmetic are wave_ops.hpp's, shared with rom_ann_fused.hip.  This file keeps the closure, the LDS overlay and the loop.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "rom_closure_device.hpp"

namespace {

using namespace bg;
using namespace bg::fused;

constexpr int AW_NB = 5;                       // column blocks of the projection: n <= 20
constexpr int AW_MAX_N = 4 * AW_NB;
constexpr int AW_MAX_NBAR = 128;
constexpr int AW_MAX_LAYERS = 8;
constexpr int AW_MAX_WIDTH = 256;
constexpr int AW_MAX_ROWS = 1 + AW_MAX_N;      // value + tangent directions
constexpr int AW_UT_LD = 512;                  // row stride of UT: the largest N

struct AnnWideArgs {
    const double* x;        // [N]
    const double* UT;       // [n + nbar][512]: rows 0 .. n-1 = U_p^T, rows n .. n+nbar-1 = U_s^T, zero columns from N
    const double* u0;       // [B][N]
    const double* mu1;      // [B]
    const double* mu2;      // [B]
    double* hist;           // [B][nsteps+1][N]
    int32_t* iters;         // [B][nsteps]
    int32_t* flags;         // [B]
    int32_t* info;          // [B]
    const int32_t* order;   // [B] or null: slot i of the persistent loop works on sample order[i]
    const float* wt[AW_MAX_LAYERS];     // layer l: W^T, [in4][ld] row-major: width[l] rounded up to 4 rows, width[l+1] to 8 columns, zero fill
    const float* bias[AW_MAX_LAYERS];   // [width[l+1]] or null
    int width[AW_MAX_LAYERS + 1];
    int act[AW_MAX_LAYERS];
    float alpha[AW_MAX_LAYERS];
    int nl;
    double dt, E, tol;
    int N, B, n, nbar, nsteps, max_it, supg, nonuniform;
};

template <int S, int PROJ>
__global__ __launch_bounds__(256, 2) void rom_ann_wide_kernel(AnnWideArgs a)
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
    __shared__ double s_f[AW_MAX_NBAR];          // N(q_p) of the latest evaluation
    __shared__ int s_info;
    // The two halves of a pass never overlap in time and share one block of LDS (two workgroups per CU need <= 80 KB each):
    //   closure: s_act (two buffers of 21 rows x 256 floats); the finished table s_J takes the buffer the last layer read
    //   tangent -> assembly + projection + solve: s_J until the fragments are formed, then s_coef, s_elo, s_ehi, s_red
    constexpr int kActHalfB = AW_MAX_ROWS * AW_MAX_WIDTH * 4, kActB = 2 * kActHalfB;
    constexpr int kJB = AW_MAX_NBAR * RW * 8;
    static_assert(kJB <= kActHalfB && kActHalfB % 16 == 0, "s_J fits the idle activation buffer");
    constexpr int kCoefB = NPAD * 4 * 8, kEdgeB = 64 * RW * 8, kRedB = 4 * RW * (RW + 4) * 8;
    constexpr int kPhaseP = kCoefB + 2 * kEdgeB + kRedB;
    __shared__ __attribute__((aligned(16))) unsigned char s_shared[kActB > kPhaseP ? kActB : kPhaseP];
    auto& s_act = *reinterpret_cast<float (*)[2][AW_MAX_ROWS][AW_MAX_WIDTH]>(s_shared);
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

    // ---- N(q_p) and dN/dq_p at q_p = s_q, float32 forward mode: rows 0 = value, 1 .. n = tangent directions --------
    // Layer l on all 256 threads.  A thread owns 4 outputs (one 16-byte weight load per input k, no guards: the host pads
    // W^T to [in4][ld]) and every KPw-th group of 4 inputs; lane = (input slice) * P + (output group), so that neighbouring
    // lanes read neighbouring 16-byte chunks of a weight row.  NRT = rows compiled in.  Returns the buffer of the outputs.
    auto mlp_impl = [&](auto nrt_c) __attribute__((always_inline)) -> int {
        constexpr int NRT = decltype(nrt_c)::value;
        int cur = 0;
        if (tid < RW) {                                              // inputs padded with zeros to a multiple of 4
            s_act[0][0][tid] = tid < n ? (float)s_q[tid] : 0.0f;
#pragma unroll
            for (int r = 1; r < NRT; ++r) s_act[0][r][tid] = (r - 1 == tid && tid < n) ? 1.0f : 0.0f;
        }
        __syncthreads();
        for (int l = 0; l < a.nl; ++l) {
            const int in4 = (a.width[l] + 3) & ~3, out = a.width[l + 1], ldw = (out + 7) & ~7, ogn = ldw >> 2;
            int P = 1, pshift = 0;
            while (4 * P < ogn) { P <<= 1; ++pshift; }                // output groups per wave (a power of two, <= 16)
            int KPw = 64 >> pshift;                                   // input slices per wave ...
            while (4 * KPw > in4 && KPw > 1) KPw >>= 1;               // ... at most one per group of 4 inputs (small layers)
            const int kp = lane >> pshift, ogr = w * P + (lane & (P - 1));
            const int og = ogr < ogn ? ogr : ogn - 1;                 // spare lanes redo the last group (no guarded loads)
            const float* __restrict__ wp = a.wt[l] + 4 * og;
            // the output this lane finishes after the fold (row rho of the wave: output rho of the thread's four)
            const int o0 = 4 * og + (lane >> 4);
            const float bias_0 = a.bias[l] ? a.bias[l][o0 < out ? o0 : out - 1] : 0.0f;
            float acc[NRT][4];
#pragma unroll
            for (int r = 0; r < NRT; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = 0.0f;
            auto kload = [&](int kb, float4 (&wv)[4]) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) wv[kk] = *reinterpret_cast<const float4*>(wp + (size_t)(kb + kk) * ldw);
            };
            auto kfma = [&](int kb, const float4 (&wv)[4]) {
#pragma unroll
                for (int r = 0; r < NRT; ++r) {
                    const float4 xv = *reinterpret_cast<const float4*>(&s_act[cur][r][kb]);
                    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        acc[r][0] = __builtin_fmaf(xs[kk], wv[kk].x, acc[r][0]); acc[r][1] = __builtin_fmaf(xs[kk], wv[kk].y, acc[r][1]);
                        acc[r][2] = __builtin_fmaf(xs[kk], wv[kk].z, acc[r][2]); acc[r][3] = __builtin_fmaf(xs[kk], wv[kk].w, acc[r][3]);
                    }
                }
            };
            // two slices per trip (8 weight loads in flight) where the registers allow it: at 18 and 21 rows that loop spills
            const int kstride = 4 * KPw;
            int kb = kp < KPw ? 4 * kp : in4;                         // lanes beyond the span hold zeros: the fold adds them
            if constexpr (NRT <= 10) {
                for (; kb + kstride < in4; kb += 2 * kstride) {
                    float4 wa[4], wb[4];
                    kload(kb, wa);
                    kload(kb + kstride, wb);
                    kfma(kb, wa);
                    kfma(kb + kstride, wb);
                }
            }
            for (; kb < in4; kb += kstride) {
                float4 wa[4];
                kload(kb, wa);
                kfma(kb, wa);
            }
            // fold the input slices (lanes P apart): inside a row of 16 lanes with shifts towards the higher lanes, so the
            // row total lands in its last P lanes ...
            auto fold = [&](auto get) {
#pragma unroll
                for (int r = 0; r < NRT; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[r][c] += get(acc[r][c]);
            };
            if (P <= 1) fold([](float v) { return dpp_f32<0x111>(v); });      // row_shr:1
            if (P <= 2) fold([](float v) { return dpp_f32<0x112>(v); });      // row_shr:2
            if (P <= 4) fold([](float v) { return dpp_f32<0x114>(v); });      // row_shr:4
            if (P <= 8) fold([](float v) { return dpp_f32<0x118>(v); });      // row_shr:8
            // ... and across the four rows with v_permlane16_swap / v_permlane32_swap (VALU, not the LDS pipe).  One swap +
            // add folds two values, paired so that row rho of the wave ends up with the total of output rho of the thread's
            // four, for ALL rows: the value and its tangent rows meet in one lane, which applies bias, activation and
            // derivative scaling in registers -- one barrier per layer.
            float res[NRT];
#pragma unroll
            for (int r = 0; r < NRT; ++r) {
                const float s01 = swap16_add(acc[r][0], acc[r][1]);
                const float s23 = swap16_add(acc[r][2], acc[r][3]);
                res[r] = swap32_add(s01, s23);
            }
            const int kind = a.act[l];
            const float alpha = a.alpha[l];
            if ((lane & 15) >= 16 - P && ogr < ogn) {
                const bool real = o0 < out;
                float av, d;                                         // bias, activation, derivative scaling
                mlp_activate(kind, alpha, res[0] + (real ? bias_0 : 0.0f), av, d);
                s_act[cur ^ 1][0][o0] = real ? av : 0.0f;            // the padding outputs feed the next layer's padded inputs
#pragma unroll
                for (int r = 1; r < NRT; ++r)
                    s_act[cur ^ 1][r][o0] = real ? ((kind != BG_ACT_NONE) ? res[r] * d : res[r]) : 0.0f;
            }
            __syncthreads();
            cur ^= 1;
        }
        return cur;
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
                if (tid < AW_MAX_NBAR) s_f[tid] = tid < nbar ? (double)s_act[cur][0][tid] : 0.0;
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
    if (max_nbar) *max_nbar = AW_MAX_NBAR;
    if (max_width) *max_width = AW_MAX_WIDTH;
    if (max_layers) *max_layers = AW_MAX_LAYERS;
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
    if (n > AW_MAX_N || nbar > AW_MAX_NBAR || n_layers > AW_MAX_LAYERS) return BG_ERR_UNSUPPORTED_R;
    if (!widths || !wt || !bias || !acts || !alphas) return BG_ERR_BAD_ARG;
    if (widths[0] != n || widths[n_layers] != nbar) return BG_ERR_BAD_ARG;
    AnnWideArgs a;
    for (int l = 0; l < n_layers; ++l) {
        if (widths[l + 1] < 1 || widths[l + 1] > AW_MAX_WIDTH) return BG_ERR_UNSUPPORTED_R;
        if (!wt[l] || ((uintptr_t)wt[l] & 15)) return BG_ERR_BAD_ARG;
        if (acts[l] != BG_ACT_NONE && acts[l] != BG_ACT_ELU && acts[l] != BG_ACT_RELU && acts[l] != BG_ACT_TANH) return BG_ERR_BAD_ARG;
        a.wt[l] = wt[l]; a.bias[l] = bias[l]; a.act[l] = acts[l]; a.alpha[l] = alphas[l];
    }
    for (int l = 0; l <= n_layers; ++l) a.width[l] = widths[l];
    if (B == 0) return BG_OK;
    if (!x || !UT || !u0 || !mu1 || !mu2 || !hist || !flags || !info || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    if ((uintptr_t)UT & 15) return BG_ERR_BAD_ARG;       // 16-byte loads
    a.x = x; a.UT = UT; a.u0 = u0; a.mu1 = mu1; a.mu2 = mu2; a.hist = hist; a.iters = iters; a.flags = flags;
    a.info = info; a.order = order; a.nl = n_layers; a.dt = dt; a.E = E; a.tol = tol; a.N = N; a.B = B; a.n = n; a.nbar = nbar;
    a.nsteps = nsteps; a.max_it = max_it; a.supg = options & BG_OPT_SUPG; a.nonuniform = (options & BG_OPT_NONUNIFORM) ? 1 : 0;
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
