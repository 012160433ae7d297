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
// This file holds the closure (scale, centre, the Jacobian and value tiles), the LDS overlay and the loop; the mesh side
// (q_p, tangent, halo edges, assembly, update of q_p, decode) is rom_closure_device.hpp's, shared with rom_ann_wide.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "rom_closure_device.hpp"

namespace {

using namespace bg;
using namespace bg::fused;

constexpr int RBF_NB = 5;                    // column blocks of the projection: n <= 20
constexpr int RBF_MAX_N = 4 * RBF_NB;
constexpr int RBF_MAX_NBAR = 128;            // Wd and bias are padded to this many columns
constexpr int RBF_MAX_NS = 1 << 16;          // centres: streamed in tiles, the bound only keeps Ns * 128 in int range
constexpr int RBF_UT_LD = 512;               // row stride of UT: the largest N of bg_rbf_rom_run
constexpr int RBF_LONG_UT_LD = 1024;         // ... and of bg_rbf_rom_run_long
constexpr int RBF_TILE = 128;                // centres per LDS tile
constexpr int RBF_GS = 24;                   // s_G row: wave w's five k = 5 w .. 5 w + 4 at [6 w .. 6 w + 4] (16-byte reads)

struct RbfRunArgs {
    const double* x;        // [N]
    const double* UT;       // [n + nbar][UT_LD]: rows 0 .. n-1 = U_p^T, rows n .. n+nbar-1 = U_s^T, zero columns from N
    const double* XtT;      // [n][Ns] centres, centre index fastest
    const double* Wd;       // [Ns][128] W dy/2, zero columns from nbar
    const double* bias;     // [128] dy/2 + y_min, zero from nbar
    const double* x_min;    // [n]
    const double* dx;       // [n] x_max - x_min with entries below 1e-15 replaced by 1
    const double* u0;       // [B][N]
    const double* mu1;      // [B]
    const double* mu2;      // [B]
    double* hist;           // [B][nsteps+1][N]
    int32_t* iters;         // [B][nsteps]
    int32_t* flags;         // [B]
    int32_t* info;          // [B]
    const int32_t* order;   // [B] or null: slot i of the persistent loop works on sample order[i]
    double eps2, dt, E, tol;
    int N, B, n, nbar, Ns, nsteps, max_it, kind, supg, nonuniform;
};

// UT_LD: the row stride of UT; NW: waves per workgroup.  The defaults are bg_rbf_rom_run's: four waves, 64 owners of S rows,
// two workgroups per CU.  bg_rbf_rom_run_long runs the same code at S = 8 on eight waves (N <= 1024: 128 owners), one
// workgroup per CU: the register profile and the two waves per SIMD of the S = 8 instantiation, 141 KB of LDS.  What the
// eight waves change: one partial system per wave summed in a fixed order (NRED = 8), waves 4 .. 7 take the second half of
// every centre tile in the Jacobian, the value phase splits a tile in four, the strided loops step by 512.
template <int S, int PROJ, int UT_LD = RBF_UT_LD, int NW = 4>
__global__ __launch_bounds__(64 * NW, 8 / NW) void rom_rbf_fused_kernel(RbfRunArgs a)
{
    static_assert(NW == 4 || NW == 8, "four waves, or eight: 128 owners of S rows each");
    constexpr int NB = RBF_NB;
    constexpr int NT = 64 * NW, NOWN = 16 * NW;  // threads, owners of S rows
    constexpr int NPAD = NOWN * S;
    constexpr int NIT = NPAD / NT;               // rows per thread of the strided loops
    constexpr int NP = NT / RBF_MAX_NBAR;        // parts of a tile in the value phase
    constexpr int RW = 4 * NB;
    constexpr bool GAL = PROJ == BG_PROJ_GALERKIN;
    // Accumulators per projection pass next to the 2 S NB fragment registers: two passes for either form (Galerkin 30 as
    // 20 + 10, LSPG 25 as 11 + 14; its operand formation keeps more live).  Larger budgets spill at S = 8
    // (kernel-resource-usage); the per-row loops outside the iteration are kept rolled (#pragma unroll 1) for the same reason.
    constexpr int kAccBudget = GAL ? 24 : 14;
    __shared__ double s_u[NPAD + 4];             // u at offset 2, zero halo on each side
    __shared__ double s_g[NPAD], s_h[NPAD];
    __shared__ double s_fdt[NPAD];              // dt F (in LDS: live across the whole sample, it took registers from the projection)
    __shared__ double s_q[RW], s_x[RW], s_xs[RW], s_sc[RW];
    __shared__ double s_part[NW][RW];            // per-wave partial sums of U_p^T u
    __shared__ double s_fp[NP][RBF_MAX_NBAR];    // closure value: partial sums of the NP parts of every tile
    __shared__ double s_f[RBF_MAX_NBAR];
    __shared__ int s_info;
    // Phases of an iteration never overlap in time and share one block of LDS (four waves: two workgroups per CU need <= 80 KB each):
    //   Jacobian + tangent: s_G, s_J  |  assembly + projection + solve: s_coef, s_elo, s_ehi, s_red  |  value: s_phi
    constexpr int kGB = RBF_TILE * RBF_GS * 8, kJB = RBF_MAX_NBAR * RW * 8;
    constexpr int kCoefB = NPAD * 4 * 8, kEdgeB = NOWN * RW * 8, kRedB = NW * RW * (RW + 4) * 8;
    constexpr int kPhaseJ = kGB + kJB, kPhaseP = kCoefB + 2 * kEdgeB + kRedB;
    __shared__ __attribute__((aligned(16))) unsigned char s_shared[kPhaseJ > kPhaseP ? kPhaseJ : kPhaseP];
    auto& s_G = *reinterpret_cast<double (*)[RBF_TILE][RBF_GS]>(s_shared);
    auto& s_J = *reinterpret_cast<double (*)[RBF_MAX_NBAR][RW]>(s_shared + kGB);
    auto& s_coef = *reinterpret_cast<double (*)[NPAD][4]>(s_shared);
    auto& s_elo = *reinterpret_cast<double (*)[NOWN][RW]>(s_shared + kCoefB);
    auto& s_ehi = *reinterpret_cast<double (*)[NOWN][RW]>(s_shared + kCoefB + kEdgeB);
    auto& s_red = *reinterpret_cast<double (*)[NW][RW][RW + 4]>(s_shared + kCoefB + 2 * kEdgeB);
    auto& s_phi = *reinterpret_cast<double (*)[RBF_TILE]>(s_shared);

    // The thread-index family is re-derived from an opaque copy at the top of every Gauss-Newton pass and of its register-heavy
    // phases: per-lane addresses are loop invariants of the whole kernel, and hoisted out of the loops they end up in scratch.
    int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform by construction
    int t = lane & 3, owner = 16 * w + (lane >> 2);
    int rowbase = owner * S;
    auto rederive = [&]() {
        int v = threadIdx.x;
        asm volatile("" : "+v"(v));
        tid = v; lane = v & 63; t = lane & 3; owner = 16 * w + (lane >> 2); rowbase = owner * S;
    };
    const int N = a.N, n = a.n, nbar = a.nbar, Ns = a.Ns;
    const double h = (a.x[N - 1] - a.x[0]) / (double)(N - 1);
    const double* __restrict__ UT = a.UT;

    if (tid < 4) s_u[tid < 2 ? tid : NPAD + tid] = 0.0;

    // xs = 2 (q - x_min) / dx - 1 and 2 / dx at q = s_q (csrc/rbf.hip); zero beyond n
    auto scale = [&]() {
        if (tid < RW) {
            const bool in = tid < n;
            const double xm = in ? a.x_min[tid] : 0.0, d = in ? a.dx[tid] : 1.0;
            s_xs[tid] = in ? 2.0 * ((s_q[tid] - xm) / d) - 1.0 : 0.0;
            s_sc[tid] = in ? 2.0 / d : 0.0;
        }
        __syncthreads();
    };
    // phi and gradient coefficient of centre i at s_xs; repeats rbf_device.hpp (shared, this kernel's branches and spills change)
    auto centre = [&](int i, double (&d)[RW], double& p, double& coef) {
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < RW; ++k) {
            d[k] = 0.0;
            if (k < n) {
                d[k] = s_xs[k] - a.XtT[(size_t)k * Ns + i];
                r2 = __builtin_fma(d[k], d[k], r2);
            }
        }
        if (a.kind == BG_RBF_GAUSSIAN) {
            p = exp(-a.eps2 * r2);
            coef = -2.0 * a.eps2 * p;
        } else {
            p = 1.0 / sqrt(1.0 + a.eps2 * r2);
            coef = -a.eps2 * (p * p * p);
        }
    };

    for (int slot = blockIdx.x; slot < a.B; slot += gridDim.x) {
        const int smp = a.order ? a.order[slot] : slot;
        if (smp < 0 || smp >= a.B) continue;                 // untrusted order entry: the same for the whole workgroup
        const double mu1 = a.mu1[smp], mu2 = a.mu2[smp];
        double* hist = a.hist + (size_t)smp * (size_t)(a.nsteps + 1) * (size_t)N;
        __syncthreads();
        // ---- per-sample constants (compute_forcing_vector :427-461, f_gp of :556-558) and the initial state ----------
#pragma unroll 1
        for (int ii = 0; ii < NIT; ++ii)
            sample_setup_row(tid + NT * ii, a.x, a.u0, smp, hist, N, mu2, h, a.nonuniform, a.dt, s_u, s_fdt, s_h);
        __syncthreads();

        int flags = 0, info_out = 0;
        for (int step = 0; step < a.nsteps && info_out == 0; ++step) {
            // ---- g = M u^n + dt F (:1330) ------------------------------------------------------------------------------
#pragma unroll 1
            for (int ii = 0; ii < NIT; ++ii) {
                const int i = tid + NT * ii;
                double g = 0.0;
                if (i < N) g = rom_mass_rhs_node(a.x, i, N, s_u[i + 1], s_u[i + 2], s_u[i + 3], s_fdt[i], h, a.nonuniform);
                s_g[i] = g;
            }
            __syncthreads();
            int k = 0;
            bool more = true;
            while (more) {
                rederive();
                // ---- q_p = U_p^T U0 (:1352) -------------------------------------------------------------------------
                project_q<NIT, NT, NW, UT_LD, RW>(UT, s_u, n, tid, lane, w, s_part, s_q, [](int, double) {});
                scale();
                // ---- closure Jacobian at q_p (:238-260): J[j][k] = sum_i Wd[i][j] G[i][k] ----------------------------
                // thread (w, lane) owns j = 2 lane, 2 lane + 1 and k = 5 w .. 5 w + 4: per centre one 16-byte load of Wd
                // (L2, shared by the four waves), three broadcast LDS reads of G, ten FMAs.  Eight waves: k = 5 (w & 3) ...,
                // waves 4 .. 7 take the second half of every tile and add their sums onto those of waves 0 .. 3 in LDS
                {
                    const int wk = NW == 8 ? (w & 3) : w;
                    double jacc[2][5];
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int kk = 0; kk < 5; ++kk) jacc[e][kk] = 0.0;
                    for (int i0 = 0; i0 < Ns; i0 += RBF_TILE) {
                        __syncthreads();                 // the previous tile is consumed
                        if (tid < RBF_TILE) {
                            const int i = i0 + tid;
                            double d[RW], p = 0.0, coef = 0.0;
                            if (i < Ns) centre(i, d, p, coef);
                            else {
#pragma unroll
                                for (int kk = 0; kk < RW; ++kk) d[kk] = 0.0;
                            }
#pragma unroll
                            for (int kk = 0; kk < RW; ++kk) s_G[tid][6 * (kk / 5) + kk % 5] = (coef * s_sc[kk]) * d[kk];
                        }
                        __syncthreads();
                        const int tn = (Ns - i0 < RBF_TILE) ? Ns - i0 : RBF_TILE;
                        const int ib = NW == 8 ? (w >> 2) * (RBF_TILE / 2) : 0;
                        const int ie = (NW == 8 && ib + RBF_TILE / 2 < tn) ? ib + RBF_TILE / 2 : tn;
                        const double* __restrict__ wrow = a.Wd + (size_t)i0 * RBF_MAX_NBAR + 2 * lane;
#pragma unroll 8
                        for (int ii = ib; ii < ie; ++ii) {
                            const double2 wd = *reinterpret_cast<const double2*>(wrow + (size_t)ii * RBF_MAX_NBAR);
                            const double2 g01 = *reinterpret_cast<const double2*>(&s_G[ii][6 * wk]);
                            const double2 g23 = *reinterpret_cast<const double2*>(&s_G[ii][6 * wk + 2]);
                            const double g4 = s_G[ii][6 * wk + 4];
                            const double g[5] = {g01.x, g01.y, g23.x, g23.y, g4};
#pragma unroll
                            for (int kk = 0; kk < 5; ++kk) {
                                jacc[0][kk] = __builtin_fma(wd.x, g[kk], jacc[0][kk]);
                                jacc[1][kk] = __builtin_fma(wd.y, g[kk], jacc[1][kk]);
                            }
                        }
                    }
                    if constexpr (NW == 4) {
#pragma unroll
                        for (int e = 0; e < 2; ++e)
#pragma unroll
                            for (int kk = 0; kk < 5; ++kk) s_J[2 * lane + e][5 * w + kk] = jacc[e][kk];
                    } else if (w < 4) {
#pragma unroll
                        for (int e = 0; e < 2; ++e)
#pragma unroll
                            for (int kk = 0; kk < 5; ++kk) s_J[2 * lane + e][5 * wk + kk] = jacc[e][kk];
                    }
                    __syncthreads();
                    if constexpr (NW == 8) {             // every entry gets exactly one add: the sum does not depend on timing
                        if (w >= 4) {
#pragma unroll
                            for (int e = 0; e < 2; ++e)
#pragma unroll
                                for (int kk = 0; kk < 5; ++kk) s_J[2 * lane + e][5 * wk + kk] += jacc[e][kk];
                        }
                        __syncthreads();
                    }
                }
                // ---- tangent W = U_p + U_s J (:1361) in this lane's projection fragments ------------------------------
                rederive();
                double frag[NB][S];
                tangent_fragments<S, NB, UT_LD>(frag, UT, s_J, n, nbar, rowbase, t);
                __syncthreads();                         // s_J consumed: the projection phase reuses its LDS
                publish_edges<S, NB>(frag, s_elo, s_ehi, owner, t);
                // ---- assembly: A(u_k), R(u_k) per row into LDS (:1330-1346) ------------------------------------------
                assemble_rows<NPAD, NT>(s_coef, s_u, s_g, s_h, a.x, N, h, a.dt, a.E, a.supg, a.nonuniform, mu1, tid);
                __syncthreads();
                // ---- projection (:1361) ------------------------------------------------------------------------------
                {
                    double (*s_wtu)[RW] = s_part;        // the Phi^T u extras of the LSPG pass: not used here
                    mfma_passes<S, NB, GAL, RW, NW, kAccBudget>(frag, HaloEdges<NB, NOWN - 1>{s_elo, s_ehi, owner, t}, s_coef, s_u,
                                                               rowbase, t, w, lane, s_red, s_wtu);
                }
                __syncthreads();
                // ---- reduced solve with partial pivoting (np.linalg.solve :1365) -------------------------------------
                if (w == 0) pivoted_solve<NB, GAL, NW>(s_red, s_x, &s_info, lane, n);
                __syncthreads();
                if (s_info != 0 && info_out == 0) info_out = s_info;
                // ---- q_new = q_p + dq, err = |dq| / |q_new| (|dq| when |q_new| = 0) (:1366-1390) ----------------------
                const double err = update_q<RW>(s_q, s_x, n, lane, w, [](double nd, double nq) { return nq > 0.0 ? nd / nq : nd; });
                ++k;
                more = (err > a.tol) && (k < a.max_it) && info_out == 0;
                if (!(err - err == 0.0)) flags |= BG_FLAG_NONFINITE;
                if (k >= a.max_it) flags |= BG_FLAG_HIT_CAP;
                scale();
                // ---- closure value at q_new (:225-236): f_j = sum_i phi_i Wd[i][j] + bias_j --------------------------
                rederive();
                {
                    const int j = tid & (RBF_MAX_NBAR - 1), half = tid >> 7;
                    double facc = 0.0;
                    for (int i0 = 0; i0 < Ns; i0 += RBF_TILE) {
                        __syncthreads();
                        if (tid < RBF_TILE) {
                            const int i = i0 + tid;
                            double d[RW], p = 0.0, coef;
                            if (i < Ns) centre(i, d, p, coef);
                            s_phi[tid] = p;
                        }
                        __syncthreads();
                        const int tn = (Ns - i0 < RBF_TILE) ? Ns - i0 : RBF_TILE;
                        const int ib = half * (RBF_TILE / NP), ie = (ib + RBF_TILE / NP < tn) ? ib + RBF_TILE / NP : tn;
                        const double* __restrict__ wcol = a.Wd + (size_t)i0 * RBF_MAX_NBAR + j;
#pragma unroll 8
                        for (int ii = ib; ii < ie; ++ii) facc = __builtin_fma(s_phi[ii], wcol[(size_t)ii * RBF_MAX_NBAR], facc);
                    }
                    s_fp[half][j] = facc;
                    __syncthreads();
                    if constexpr (NP == 2) {
                        if (tid < RBF_MAX_NBAR) s_f[tid] = (s_fp[0][tid] + s_fp[1][tid]) + a.bias[tid];
                    } else {
                        if (tid < RBF_MAX_NBAR) s_f[tid] = ((s_fp[0][tid] + s_fp[1][tid]) + (s_fp[2][tid] + s_fp[3][tid])) + a.bias[tid];
                    }
                    __syncthreads();
                }
                // ---- decode U1 = U_p q_new + U_s f (:1378-1381) ------------------------------------------------------
                rederive();
                decode_u<NIT, NT, UT_LD>(s_u, UT, s_q, s_f, N, n, nbar, tid);
            }
            write_hist_row<NT>(hist + (size_t)(step + 1) * N, s_u, N, tid);
            if (tid == 0) a.iters[(size_t)smp * a.nsteps + step] = k;
        }
        if (tid == 0) {
            a.flags[smp] = flags;
            a.info[smp] = info_out;
        }
    }
}

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
