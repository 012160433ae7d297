// rom_rbf_loop_device.hpp -- the POD-RBF PROM time loop of one sample on one workgroup, as a body two files instantiate:
// rom_rbf_fused.hip (bg_rbf_rom_run, bg_rbf_rom_run_long: the mesh itself, N <= 1024) and rom_hyper_rbf.hip
// (bg_hyper_rbf_rom_run: the compacted mesh of a row sampling's stencil nodes, any N).  The phases of an iteration are
// described in rom_rbf_fused.hip; this file holds the closure (scale, centre, the Jacobian and value tiles), the LDS overlay
// and the loop; the mesh side is rom_closure_device.hpp's.
//
// The hyper-reduced form (Args = HyperRbfRunArgs) is described in rom_hyper_table_device.hpp, which holds its table side; the
// blocks under `if constexpr (HYPER)` call it.  The closure value of a step's decode is f(q_p), the last evaluation's s_f.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "rom_closure_device.hpp"

namespace {

using namespace bg;
using namespace bg::fused;

constexpr int RBF_NB = 5;                   // column blocks of the projection: n <= 20
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

// bg_hyper_rbf_rom_run: x, UT, u0 are the table's xn [nodes], UTn [n + nbar][UT_LD] (zero from nodes), u0n [B][nodes]; hist
// is qhist [B][nsteps+1][n]; N is the mesh's node count (it decides the last row), nonuniform is not read
struct HyperRbfRunArgs : RbfRunArgs, HyperClosureTableArgs {};

// rows of the mesh the body works on
__device__ __forceinline__ int rbf_loop_rows(const RbfRunArgs& a) { return a.N; }
__device__ __forceinline__ int rbf_loop_rows(const HyperRbfRunArgs& a) { return a.nodes; }

// UT_LD: the row stride of UT; NW: waves per workgroup.  The defaults are bg_rbf_rom_run's: four waves, 64 owners of S rows,
// two workgroups per CU.  bg_rbf_rom_run_long runs the same code at S = 8 on eight waves (N <= 1024: 128 owners), one
// workgroup per CU: the register profile and the two waves per SIMD of the S = 8 instantiation, 141 KB of LDS.  What the
// eight waves change: one partial system per wave summed in a fixed order (NRED = 8), waves 4 .. 7 take the second half of
// every centre tile in the Jacobian, the value phase splits a tile in four, the strided loops step by 512.
template <int S, int PROJ, int UT_LD = RBF_UT_LD, int NW = 4, class Args = RbfRunArgs>
__global__ __launch_bounds__(64 * NW, 8 / NW) void rom_rbf_fused_kernel(Args a)
{
    constexpr bool HYPER = std::is_same<Args, HyperRbfRunArgs>::value;
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
    // hyper-reduced form: the mesh row of every table node (a.N: only a neighbour, an identity row) and its weight factor
    __shared__ int s_hnode[HYPER ? NPAD : 1];
    __shared__ double s_hmul[HYPER ? NPAD : 1];
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
    const int N = rbf_loop_rows(a), n = a.n, nbar = a.nbar, Ns = a.Ns;
    const int nonuniform = HYPER ? 1 : a.nonuniform;             // the table always is a non-uniform mesh
    const double h = HYPER ? 1.0 : (a.x[N - 1] - a.x[0]) / (double)(N - 1);      // (not read on a non-uniform mesh)
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

    // ---- hyper-reduced form: s_hnode, s_hmul of every table node, the same for every sample; scattered from pos / xi through
    // the LDS the phases share
    if constexpr (HYPER) {
        int* s_smp = reinterpret_cast<int*>(s_shared);          // [NPAD]: 1 + the sampled row at this table node, or 0
        static_assert(NPAD * 4 <= sizeof(s_shared), "the scatter table fits the shared block");
        hyper_scatter_rows<NT>(s_smp, NPAD, a.pos, a.nrows, N, tid);
        for (int k = tid; k < NPAD; k += NT) hyper_table_node<GAL>(s_smp[k], k, a.node, a.xi, a.N, N, s_hnode[k], s_hmul[k]);
    }

    for (int slot = blockIdx.x; slot < a.B; slot += gridDim.x) {
        const int smp = a.order ? a.order[slot] : slot;
        if (smp < 0 || smp >= a.B) continue;                 // untrusted order entry: the same for the whole workgroup
        const double mu1 = a.mu1[smp], mu2 = a.mu2[smp];
        double* hist = a.hist + (size_t)smp * (size_t)(a.nsteps + 1) * (size_t)(HYPER ? n : N);      // HYPER: q_p of every step
        __syncthreads();
        // ---- per-sample constants (compute_forcing_vector :427-461, f_gp of :556-558) and the initial state ----------
        if constexpr (HYPER) {                      // u0 at the table nodes, q_p = q0 (the caller's U_p^T u0); no closure value belongs to u0
#pragma unroll 1
            for (int ii = 0; ii < NIT; ++ii)
                sample_setup_row<false>(tid + NT * ii, a.x, a.u0, smp, nullptr, N, mu2, h, nonuniform, a.dt, s_u, s_fdt, s_h);
            rederive();
            double zero = 0.0;
            asm volatile("" : "+v"(zero));         // (as a constant it was kept in registers for the whole kernel, and spilled)
            hyper_sample_start<NT, RW>(a.q0, s_q, hist, a.qshist, smp, a.nsteps, n, nbar, tid, zero);
        } else {
#pragma unroll 1
            for (int ii = 0; ii < NIT; ++ii)
                sample_setup_row(tid + NT * ii, a.x, a.u0, smp, hist, N, mu2, h, nonuniform, a.dt, s_u, s_fdt, s_h);
        }
        __syncthreads();

        int flags = 0, info_out = 0;
        // (HYPER: the step count as a scalar by construction -- as a vector pair it went to scratch on eight waves)
        auto next = [](int s) { if constexpr (HYPER) return __builtin_amdgcn_readfirstlane(s + 1); else return s + 1; };
        for (int step = 0; step < a.nsteps && info_out == 0; step = next(step)) {
            // ---- g = M u^n + dt F (:1330) ------------------------------------------------------------------------------
#pragma unroll 1
            for (int ii = 0; ii < NIT; ++ii) {
                const int i = tid + NT * ii;
                double g = 0.0;
                if (i < N) g = rom_mass_rhs_node(a.x, i, N, s_u[i + 1], s_u[i + 2], s_u[i + 3], s_fdt[i], h, nonuniform);
                s_g[i] = g;
            }
            __syncthreads();
            int k = 0;
            bool more = true;
            while (more) {
                rederive();
                // ---- q_p = U_p^T U0 (:1352); HYPER: q_p carries over ------------------------------------------------
                if constexpr (!HYPER)
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
                if constexpr (HYPER)
                    hyper_assemble_rows<NPAD, NT>(s_coef, s_hnode, s_hmul, s_u, s_g, s_h, a.x, a.N, h, a.dt, a.E, a.supg, mu1, tid);
                else
                    assemble_rows<NPAD, NT>(s_coef, s_u, s_g, s_h, a.x, N, h, a.dt, a.E, a.supg, nonuniform, mu1, tid);
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
            if constexpr (HYPER) {                  // q_p and the closure value of the decode
                rederive();                         // (the per-lane output addresses, hoisted out of the time loop, went to scratch)
                hyper_write_step<NT>(hist, a.qshist, smp, a.nsteps, step, s_q, s_f, n, nbar, tid);
            } else
                write_hist_row<NT>(hist + (size_t)(step + 1) * N, s_u, N, tid);
            if (tid == 0) a.iters[(size_t)smp * a.nsteps + step] = k;
        }
        if (tid == 0) {
            a.flags[smp] = flags;
            a.info[smp] = info_out;
        }
    }
}

}  // namespace
