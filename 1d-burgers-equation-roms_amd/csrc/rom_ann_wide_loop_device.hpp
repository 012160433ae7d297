// rom_ann_wide_loop_device.hpp -- the POD-ANN PROM time loop of one sample on one 256-thread workgroup for up to 20 primary
// modes, as a body two files instantiate: rom_ann_wide.hip (bg_ann_rom_run_wide: the mesh itself, N <= 512) and
// rom_hyper_ann_wide.hip (bg_hyper_ann_rom_run_wide: the compacted mesh of a row sampling's stencil nodes, any N).  The phases
// of an iteration are described in rom_ann_wide.hip; this file holds the input set-up, the tables s_f and s_J, the LDS
// overlay and the loop.  The mesh side is rom_closure_device.hpp's, the closure MLP rom_ann_device.hpp's.
//
// The hyper-reduced form (Args = HyperAnnWideRunArgs) is described in rom_hyper_table_device.hpp, which holds its table side;
// the blocks under `if constexpr (HYPER)` call it (the step write keeps its own text, see there).
// The closure value of a step's decode is the last evaluation's s_f.
#pragma once
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
constexpr int AW_UT_LD = 512;                  // row stride of UT: the largest N of bg_ann_rom_run_wide

// bg_hyper_ann_rom_run_wide: x, UT, u0 are the table's xn [nodes], UTn [n + nbar][UT_LD] (zero from nodes), u0n [B][nodes];
// hist is qhist [B][nsteps+1][n]; N is the mesh's node count (it decides the last row), nonuniform is not read
struct HyperAnnWideRunArgs : AnnRunArgs, HyperClosureTableArgs {};

// rows of the mesh the body works on
__device__ __forceinline__ int ann_wide_loop_rows(const AnnRunArgs& a) { return a.N; }
__device__ __forceinline__ int ann_wide_loop_rows(const HyperAnnWideRunArgs& a) { return a.nodes; }

// S: rows per owner (64 owners: 64 S rows), WPC: workgroups per CU the register budget is cut for, UT_LD: row stride of UT.
// The defaults are bg_ann_rom_run_wide's.
template <int S, int PROJ, int WPC = 2, int UT_LD = AW_UT_LD, class Args = AnnRunArgs>
__global__ __launch_bounds__(256, WPC) void rom_ann_wide_kernel(Args a)
{
    constexpr bool HYPER = std::is_same<Args, HyperAnnWideRunArgs>::value;
    constexpr int NB = AW_NB;
    constexpr int NPAD = 64 * S;
    constexpr int NIT = NPAD / 256;              // rows per thread of the strided loops
    constexpr int RW = 4 * NB;
    constexpr bool GAL = PROJ == BG_PROJ_GALERKIN;
    constexpr int kAccBudget = GAL ? 24 : 14;    // accumulators per projection pass (see rom_rbf_fused.hip)
    static_assert(NPAD <= UT_LD && NPAD % 256 == 0, "the strided loops and the fragments stay inside a row of UT");
    __shared__ double s_u[NPAD + 4];             // u at offset 2, zero halo on each side
    __shared__ double s_g[NPAD], s_h[NPAD];
    __shared__ double s_fdt[NPAD];               // dt F
    __shared__ double s_q[RW], s_x[RW];
    __shared__ double s_part[4][RW];             // per-wave partial sums of U_p^T u
    __shared__ double s_f[ANN_MAX_NBAR];         // N(q_p) of the latest evaluation
    __shared__ int s_info;
    // hyper-reduced form: the mesh row of every table node (a.N: only a neighbour, an identity row) and its weight factor
    __shared__ int s_hnode[HYPER ? NPAD : 1];
    __shared__ double s_hmul[HYPER ? NPAD : 1];
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
    const int N = ann_wide_loop_rows(a), n = a.n, nbar = a.nbar, nr = 1 + a.n;
    const int nonuniform = HYPER ? 1 : a.nonuniform;             // the table always is a non-uniform mesh
    const double h = HYPER ? 1.0 : (a.x[N - 1] - a.x[0]) / (double)(N - 1);      // (not read on a non-uniform mesh)
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

    // ---- hyper-reduced form: s_hnode, s_hmul of every table node, the same for every sample; scattered from pos / xi through
    // the LDS the phases share
    if constexpr (HYPER) {
        int* s_smp = reinterpret_cast<int*>(s_shared);          // [NPAD]: 1 + the sampled row at this table node, or 0
        static_assert(NPAD * 4 <= sizeof(s_shared), "the scatter table fits the shared block");
        hyper_scatter_rows<256>(s_smp, NPAD, a.pos, a.nrows, N, tid);
        for (int k = tid; k < NPAD; k += 256) hyper_table_node<GAL>(s_smp[k], k, a.node, a.xi, a.N, N, s_hnode[k], s_hmul[k]);
    }

    __builtin_amdgcn_s_setprio(3);
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
                sample_setup_row<false>(tid + 256 * ii, a.x, a.u0, smp, nullptr, N, mu2, h, nonuniform, a.dt, s_u, s_fdt, s_h);
            rederive();
            hyper_sample_start<256, RW>(a.q0, s_q, hist, a.qshist, smp, a.nsteps, n, nbar, tid, 0.0);
        } else {
#pragma unroll 1
            for (int ii = 0; ii < NIT; ++ii)
                sample_setup_row(tid + 256 * ii, a.x, a.u0, smp, hist, N, mu2, h, nonuniform, a.dt, s_u, s_fdt, s_h);
        }
        __syncthreads();

        int flags = 0, info_out = 0;
        for (int step = 0; step < a.nsteps && info_out == 0; ++step) {
            if constexpr (HYPER) {
                // ---- g = M u^n + dt F (:1214) at the table nodes; q_p carries over ----------------------------------------
#pragma unroll 1
                for (int ii = 0; ii < NIT; ++ii) {
                    const int i = tid + 256 * ii;
                    double g = 0.0;
                    if (i < N) g = rom_mass_rhs_node(a.x, i, N, s_u[i + 1], s_u[i + 2], s_u[i + 3], s_fdt[i], h, nonuniform);
                    s_g[i] = g;
                }
                __syncthreads();
            } else {
                // ---- g = M u^n + dt F (:1214) and q_p = U_p^T u^n (:1197) ----------------------------------------------
                project_q<NIT, 256, 4, UT_LD, RW>(UT, s_u, n, tid, lane, w, s_part, s_q, [&](int i, double uc) {
                    double g = 0.0;
                    if (i < N) g = rom_mass_rhs_node(a.x, i, N, s_u[i + 1], uc, s_u[i + 3], s_fdt[i], h, nonuniform);
                    s_g[i] = g;
                });
            }
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
                if (decode) decode_u<NIT, 256, UT_LD>(s_u, UT, s_q, s_f, N, n, nbar, tid);
                if (!more) break;
                decode = true;
                // ---- tangent W = U_p + U_s dN (:1224) in this lane's projection fragments -----------------------------------
                rederive();
                double frag[NB][S];
                tangent_fragments<S, NB, UT_LD>(frag, UT, s_J, n, nbar, rowbase, t);
                __syncthreads();                         // s_J consumed: the projection phase reuses its LDS
                publish_edges<S, NB>(frag, s_elo, s_ehi, owner, t);
                // ---- assembly: A(u_k), R(u_k) per row into LDS -------------------------------------------------------
                if constexpr (HYPER)
                    hyper_assemble_rows<NPAD, 256>(s_coef, s_hnode, s_hmul, s_u, s_g, s_h, a.x, a.N, h, a.dt, a.E, a.supg, mu1, tid);
                else
                    assemble_rows<NPAD, 256>(s_coef, s_u, s_g, s_h, a.x, N, h, a.dt, a.E, a.supg, nonuniform, mu1, tid);
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
            if constexpr (HYPER) {                  // q_p and the closure value of the decode: s_f is the last evaluation's
                rederive();
                // (inline: through hyper_write_step these three lines cost 16 / 30 / 4 more spilled SGPRs at S = 4 / 8 / 12)
                if (tid < n) hist[(size_t)(step + 1) * n + tid] = s_q[tid];
                double* qs = a.qshist + ((size_t)smp * (size_t)(a.nsteps + 1) + (size_t)(step + 1)) * (size_t)nbar;
                for (int j = tid; j < nbar; j += 256) qs[j] = s_f[j];
            } else
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
