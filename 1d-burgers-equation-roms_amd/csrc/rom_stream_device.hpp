// rom_stream_device.hpp -- the whole POD-PROM time loop of one sample on one compute unit with the basis STREAMED through
// LDS: the one source of bg_rom_run_wide (rom_wide.hip, 40 < r <= 96, N <= 512), bg_rom_run_long (rom_long.hip, r <= 40,
// 513 <= N <= 1024), bg_rom_run_long_wide (rom_long_wide.hip, 40 < r <= 96 on those meshes) and bg_local_rom_run_long
// (rom_local_long.hip, local POD on the same meshes).
// reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785; local_prom_burgers, :979-1079.
//
// bg_rom_run (rom_fused.hip) keeps the basis in registers.  Here it streams through LDS, 64 mesh rows at a time (one pass over
// the padded copy PhiP per Picard iteration, L2-resident), and what stays in registers are the ACCUMULATORS of the reduced
// system: its 4 x 4 block pairs are dealt round-robin to the four waves (one wave per SIMD), every wave sweeps ALL mesh rows
// for its own pairs, so there are no per-wave partial systems to add up.  The slabs are double buffered and arrive by LDS
// DMA (global_load_lds: no registers, the next slab lands while this one is worked on).  Per slab:
//   four lanes per row lift u = Phi q for rows i - 1, i, i + 1 (:773; iterations after the first) and assemble A(u), R(u)
//   of row i (:730-753, rom_assemble_row)  ->  each wave forms the rows of Y = A Phi it multiplies, from the slab and the
//   coefficients in LDS (lane (k, blk, t): mesh row 4 k + blk of the 16-row step, columns NB t + c for block c: NB / 2
//   16-byte reads per row)  ->  v_mfma_f64_4x4x4_4b.  Two workgroup barriers per slab.
// Then the reduced system is parked in LDS over the dead slabs and solved (the kernel's own step), q = Phi^T u + dq, the
// stopping test, and after the last iteration one lift-only sweep for U[:, n+1] = Phi q (:779).
//
// What the kernels do not share is stated once per kernel in a description K (WidePod, LongWidePod, LongPod, LongLocal):
//   K::NB                        4-column blocks of the padded reduced dimension R = 4 NB: column NB t + c <-> (lane index t, block c)
//   K::PS, K::SW                 doubles per row of the LDS slabs and of the parked system Ar | br | Phi^T u (16-byte aligned rows)
//   K::NMAX                      mesh rows held: the length of u, g, h_f, dt F in LDS and of every per-node loop
//   K::cf_by_mesh_row            the coefficients lo, di, up, R in LDS are indexed by mesh row (all NMAX kept) or by slab row (one slab's)
//   K::mirror_lspg               LSPG parks the lower block pairs too; otherwise the solve reads them through a symmetric accessor
//   K::has_repair                a second instantiation PIV redoes the samples marked BG_INFO_NEEDS_PIVOTING (and only those)
//   K::solve_update<GAL, PIV, W> solve(Ar, -br) of the parked system (r live unknowns) by all four waves, q = Phi^T u + dq into L.q,
//                                |dq|^2 and |q|^2
//   K::Args                      the kernel's argument struct: StreamRunArgs, or LocalStreamRunArgs when K::local
//   K::local                     local POD: at the top of every time step the nearest centre to U_g^T u^n picks the step's basis
//                                (a block of the stack PhiP [C][NPAD + 2][R]) and its width; the sweep streams that block
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "rom_device.hpp"

namespace bg {

constexpr int SRS = 64;                // mesh rows per slab
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;

template <class K>
struct StreamDims {
    static constexpr int R = 4 * K::NB;                          // padded reduced dimension
    static constexpr int SLAB = (SRS + 2) * K::PS;               // doubles of one slab buffer: mesh rows [r0 - 1, r0 + 64]
    static constexpr int CHUNKS = (SLAB * 8 + 1023) / 1024;      // 1-KB LDS DMA pieces per slab
};

struct StreamRunArgs {
    const double* x;        // [N]
    const double* PhiP;     // [NPAD + 2][R]: Phi row i at index i + 1, zero rows around and beyond N, zero columns beyond r
    const double* u0;       // [B][N]
    const double* mu1;      // [B]
    const double* mu2;      // [B]
    double* hist;           // [B][nsteps+1][N]
    int32_t* iters;         // [B][nsteps]
    int32_t* flags;         // [B]
    int32_t* info;          // [B]
    const int32_t* order;   // [B] or null: slot i of the persistent loop works on sample order[i]
    double dt, E, tol;
    int N, NPAD, B, r, nsteps, max_it, supg, nonuniform, force_pivoted;
};

// Local POD (K::local): one basis per time step, picked from the stack by the nearest centre.  PhiP is the stack
// [C][NPAD + 2][R], every block laid out like the POD operand with zero columns beyond its width; r the widest width.
struct LocalStreamRunArgs : StreamRunArgs {
    const int32_t* widths;    // [C], 1 .. r
    const double* UgT;        // [m][N]: U_global[:, :m] transposed
    const double* centres;    // [C][m]
    int32_t* clusters;        // [B][nsteps] or null
    int C, m;
};

struct StreamLds {
    double* slab;           // two slab buffers; later the parked system
    double* u;              // [NMAX + 4]: u at offset 2, zero halo on each side
    double* g; double* h; double* fdt;      // [NMAX]
    double (*cf)[4];        // lo, di, up, R per mesh row or per row of the slab at hand (K::cf_by_mesh_row)
    double* q;              // [R]
    double* m; double* diag; double* y; double* x;      // the solve's own arrays: multipliers of two panels, diagonal, y (and x)
    int* bad;               // guard of each wave (and the info of a pivoted solve)
    double* qg;             // K::local: [64], U_g^T u^n of the current time step
};

// Local POD, the start of a time step (reference :1011-1012), with the arithmetic of rom_fused_kernel<..., LOCAL>
// (rom_fused.hip) written again: called from there, these two functions changed the SGPR spills of every local instantiation
// (and the VGPR count of two), and those kernels are meant to stay what they are.
// local_global_coords: q_g = U_g^T u^n into s_qg[0 .. m) -- wave w of the workgroup's four takes the columns j = w (mod 4),
// lanes stride the rows; s_u2 = u^n at node 0; the caller puts a workgroup barrier behind it.
__device__ __forceinline__ void local_global_coords(const double* UgT, const double* s_u2, int N, int m, int w, int lane, double* s_qg)
{
    for (int j = w; j < m; j += 4) {
        double p = 0.0;
#pragma unroll 4                                 // (loads in flight together: each one is an L2 round trip)
        for (int i = lane; i < N; i += 64) p = __builtin_fma(UgT[(size_t)j * N + i], s_u2[i], p);
        p = wave_sum(p);
        if (lane == 0) s_qg[j] = p;
    }
}

// kmeans.predict (:1012): lane c holds |q_g - centre_c|^2 (summed in j order), then the FIRST index of the minimum over the
// wave (a NaN distance counts as the smallest, as in np.argmin).  Every wave computes it: the cluster is workgroup-uniform
// without a broadcast.  C <= 64.
// KEEP (the offline clustering, kmeans.hip, which labels the training snapshots with this very function so that the same q_g
// gets the same centre there and here): *d_lane receives this lane's distance (+inf beyond C), *d_min the smallest.  The
// time loops call it without, and compile to what they were before the parameter existed.
template <bool KEEP = false>
__device__ __forceinline__ int local_nearest_centre(const double* s_qg, const double* centres, int C, int m, int lane,
                                                    double* d_lane = nullptr, double* d_min = nullptr)
{
    double d = __builtin_inf();
    int ci = lane;
    if (lane < C) {
        d = 0.0;
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const double e = s_qg[j] - centres[(size_t)lane * m + j];
            d = __builtin_fma(e, e, d);
        }
    }
    if constexpr (KEEP) *d_lane = d;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double od = __shfl_xor(d, off);
        const int oc = __shfl_xor(ci, off);
        const bool take = (od != od) ? (d == d || oc < ci) : (od < d || (od == d && oc < ci));
        d = take ? od : d;
        ci = take ? oc : ci;
    }
    if constexpr (KEEP) *d_min = d;
    return __builtin_amdgcn_readfirstlane(ci);
}

template <class K, bool GAL>
struct StreamItems {
    // LSPG: pairs (ca <= cb) of Y, then (Y[ca], X) for br, then (Phi[ca], X) for Phi^T u; Galerkin: (Phi[ca], Y[cb]), then (Phi[ca], X)
    static constexpr int pairs = GAL ? K::NB * K::NB : K::NB * (K::NB + 1) / 2;
    static constexpr int total = pairs + (GAL ? K::NB : 2 * K::NB);
    static constexpr int per_wave = (total + 3) / 4;
};

// The matrix instructions of one 16-row step for wave W: item i of the fixed enumeration belongs to wave i % 4, accumulator i / 4.
template <class K, bool GAL, int W>
__device__ __forceinline__ void stream_step_mfma(const double (&Y)[K::NB], const double (&P)[K::NB], double X,
                                                 double (&acc)[StreamItems<K, GAL>::per_wave])
{
    constexpr int NB = K::NB;
    int i = 0;
    if constexpr (GAL) {
#pragma unroll
        for (int ca = 0; ca < NB; ++ca) {
#pragma unroll
            for (int cb = 0; cb < NB; ++cb, ++i)
                if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(P[ca], Y[cb], acc[i / 4], 0, 0, 0);
        }
#pragma unroll
        for (int ca = 0; ca < NB; ++ca, ++i)
            if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(P[ca], X, acc[i / 4], 0, 0, 0);
    } else {
#pragma unroll
        for (int ca = 0; ca < NB; ++ca) {
#pragma unroll
            for (int cb = ca; cb < NB; ++cb, ++i)
                if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(Y[ca], Y[cb], acc[i / 4], 0, 0, 0);
        }
#pragma unroll
        for (int ca = 0; ca < NB; ++ca, ++i)
            if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(Y[ca], X, acc[i / 4], 0, 0, 0);
#pragma unroll
        for (int ca = 0; ca < NB; ++ca, ++i)
            if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(P[ca], X, acc[i / 4], 0, 0, 0);
    }
}

// Sum the four block partials of wave W's accumulators and park them: S[NB i + ca][NB j + cb] = Ar (LSPG: the pairs cover
// ca <= cb; K::mirror_lspg parks the mirror image too), column R = br, column R + 1 = Phi^T u.
template <class K, bool GAL, int W>
__device__ __forceinline__ void stream_park(const double (&acc)[StreamItems<K, GAL>::per_wave], double* __restrict__ S, int lane)
{
    constexpr int NB = K::NB, R = 4 * NB, SW = K::SW;
    const int oi = lane >> 4, oj = lane & 3;
    const bool writer = ((lane >> 2) & 3) == 3;
    auto put = [&](int i, int row_c, int col_c, int kind) {      // kind 0: block pair, 1: br (column j = 0), 2: Phi^T u (column j = 1)
        if (i % 4 != W) return;
        double v = acc[i / 4];
        v += dpp_mov<0x114>(v);              // row_shr:4
        v += dpp_mov<0x118>(v);              // row_shr:8 -> lanes with blk == 3 hold the sum
        if (kind == 0) {
            if (writer) {
                S[(NB * oi + row_c) * SW + NB * oj + col_c] = v;
                if (K::mirror_lspg && !GAL && row_c != col_c) S[(NB * oj + col_c) * SW + NB * oi + row_c] = v;
            }
        }
        else if (kind == 1) { if (writer && oj == 0) S[(NB * oi + row_c) * SW + R] = v; }
        else { if (writer && oj == 1) S[(NB * oi + row_c) * SW + R + 1] = v; }
    };
    int i = 0;
    if constexpr (GAL) {
#pragma unroll
        for (int ca = 0; ca < NB; ++ca)
#pragma unroll
            for (int cb = 0; cb < NB; ++cb, ++i) put(i, ca, cb, 0);
#pragma unroll
        for (int ca = 0; ca < NB; ++ca, ++i) { put(i, ca, 0, 1); put(i, ca, 0, 2); }
    } else {
#pragma unroll
        for (int ca = 0; ca < NB; ++ca)
#pragma unroll
            for (int cb = ca; cb < NB; ++cb, ++i) put(i, ca, cb, 0);
#pragma unroll
        for (int ca = 0; ca < NB; ++ca, ++i) put(i, ca, 0, 1);
#pragma unroll
        for (int ca = 0; ca < NB; ++ca, ++i) put(i, ca, 0, 2);
    }
}

// The two row routines of a slab, for this loop and for the hyper-reduced one (rom_hyper.hip), which keeps the three stencil
// rows of a sampled row side by side: `rows` is the first of three LDS rows PS doubles apart (basis rows i - 1, i, i + 1),
// already at this lane's columns NB t .. NB t + NB - 1.
// The lift u_{i-1}, u_i, u_{i+1} = Phi q of one row by its four lanes: qs = this lane's slice of q (s_q + NB t).  After the
// two quad sums every lane of the quad holds the three values.
template <int NB, int PS>
__device__ __forceinline__ void stream_lift_rows(const double* rows, const double* qs, double& um, double& u0, double& ur)
{
    double sm = 0.0, s0 = 0.0, sr = 0.0;
#pragma unroll
    for (int c2 = 0; c2 < NB / 2; ++c2) {
        const double2 qv = *reinterpret_cast<const double2*>(qs + 2 * c2);
        const double2 pm = *reinterpret_cast<const double2*>(rows + 2 * c2);
        const double2 p0 = *reinterpret_cast<const double2*>(rows + PS + 2 * c2);
        const double2 pr = *reinterpret_cast<const double2*>(rows + 2 * PS + 2 * c2);
        sm = __builtin_fma(pm.x, qv.x, sm); sm = __builtin_fma(pm.y, qv.y, sm);
        s0 = __builtin_fma(p0.x, qv.x, s0); s0 = __builtin_fma(p0.y, qv.y, s0);
        sr = __builtin_fma(pr.x, qv.x, sr); sr = __builtin_fma(pr.y, qv.y, sr);
    }
    sm += dpp_mov<0xB1>(sm); sm += dpp_mov<0x4E>(sm);
    s0 += dpp_mov<0xB1>(s0); s0 += dpp_mov<0x4E>(s0);
    sr += dpp_mov<0xB1>(sr); sr += dpp_mov<0x4E>(sr);
    um = sm; u0 = s0; ur = sr;
}

// The operands of one row of a 16-row step: Y = lo Phi[i-1] + di Phi[i] + up Phi[i+1] (c01 = lo, di; c23 = up, R) and
// P = Phi[i], this lane's NB columns of each.
template <int NB, int PS>
__device__ __forceinline__ void stream_row_operands(const double* rows, double2 c01, double2 c23, double (&Y)[NB], double (&P)[NB])
{
#pragma unroll
    for (int c2 = 0; c2 < NB / 2; ++c2) {
        const double2 tb = *reinterpret_cast<const double2*>(rows + 2 * c2);
        const double2 tm = *reinterpret_cast<const double2*>(rows + PS + 2 * c2);
        const double2 ta = *reinterpret_cast<const double2*>(rows + 2 * PS + 2 * c2);
        P[2 * c2] = tm.x; P[2 * c2 + 1] = tm.y;
        Y[2 * c2] = __builtin_fma(c23.x, ta.x, __builtin_fma(c01.y, tm.x, c01.x * tb.x));
        Y[2 * c2 + 1] = __builtin_fma(c23.x, ta.y, __builtin_fma(c01.y, tm.y, c01.x * tb.y));
    }
}

// The body of the kernel for wave W of the workgroup.  The wave number is a template parameter of the WHOLE body (the kernel
// branches once, at its top): every wave runs its own quarter of the block pairs with accumulators that never change
// registers.  A `switch (w)` around the matrix instructions of each row step instead cost 340 accumulator moves per
// 87 instructions (first version of the wide kernel: 6.5e5 sample-steps/s).  All four copies execute the same sequence of barriers.
template <class K, bool GAL, bool PIV, int W>
__device__ __forceinline__ void rom_stream_body(const typename K::Args& a, const StreamLds& L)
{
    static_assert(!PIV || K::has_repair, "this kernel has no repair instantiation");
    constexpr int NB = K::NB, R = 4 * NB, PS = K::PS, NMAX = K::NMAX, SLAB = StreamDims<K>::SLAB, CHUNKS = StreamDims<K>::CHUNKS;
    constexpr int NACC = StreamItems<K, GAL>::per_wave;
    constexpr int w = W;
    double* const s_slab = L.slab;
    double* const s_u = L.u;
    double* const s_g = L.g;
    double* const s_h = L.h;
    double* const s_fdt = L.fdt;
    double (*const s_cf)[4] = L.cf;
    double* const s_q = L.q;
    double* const S = s_slab;                                    // [R][K::SW]: Ar | br | Phi^T u (over the dead slabs)

    const int tid = threadIdx.x;
    const int N = a.N;
    const double h = (a.x[N - 1] - a.x[0]) / (double)(N - 1);
    const int nslab = (N + SRS - 1) / SRS;       // (= a.NPAD / 64; read from the arguments it cost the Galerkin wide kernel 400 B of scratch)
    if (tid < 4) s_u[tid < 2 ? tid : NMAX + tid] = 0.0;

    for (int slot = blockIdx.x; slot < a.B; slot += gridDim.x) {
        const int smp = a.order ? a.order[slot] : slot;
        if (smp < 0 || smp >= a.B) continue;                     // workgroup-uniform
        if (PIV && !a.force_pivoted && a.info[smp] != BG_INFO_NEEDS_PIVOTING) continue;      // workgroup-uniform
        const double mu1 = a.mu1[smp], mu2 = a.mu2[smp];
        double* hist = a.hist + (size_t)smp * (size_t)(a.nsteps + 1) * (size_t)N;
        __syncthreads();
        // ---- per-sample constants (compute_forcing_vector :427-461, f_gp of :556-558) and the initial state ------------
        for (int i = tid; i < NMAX; i += 256) {
            double frPrev = 0.0, fl = 0.0, hf = 0.0, u = 0.0;
            if (i < N) {
                rom_nodal_forcing(a.x, i, N, mu2, h, a.nonuniform, frPrev, fl, hf);
                u = a.u0[(size_t)smp * N + i];
                hist[i] = u;
            }
            s_fdt[i] = a.dt * (frPrev + fl);
            s_h[i] = hf;
            s_u[i + 2] = u;
        }
        if (tid < R) s_q[tid] = 0.0;
        __syncthreads();

        int flags = 0, info_out = 0;
        bool aborted = false;
        PhaseClock<kPhaseClock && W == 0, 6> clk;                // diagnostic builds (tools/time_wide_rom.py --phases); thread 0 stores
        // K::local: the step's basis and width are the picked cluster's (wave-uniform: the DMA source base stays in scalar
        // registers); otherwise the arguments are read where they are used, as before there was a pick
        const double* PhiL = nullptr;
        int r_local = 0;
        auto step_basis = [&]() -> const double* { if constexpr (K::local) return PhiL; else return a.PhiP; };
        auto step_width = [&]() -> int { if constexpr (K::local) return r_local; else return a.r; };
        // LDS DMA of slab `slab` (mesh rows [r0 - 1, r0 + 64] = rows r0 .. r0 + 65 of PhiP) into buffer `buf`: wave w moves the
        // 1-KB pieces w, w + 4, ...; a lane's 16 bytes land at piece base + 16 lane, i.e. LDS row o / (8 PS), byte o % (8 PS) of it
        // (the 16 bytes of row padding are filled from a valid dummy address)
        auto slab_dma = [&](int slab, int buf) {
            const char* src = reinterpret_cast<const char*>(step_basis() + (size_t)slab * SRS * R);
            const int ln = tid & 63;
            for (int j = w; j < CHUNKS; j += 4) {
                const int o = 1024 * j + 16 * ln;
                const int row = o / (PS * 8), within = o - row * (PS * 8);
                const char* g = src + (within < R * 8 ? row * (R * 8) + within : 0);
                if (row < SRS + 2)                           // lanes beyond the slab's last row write nothing (the next buffer starts there)
                    __builtin_amdgcn_global_load_lds((gbl_void_t*)g, (lds_void_t*)(reinterpret_cast<char*>(s_slab + buf * SLAB) + 1024 * j), 16, 0, 0);
            }
        };

        for (int step = 0; step < a.nsteps && info_out == 0 && !aborted; ++step) {
            // ---- g = M u^n + dt F (`M @ U[:, n] + At*F`, :746) -----------------------------------------------------------
            for (int i = tid; i < NMAX; i += 256) {
                double g = 0.0;
                if (i < N) g = rom_mass_rhs_node(a.x, i, N, s_u[i + 1], s_u[i + 2], s_u[i + 3], s_fdt[i], h, a.nonuniform);
                s_g[i] = g;
            }
            if constexpr (K::local)                            // q_g = U_g^T u^n (:1011); s_u is not written before the barrier
                local_global_coords(a.UgT, s_u + 2, N, a.m, w, tid & 63, L.qg);
            __syncthreads();
            if constexpr (K::local) {
                // kmeans.predict (:1012), (:1013): the nearest centre's block of the stack and its width serve this step.  No
                // DMA is in flight here, and the streaming sweep re-reads the basis on every pass: a switch costs nothing more.
                const int cl = local_nearest_centre(L.qg, a.centres, a.C, a.m, tid & 63);
                PhiL = a.PhiP + (size_t)cl * (size_t)(a.NPAD + 2) * R;
                r_local = a.widths[cl] < a.r ? a.widths[cl] : a.r;      // (clamped: the blocks are R wide, a.r <= R)
                if (tid == 0 && a.clusters) a.clusters[(size_t)smp * a.nsteps + step] = cl;
            }
            int k = 0;
            bool proj = true;
            while (true) {
                // per-lane indices from an opaque copy of the thread index: their address arithmetic is recomputed per pass
                // instead of being hoisted out of the time loop and spilled (see rom_fused.hip)
                int tid_i = tid;
                asm volatile("" : "+v"(tid_i));
                const int lane = tid_i & 63, pk = lane >> 4, pblk = (lane >> 2) & 3, pt = lane & 3;
                const bool lift = k > 0;                 // iteration 0 of a step assembles at u^n, which s_u holds (:725)
                double acc[NACC];
#pragma unroll
                for (int p = 0; p < NACC; ++p) acc[p] = 0.0;
                clk.pass();
                clk.lap(5);
                slab_dma(0, 0);                                // (not across the pass boundary: the parked system lies over both buffers)
                for (int slab = 0; slab < nslab; ++slab) {
                    const int r0 = slab * SRS, cur = slab & 1;
                    const int cf0 = K::cf_by_mesh_row ? r0 : 0;               // the row of s_cf of this slab's first mesh row
                    const double* s_P = s_slab + cur * SLAB;                  // local row l = mesh row r0 - 1 + l
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's DMA pieces of the slab have landed
                    __syncthreads();                                          // ... and everybody's; the other buffer (and a per-slab s_cf) is no longer read
                    clk.lap(0);
                    if (slab + 1 < nslab) slab_dma(slab + 1, cur ^ 1);        // the next slab lands while this one is worked on
                    // ---- four lanes per row i = r0 + q4: u_{i-1}, u_i, u_{i+1} = Phi q (:773), then A(u), R(u) of row i --------------
                    {
                        const int q4 = tid_i >> 2, i = r0 + q4;
                        double um, u0, ur;
                        if (lift) {
                            stream_lift_rows<NB, PS>(s_P + q4 * PS + NB * pt, s_q + NB * pt, um, u0, ur);      // rows outside the mesh are zero rows of PhiP
                            if (pt == 0) s_u[i + 2] = u0;
                        } else {
                            um = s_u[i + 1]; u0 = s_u[i + 2]; ur = s_u[i + 3];
                        }
                        if (proj && pt == 0) {
                            const bool in = i < N;
                            const MeshConst mc = make_mesh_const(h, a.dt, a.E, a.supg);
                            double lo, di, up, R_i;
                            rom_assemble_row(i, N, um, u0, (i + 1 < N) ? ur : 0.0, in ? s_g[i] : 0.0,
                                             (in && i > 0) ? s_h[i - 1] : 0.0, (in && i < N - 1) ? s_h[i] : 0.0, mu1, mc,
                                             a.nonuniform, a.x, a.dt, a.E, lo, di, up, R_i);
                            *reinterpret_cast<double2*>(&s_cf[cf0 + q4][0]) = make_double2(lo, di);
                            *reinterpret_cast<double2*>(&s_cf[cf0 + q4][2]) = make_double2(up, R_i);
                        }
                    }
                    clk.lap(1);
                    if (proj) {
                        __syncthreads();                                      // the slab's coefficients (and u) are in LDS
                        // ---- projection: four steps of 16 rows; lane (k, blk, t): row 16 st + 4 k + blk, columns NB t + c ------------
#pragma unroll 1
                        for (int st = 0; st < SRS / 16; ++st) {
                            const int rl = 16 * st + 4 * pk + pblk;
                            const double2 c01 = *reinterpret_cast<const double2*>(&s_cf[cf0 + rl][0]);
                            const double2 c23 = *reinterpret_cast<const double2*>(&s_cf[cf0 + rl][2]);
                            double Y[NB], P[NB];                                  // from the row below (local row rl = mesh row r0 - 1 + rl) on
                            stream_row_operands<NB, PS>(s_P + rl * PS + NB * pt, c01, c23, Y, P);
                            const double ui = s_u[r0 + rl + 2];
                            const double X = (pt == 0) ? c23.y : ((pt == 1) ? ui : 0.0);      // extra B block [R, u, 0, 0]
                            stream_step_mfma<K, GAL, W>(Y, P, X, acc);
                        }
                    }
                    clk.lap(2);
                }
                __syncthreads();                               // the last slab's rows are no longer read (the system is parked over them)
                if (!proj) break;                              // that was the lift for U[:, n+1] = Phi q (:779)
                // ---- park the reduced system (over the dead slabs) ---------------------------------------------------------------
                stream_park<K, GAL, W>(acc, S, lane);
                __syncthreads();
                clk.lap(3);
                // ---- solve(Ar, -br) (:767), q = Phi^T u_k + dq, err = |dq| / |q|  (:770-776) -------------------------------------
                double nd, nq;
                K::template solve_update<GAL, PIV, W>(a, L, step_width(), lane, aborted, info_out, nd, nq, [&] { clk.lap(4); });
                nd = sqrt(nd); nq = sqrt(nq);
                const double err = nd / nq;
                ++k;
                const bool more = (err > a.tol) && (k < a.max_it) && info_out == 0 && !aborted;
                if (!(err - err == 0.0)) flags |= BG_FLAG_NONFINITE;
                if (k >= a.max_it) flags |= BG_FLAG_HIT_CAP;
                __syncthreads();
                if (aborted) break;
                proj = more;                                   // after the last iteration: one lift-only sweep
            }
            // ---- U[:, n+1] = U1 (:779): one coalesced row ---------------------------------------------------------------------
            double* hrow = hist + (size_t)(step + 1) * N;
            for (int i = tid; i < N; i += 256) hrow[i] = s_u[i + 2];
            if (tid == 0) a.iters[(size_t)smp * a.nsteps + step] = k;
        }
        if (tid == 0) {
            a.flags[smp] = flags;
            a.info[smp] = aborted ? BG_INFO_NEEDS_PIVOTING : info_out;
            clk.store(a.iters + (size_t)smp * a.nsteps, a.nsteps);
        }
    }
}

// The four-way branch on the wave at the top of a kernel.
template <class K, bool GAL, bool PIV>
__device__ __forceinline__ void rom_stream_waves(const typename K::Args& a, const StreamLds& L)
{
    switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {       // wave-uniform by construction
        case 0: rom_stream_body<K, GAL, PIV, 0>(a, L); break;
        case 1: rom_stream_body<K, GAL, PIV, 1>(a, L); break;
        case 2: rom_stream_body<K, GAL, PIV, 2>(a, L); break;
        default: rom_stream_body<K, GAL, PIV, 3>(a, L); break;
    }
}

// The argument checks of an entry point (mesh sizes n_min .. n_max, bases of up to r_max modes) and the kernel's arguments.
// BG_OK with B == 0 means there is nothing to launch.
inline int stream_run_args(StreamRunArgs& a, int n_min, int n_max, int r_max, int N, int B, int r, int nsteps, int projection,
                           const double* x, const double* PhiP, const double* u0, const double* mu1, const double* mu2, double dt,
                           double E, double tol, int max_it, int options, double* hist, int32_t* iters, int32_t* flags,
                           int32_t* info, const int32_t* order)
{
    if (N < n_min || B < 0 || r < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > n_max) return BG_ERR_UNSUPPORTED_N;
    if (r > r_max) return BG_ERR_UNSUPPORTED_R;
    if (B == 0) return BG_OK;
    if (!x || !PhiP || !u0 || !mu1 || !mu2 || !hist || !flags || !info || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    if ((uintptr_t)PhiP & 15) return BG_ERR_BAD_ARG;
    a.x = x; a.PhiP = PhiP; a.u0 = u0; a.mu1 = mu1; a.mu2 = mu2; a.hist = hist; a.iters = iters; a.flags = flags; a.info = info; a.order = order;
    a.dt = dt; a.E = E; a.tol = tol; a.N = N; a.NPAD = ((N + SRS - 1) / SRS) * SRS; a.B = B; a.r = r; a.nsteps = nsteps; a.max_it = max_it;
    a.supg = options & BG_OPT_SUPG; a.nonuniform = (options & BG_OPT_NONUNIFORM) ? 1 : 0;
    a.force_pivoted = (options & BG_OPT_FORCE_PIVOTED) ? 1 : 0;
    return BG_OK;
}

}  // namespace bg
