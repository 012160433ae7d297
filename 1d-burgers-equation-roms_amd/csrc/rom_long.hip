// rom_long.hip -- the whole POD-PROM time loop of one sample on one compute unit for LONG meshes, 513 <= N <= 1024, with
// bases of up to 40 modes (bg_rom_run_long).  reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785.
//
// bg_rom_run (rom_fused.hip) keeps the basis in registers, 2 (N / 64) (r / 4) of them per lane: 160 at N = 512, 320 at
// N = 1024.  Here the basis streams through LDS as in rom_wide.hip -- 64 mesh rows at a time, double buffered, by LDS DMA
// from the padded copy PhiP [NPAD + 2][40] (one pass over it per Picard iteration, L2-resident: 328 KB at N = 1024) -- and
// what stays in registers are the accumulators of the reduced system: its 4 x 4 block pairs are dealt round-robin to the
// four waves (Galerkin 110 items: 28 per wave; LSPG 75: 19 per wave), every wave sweeps ALL mesh rows for its own pairs,
// so no per-wave partial systems are added up.  Per slab:
//   four lanes per row lift u = Phi q for rows i - 1, i, i + 1 (:773; iterations after the first) and assemble A(u), R(u)
//   of row i (:730-753, rom_assemble_row)  ->  each wave forms the rows of Y = A Phi it multiplies from the slab and the
//   slab's coefficients in LDS (lane (k, blk, t): mesh row 4 k + blk of the 16-row step, columns 10 t + c for block c:
//   five 16-byte reads per row)  ->  v_mfma_f64_4x4x4_4b.  Two workgroup barriers per slab.
// The reduced system is parked WHOLE in LDS over the dead slabs (LSPG: the lower block pairs mirrored on the way) and
// solved by rom_fused_device.hpp's routines: the guarded pivot-free Gauss-Jordan of all four waves in the fast kernel; a
// sample in which a multiplier below the diagonal exceeds 1 or a pivot is 0 (np.linalg.solve would have exchanged rows)
// is marked and redone from u0 by the repair instantiation (PIV: one-wave partial pivoting) launched behind the fast one,
// as in bg_rom_run.  Then q = Phi^T u + dq, the stopping test, and after the last iteration one lift-only sweep for
// U[:, n+1] = Phi q (:779).
// LDS: 8 B per mesh row for each of u, g, h_f, dt F (32 KB at 1024 rows), the coefficients of ONE slab (2 KB), two slabs
// of 66 x 42 doubles (43.3 KB) -- 77.7 KB, so two workgroups share a compute unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "rom_fused_device.hpp"

namespace {

using namespace bg;

constexpr int LNMAX = 1024;            // mesh rows
constexpr int LR = 40;                 // padded reduced dimension: column 10 t + c  <->  (lane index t, block c)
constexpr int LNB = 10;                // 4-column blocks
constexpr int LRS = 64;                // mesh rows per slab
constexpr int LPS = 42;                // doubles per row of the LDS slabs (16-byte aligned rows)
constexpr int LSW = LR + 4;            // doubles per row of the parked system: Ar | br | Phi^T u
constexpr int LSLAB = (LRS + 2) * LPS;                       // doubles of one slab buffer: mesh rows [r0 - 1, r0 + 64]
constexpr int LCHUNKS = (LSLAB * 8 + 1023) / 1024;           // 1-KB LDS DMA pieces per slab (22)
#ifndef BG_LONG_WG_PER_CU
#define BG_LONG_WG_PER_CU 2
#endif
constexpr int LWG_PER_CU = BG_LONG_WG_PER_CU;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;

struct LongRunArgs {
    const double* x;        // [N]
    const double* PhiP;     // [NPAD + 2][40]: Phi row i at index i + 1, zero rows around and beyond N, zero columns beyond r
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

template <bool GAL>
struct LongItems {
    // LSPG: pairs (ca <= cb) of Y, then (Y[ca], X) for br, then (Phi[ca], X) for Phi^T u; Galerkin: (Phi[ca], Y[cb]), then (Phi[ca], X)
    static constexpr int pairs = GAL ? LNB * LNB : LNB * (LNB + 1) / 2;
    static constexpr int total = pairs + (GAL ? LNB : 2 * LNB);
    static constexpr int per_wave = (total + 3) / 4;
};

// The matrix instructions of one 16-row step for wave W: item i of the fixed enumeration belongs to wave i % 4, accumulator i / 4.
template <bool GAL, int W>
__device__ __forceinline__ void long_step_mfma(const double (&Y)[LNB], const double (&P)[LNB], double X, double (&acc)[LongItems<GAL>::per_wave])
{
    int i = 0;
    if constexpr (GAL) {
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca) {
#pragma unroll
            for (int cb = 0; cb < LNB; ++cb, ++i)
                if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(P[ca], Y[cb], acc[i / 4], 0, 0, 0);
        }
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca, ++i)
            if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(P[ca], X, acc[i / 4], 0, 0, 0);
    } else {
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca) {
#pragma unroll
            for (int cb = ca; cb < LNB; ++cb, ++i)
                if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(Y[ca], Y[cb], acc[i / 4], 0, 0, 0);
        }
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca, ++i)
            if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(Y[ca], X, acc[i / 4], 0, 0, 0);
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca, ++i)
            if (i % 4 == W) acc[i / 4] = __builtin_amdgcn_mfma_f64_4x4x4f64(P[ca], X, acc[i / 4], 0, 0, 0);
    }
}

// Sum the four block partials of wave W's accumulators and park them: S[10 i + ca][10 j + cb] = Ar (LSPG: and its mirror
// image, the pairs cover ca <= cb), column 40 = br, column 41 = Phi^T u.
template <bool GAL, int W>
__device__ __forceinline__ void long_park(const double (&acc)[LongItems<GAL>::per_wave], double* __restrict__ S, int lane)
{
    const int oi = lane >> 4, oj = lane & 3;
    const bool writer = ((lane >> 2) & 3) == 3;
    auto put = [&](int i, int row_c, int col_c, int kind) {      // kind 0: block pair, 1: br (column j = 0), 2: Phi^T u (column j = 1)
        if (i % 4 != W) return;
        double v = acc[i / 4];
        v += dpp_mov<0x114>(v);              // row_shr:4
        v += dpp_mov<0x118>(v);              // row_shr:8 -> lanes with blk == 3 hold the sum
        if (kind == 0) {
            if (writer) {
                S[(LNB * oi + row_c) * LSW + LNB * oj + col_c] = v;
                if (!GAL && row_c != col_c) S[(LNB * oj + col_c) * LSW + LNB * oi + row_c] = v;
            }
        }
        else if (kind == 1) { if (writer && oj == 0) S[(LNB * oi + row_c) * LSW + LR] = v; }
        else { if (writer && oj == 1) S[(LNB * oi + row_c) * LSW + LR + 1] = v; }
    };
    int i = 0;
    if constexpr (GAL) {
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca)
#pragma unroll
            for (int cb = 0; cb < LNB; ++cb, ++i) put(i, ca, cb, 0);
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca, ++i) { put(i, ca, 0, 1); put(i, ca, 0, 2); }
    } else {
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca)
#pragma unroll
            for (int cb = ca; cb < LNB; ++cb, ++i) put(i, ca, cb, 0);
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca, ++i) put(i, ca, 0, 1);
#pragma unroll
        for (int ca = 0; ca < LNB; ++ca, ++i) put(i, ca, 0, 2);
    }
}

struct LongLdsPtrs {
    double* slab;           // two slab buffers; during the solve the parked system and the solve's own arrays
    double* u;              // [LNMAX + 4]
    double* g; double* h; double* fdt;      // [LNMAX]
    double (*cf)[4];        // [LRS][4]: lo, di, up, R of the rows of the slab at hand
    double* q;              // [LR]
    int* bad;               // [4] guard of each wave, [4] info of the pivoted solve
};

// The body of the kernel for wave W of the workgroup.  As in rom_wide.hip the wave number is a template parameter of the
// WHOLE body (the kernel branches once, at its top), so that every wave's accumulators never change registers.  All four
// copies execute the same sequence of barriers.
template <bool GAL, bool PIV, int W>
__device__ __forceinline__ void rom_long_body(const LongRunArgs& a, const LongLdsPtrs& L)
{
    constexpr int NACC = LongItems<GAL>::per_wave;
    constexpr int w = W;
    double* const s_slab = L.slab;
    double* const s_u = L.u;
    double* const s_g = L.g;
    double* const s_h = L.h;
    double* const s_fdt = L.fdt;
    double (*const s_cf)[4] = L.cf;
    double* const s_q = L.q;
    int* const s_bad = L.bad;
    // over the dead slabs: the system [LR][LSW], then the multipliers of two panels, the diagonal, y and x
    double* const S = s_slab;
    double (*const s_m)[4][64] = reinterpret_cast<double (*)[4][64]>(s_slab + LR * LSW);
    double* const s_diag = s_slab + LR * LSW + 512;
    double* const s_y = s_diag + 64;
    double* const s_x = s_y + 64;
    static_assert(LR * LSW + 512 + 3 * 64 <= 2 * LSLAB, "the solve's arrays fit over the slabs");

    const int tid = threadIdx.x;
    const int N = a.N, r = a.r;
    const double h = (a.x[N - 1] - a.x[0]) / (double)(N - 1);
    const int nslab = a.NPAD / LRS;
    if (tid < 4) s_u[tid < 2 ? tid : LNMAX + tid] = 0.0;

    for (int slot = blockIdx.x; slot < a.B; slot += gridDim.x) {
        const int smp = a.order ? a.order[slot] : slot;
        if (smp < 0 || smp >= a.B) continue;                     // workgroup-uniform
        if (PIV && !a.force_pivoted && a.info[smp] != BG_INFO_NEEDS_PIVOTING) continue;      // workgroup-uniform
        const double mu1 = a.mu1[smp], mu2 = a.mu2[smp];
        double* hist = a.hist + (size_t)smp * (size_t)(a.nsteps + 1) * (size_t)N;
        __syncthreads();
        // ---- per-sample constants (compute_forcing_vector :427-461, f_gp of :556-558) and the initial state ------------
        for (int i = tid; i < LNMAX; i += 256) {
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
        if (tid < LR) s_q[tid] = 0.0;
        __syncthreads();

        int flags = 0, info_out = 0;
        bool aborted = false;
        // LDS DMA of slab `slab` (mesh rows [r0 - 1, r0 + 64] = rows r0 .. r0 + 65 of PhiP) into buffer `buf`: wave w moves the
        // 1-KB pieces w, w + 4, ...; a lane's 16 bytes land at piece base + 16 lane, i.e. LDS row o / 336, byte o % 336 of it
        // (the 16 bytes of row padding are filled from a valid dummy address)
        auto slab_dma = [&](int slab, int buf) {
            const char* src = reinterpret_cast<const char*>(a.PhiP + (size_t)slab * LRS * LR);
            const int ln = tid & 63;
            for (int j = w; j < LCHUNKS; j += 4) {
                const int o = 1024 * j + 16 * ln;
                const int row = o / (LPS * 8), within = o - row * (LPS * 8);
                const char* g = src + (within < LR * 8 ? row * (LR * 8) + within : 0);
                if (row < LRS + 2)                           // lanes beyond the slab's last row write nothing (the next buffer starts there)
                    __builtin_amdgcn_global_load_lds((gbl_void_t*)g, (lds_void_t*)(reinterpret_cast<char*>(s_slab + buf * LSLAB) + 1024 * j), 16, 0, 0);
            }
        };

        for (int step = 0; step < a.nsteps && info_out == 0 && !aborted; ++step) {
            // ---- g = M u^n + dt F (`M @ U[:, n] + At*F`, :746) -----------------------------------------------------------
            for (int i = tid; i < LNMAX; i += 256) {
                double g = 0.0;
                if (i < N) {
                    const double um = s_u[i + 1], u0 = s_u[i + 2], ur = s_u[i + 3];
                    if (a.nonuniform) {
                        double v = 0.0;
                        if (i > 0) v = (a.x[i] - a.x[i - 1]) / 6.0 * __builtin_fma(2.0, u0, um);
                        if (i < N - 1) v = __builtin_fma((a.x[i + 1] - a.x[i]) / 6.0, __builtin_fma(2.0, u0, ur), v);
                        g = v + s_fdt[i];
                    } else {
                        double acc;
                        if (i == 0) acc = __builtin_fma(2.0, u0, ur);
                        else if (i == N - 1) acc = __builtin_fma(2.0, u0, um);
                        else acc = __builtin_fma(4.0, u0, um) + ur;
                        g = __builtin_fma(h / 6.0, acc, s_fdt[i]);
                    }
                }
                s_g[i] = g;
            }
            __syncthreads();
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
                slab_dma(0, 0);                                // (not across the pass boundary: the parked system lies over the buffers)
                for (int slab = 0; slab < nslab; ++slab) {
                    const int r0 = slab * LRS, cur = slab & 1;
                    const double* s_P = s_slab + cur * LSLAB;                 // local row l = mesh row r0 - 1 + l
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's DMA pieces of the slab have landed
                    __syncthreads();                                          // ... and everybody's; the other buffer and s_cf are no longer read
                    if (slab + 1 < nslab) slab_dma(slab + 1, cur ^ 1);        // the next slab lands while this one is worked on
                    // ---- four lanes per row i = r0 + q4: u_{i-1}, u_i, u_{i+1} = Phi q (:773), then A(u), R(u) of row i --------------
                    {
                        const int q4 = tid_i >> 2, i = r0 + q4;
                        double um, u0, ur;
                        if (lift) {
                            const double* prow = s_P + q4 * LPS + LNB * pt;
                            double sm = 0.0, s0 = 0.0, sr = 0.0;
#pragma unroll
                            for (int c2 = 0; c2 < LNB / 2; ++c2) {
                                const double2 qv = *reinterpret_cast<const double2*>(&s_q[LNB * pt + 2 * c2]);
                                const double2 pm = *reinterpret_cast<const double2*>(prow + 2 * c2);
                                const double2 p0 = *reinterpret_cast<const double2*>(prow + LPS + 2 * c2);
                                const double2 pr = *reinterpret_cast<const double2*>(prow + 2 * LPS + 2 * c2);
                                sm = __builtin_fma(pm.x, qv.x, sm); sm = __builtin_fma(pm.y, qv.y, sm);
                                s0 = __builtin_fma(p0.x, qv.x, s0); s0 = __builtin_fma(p0.y, qv.y, s0);
                                sr = __builtin_fma(pr.x, qv.x, sr); sr = __builtin_fma(pr.y, qv.y, sr);
                            }
                            sm += dpp_mov<0xB1>(sm); sm += dpp_mov<0x4E>(sm);          // quad sums: every lane of the quad holds the three values
                            s0 += dpp_mov<0xB1>(s0); s0 += dpp_mov<0x4E>(s0);
                            sr += dpp_mov<0xB1>(sr); sr += dpp_mov<0x4E>(sr);
                            um = sm; u0 = s0; ur = sr;                                 // rows outside the mesh are zero rows of PhiP
                            if (pt == 0) s_u[i + 2] = u0;
                        } else {
                            um = s_u[i + 1]; u0 = s_u[i + 2]; ur = s_u[i + 3];
                        }
                        if (proj && pt == 0) {
                            const bool in = i < N;
                            const MeshConst mc = make_mesh_const(h, a.dt, a.E, a.supg);
                            double lo, di, up, R;
                            rom_assemble_row(i, N, um, u0, (i + 1 < N) ? ur : 0.0, in ? s_g[i] : 0.0,
                                             (in && i > 0) ? s_h[i - 1] : 0.0, (in && i < N - 1) ? s_h[i] : 0.0, mu1, mc,
                                             a.nonuniform, a.x, a.dt, a.E, lo, di, up, R);
                            *reinterpret_cast<double2*>(&s_cf[q4][0]) = make_double2(lo, di);
                            *reinterpret_cast<double2*>(&s_cf[q4][2]) = make_double2(up, R);
                        }
                    }
                    if (proj) {
                        __syncthreads();                                      // the slab's coefficients (and u) are in LDS
                        // ---- projection: four steps of 16 rows; lane (k, blk, t): row 16 st + 4 k + blk, columns 10 t + c -------------
#pragma unroll 1
                        for (int st = 0; st < LRS / 16; ++st) {
                            const int rl = 16 * st + 4 * pk + pblk;
                            const double2 c01 = *reinterpret_cast<const double2*>(&s_cf[rl][0]);
                            const double2 c23 = *reinterpret_cast<const double2*>(&s_cf[rl][2]);
                            const double* pb = s_P + rl * LPS + LNB * pt;         // the row below (local row rl = mesh row r0 - 1 + rl)
                            double Y[LNB], P[LNB];
#pragma unroll
                            for (int c2 = 0; c2 < LNB / 2; ++c2) {
                                const double2 tb = *reinterpret_cast<const double2*>(pb + 2 * c2);
                                const double2 tm = *reinterpret_cast<const double2*>(pb + LPS + 2 * c2);
                                const double2 ta = *reinterpret_cast<const double2*>(pb + 2 * LPS + 2 * c2);
                                P[2 * c2] = tm.x; P[2 * c2 + 1] = tm.y;
                                Y[2 * c2] = __builtin_fma(c23.x, ta.x, __builtin_fma(c01.y, tm.x, c01.x * tb.x));
                                Y[2 * c2 + 1] = __builtin_fma(c23.x, ta.y, __builtin_fma(c01.y, tm.y, c01.x * tb.y));
                            }
                            const double ui = s_u[r0 + rl + 2];
                            const double X = (pt == 0) ? c23.y : ((pt == 1) ? ui : 0.0);      // extra B block [R, u, 0, 0]
                            long_step_mfma<GAL, W>(Y, P, X, acc);
                        }
                    }
                }
                __syncthreads();                               // the last slab's rows are no longer read (the system is parked over them)
                if (!proj) break;                              // that was the lift for U[:, n+1] = Phi q (:779)
                // ---- park the reduced system (over the dead slabs) ---------------------------------------------------------------
                long_park<GAL, W>(acc, S, lane);
                __syncthreads();
                // ---- solve(Ar, -br) (:767) ----------------------------------------------------------------------------------------
                const double wtu = (lane < r) ? S[lane * LSW + LR + 1] : 0.0;            // Phi^T u
                auto entry = [&](int i, int j) -> double { return S[i * LSW + j]; };      // (Ar | br)[i][j]
                double xout;
                if constexpr (PIV) {
                    if (w == 0) fused::pivoted_solve_of<LNB>(entry, s_x, &s_bad[4], lane, r);
                    __syncthreads();
                    xout = (lane < LR) ? s_x[lane] : 0.0;
                    if (s_bad[4] != 0 && info_out == 0) info_out = s_bad[4];
                } else {
                    bool tripped;
                    xout = fused::coop_gj_solve_of<LNB>(entry, s_m, s_diag, s_y, s_bad, w, lane, r, tripped);
                    if (tripped) aborted = true;
                }
                // ---- q = Phi^T u_k + dq, err = |dq| / |q|  (:770-776) -----------------------------------------------------------
                const double dq = (lane < r) ? xout : 0.0;
                const double qn = wtu + dq;
                double nd, nq;
                wave_sum2(dq * dq, qn * qn, nd, nq);
                nd = sqrt(nd); nq = sqrt(nq);
                const double err = nd / nq;
                ++k;
                const bool more = (err > a.tol) && (k < a.max_it) && info_out == 0 && !aborted;
                if (!(err - err == 0.0)) flags |= BG_FLAG_NONFINITE;
                if (k >= a.max_it) flags |= BG_FLAG_HIT_CAP;
                if (w == 0 && lane < LR) s_q[lane] = qn;
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
        }
    }
}

// The repair kernel (PIV) keeps one workgroup per CU: its one-wave pivoted solve holds a 41-double row per lane.
template <bool GAL, bool PIV>
__global__ __launch_bounds__(256, PIV ? 1 : LWG_PER_CU) void rom_long_kernel(LongRunArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_slab[2 * LSLAB];             // two slab buffers; later the system
    __shared__ __attribute__((aligned(16))) double s_u[LNMAX + 4];                // u at offset 2, zero halo on each side
    __shared__ double s_g[LNMAX], s_h[LNMAX], s_fdt[LNMAX];
    __shared__ __attribute__((aligned(16))) double s_cf[LRS][4];                  // lo, di, up, R per row of the slab
    __shared__ __attribute__((aligned(16))) double s_q[LR];
    __shared__ int s_bad[8];
    static_assert(sizeof(double) * (2 * LSLAB + LNMAX + 4 + 3 * LNMAX + 4 * LRS + LR) + 32 <= 160 * 1024 / LWG_PER_CU, "LDS per workgroup");
    const LongLdsPtrs L{s_slab, s_u, s_g, s_h, s_fdt, s_cf, s_q, s_bad};
    switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {       // wave-uniform by construction
        case 0: rom_long_body<GAL, PIV, 0>(a, L); break;
        case 1: rom_long_body<GAL, PIV, 1>(a, L); break;
        case 2: rom_long_body<GAL, PIV, 2>(a, L); break;
        default: rom_long_body<GAL, PIV, 3>(a, L); break;
    }
}

template <bool PIV>
void launch_long(int projection, int grid, hipStream_t st, const LongRunArgs& a)
{
    if (projection == BG_PROJ_GALERKIN)
        hipLaunchKernelGGL((rom_long_kernel<true, PIV>), dim3(grid), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((rom_long_kernel<false, PIV>), dim3(grid), dim3(256), 0, st, a);
}

}  // namespace

extern "C" {

int bg_rom_run_long_max_n(void) { return LNMAX; }
int bg_rom_run_long_max_r(void) { return LR; }
int bg_rom_run_long_workgroups_per_cu(void) { return LWG_PER_CU; }

// doubles of the padded basis copy bg_rom_run_long reads: (NPAD + 2) rows of 40, NPAD = N rounded up to 64 (any r <= 40)
long long bg_rom_run_long_phi_elems(int N, int r)
{
    if (N < 3 || N > LNMAX || r < 1 || r > LR) return 0;
    return (long long)(((N + LRS - 1) / LRS) * LRS + 2) * LR;
}

int bg_rom_run_long(int N, int B, int r, int nsteps, int projection, const double* x, const double* PhiP, const double* u0,
                    const double* mu1, const double* mu2, double dt, double E, double tol, int max_it, int options,
                    double* hist, int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    if (N < 3 || B < 0 || r < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > LNMAX) return BG_ERR_UNSUPPORTED_N;
    if (r > LR) return BG_ERR_UNSUPPORTED_R;
    if (B == 0) return BG_OK;
    if (!x || !PhiP || !u0 || !mu1 || !mu2 || !hist || !flags || !info || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    if ((uintptr_t)PhiP & 15) return BG_ERR_BAD_ARG;
    LongRunArgs a;
    a.x = x; a.PhiP = PhiP; a.u0 = u0; a.mu1 = mu1; a.mu2 = mu2; a.hist = hist; a.iters = iters; a.flags = flags; a.info = info; a.order = order;
    a.dt = dt; a.E = E; a.tol = tol; a.N = N; a.NPAD = ((N + LRS - 1) / LRS) * LRS; a.B = B; a.r = r; a.nsteps = nsteps; a.max_it = max_it;
    a.supg = options & BG_OPT_SUPG; a.nonuniform = (options & BG_OPT_NONUNIFORM) ? 1 : 0;
    a.force_pivoted = (options & BG_OPT_FORCE_PIVOTED) ? 1 : 0;
    const int cus = device_cu_count();
    const int grid = B < LWG_PER_CU * cus ? B : LWG_PER_CU * cus;
    const int grid_repair = B < cus ? B : cus;
    hipStream_t st = (hipStream_t)stream;
    if (!a.force_pivoted) {
        launch_long<false>(projection, grid, st, a);
        const int rc = check_launch();
        if (rc != BG_OK) return rc;
    }
    launch_long<true>(projection, grid_repair, st, a);         // every workgroup leaves at once unless a sample is marked
    return check_launch();
}

}  // extern "C"
