// rom_blocked.hip -- the whole POD-PROM time loop of one sample on one compute unit for the thesis' FINEST bases, r <= 256
// (bg_rom_run_blocked).  reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785; the bases are
// POD/modes/U_modes_tol_1e-05.npy (r = 160) and _1e-06.npy (r = 227), driven by POD/Results_thesis/prom_pod.py:35-58.
//
// bg_rom_run_wide (rom_wide.hip) keeps the whole reduced system on chip; an r x (r + 1) fp64 system is 207 KB at r = 160 and
// 414 KB at r = 227, more than the LDS (160 KiB) and most of the register file.  Here the system lives in a per-workgroup
// slot of a caller-provided workspace (L2 / Infinity Cache resident) and only 16-wide tiles of it are on chip at a time:
//   lift     u = Phi q: 16 lanes per mesh row, the basis read from PhiP (L2), a 16-lane DPP sum.
//   assembly A(u), R(u) of every mesh row into LDS (rom_assemble_row, the arithmetic of every other kernel).
//   projection  the padded system Ar | br is a grid of 16 x 16 tiles (RP = r rounded up to 16), Galerkin all NB^2 tiles of
//            Phi^T (A Phi), LSPG the lower triangle of (A Phi)^T (A Phi); plus one tile column [R, u, 0 ...] that yields br and
//            Phi^T u.  The tiles are dealt to the four waves; every wave sweeps the whole mesh for its own tiles on
//            v_mfma_f64_16x16x4 (no cross-wave sums).  The mesh passes in slabs of 8 rows: thread c loads column c of the
//            basis rows r0 - 1 .. r0 + 8 for the NEXT slab into registers while the matrix instructions of this one run, then
//            writes Phi and Y = A Phi (from the tridiagonal coefficients in LDS) of its column into the other LDS buffer.
//            Y is never stored outside LDS.  When the tiles of one wave exceed its accumulator budget (BT tiles) the mesh is
//            swept again for the rest.  Finished tiles go to the workspace with plain stores.
//   solve    solve(Ar, -br) (:767) as a blocked, guarded pivot-free Gauss-Jordan over 16-column panels in the workspace:
//            wave 0 factors the 16 x 16 diagonal block in registers, every thread forms the multipliers of one other row
//            (m = a U11^-1) and the panel rows' remaining columns (L11^-1 A12), and all four waves apply the rank-16 update
//            to every other row on the matrix cores, tile by tile through the workspace.  What is left is block diagonal:
//            each 16-row block is solved by its own 16 lanes.  As in bg_rom_run_wide a multiplier of a row BELOW the pivot
//            with modulus above 1 (np.linalg.solve would have exchanged rows) marks the sample BG_INFO_NEEDS_PIVOTING and the
//            caller redoes it; a zero pivot whose column below is zero as well (LAPACK's info > 0) gives info = k + 1.
// Then q = Phi^T u + dq, the stopping test, and after the last iteration one lift for U[:, n+1] = Phi q (:779).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "rom_blocked_device.hpp"

namespace {

using namespace bg;

constexpr int BNMAX = 512;             // largest mesh
// The slab, panel and item sizes and tile_ptr are rom_blocked_device.hpp's, shared with rom_hyper_blocked.hip.  The item table,
// the matrix steps, the tile store and the solve below are also there as routines (blocked_fill_items, blocked_slab_steps,
// blocked_store_tiles, blocked_solve), word for word, and this kernel does not call them: with any one of the four called
// from here the register allocation of the whole kernel changed (228 AGPRs became 174 .. 177 with one or two spilled VGPRs),
// and the kernel is meant to stay exactly what it was.  A change to one copy belongs in the other.

struct BlockedRunArgs {
    const double* x;        // [N]
    const double* PhiP;     // [NPAD + 2][RP]: Phi row i at index i + 1, zero rows around and beyond N, zero columns beyond r
    const double* u0;       // [B][N]
    const double* mu1;      // [B]
    const double* mu2;      // [B]
    double* work;           // [slots][RP][RP + 16]
    double* hist;           // [B][nsteps+1][N]
    int32_t* iters;         // [B][nsteps]
    int32_t* flags;         // [B]
    int32_t* info;          // [B]
    const int32_t* order;   // [B] or null
    double dt, E, tol;
    long long work_elems;
    int N, NPAD, B, r, RP, nsteps, max_it, supg, nonuniform, force_handback;
};

template <bool GAL>
__global__ __launch_bounds__(256, 1) void rom_blocked_kernel(BlockedRunArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_reg[BREGION];   // slab buffers (projection) / panels (solve)
    __shared__ __attribute__((aligned(16))) double s_u[BNMAX + 4];   // u at offset 2, zero halo on each side
    __shared__ double s_g[BNMAX], s_h[BNMAX], s_fdt[BNMAX];
    __shared__ __attribute__((aligned(16))) double s_cf[BNMAX][4];  // lo, di, up, R per mesh row
    __shared__ double s_q[BMAX_R], s_wtu[BMAX_R], s_dq[BMAX_R];
    __shared__ double s_red[2][4];
    __shared__ int s_item[BMAXITEMS];     // projection items: A offset | B offset << 16 (doubles into a slab buffer)
    __shared__ int s_tile[BMAXITEMS];     // a | b << 8 | (A from Y) << 16;  b = 16: the [R, u] block
    __shared__ int s_zero;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, r = a.r, RP = a.RP, NB = RP / 16, MW = RP + 16;
    const double h = (a.x[N - 1] - a.x[0]) / (double)(N - 1);
    const int nslab = a.NPAD / BSR;
    double* const M = a.work + (size_t)blockIdx.x * (size_t)a.work_elems;
    const int loff = (lane >> 4) * BSPS + (lane & 15);          // a lane's operand of a 16x16x4 step within a section

    // ---- the projection items (fixed per launch) ------------------------------------------------------------------------
    const int nitems = GAL ? NB * NB + NB : NB * (NB + 1) / 2 + 2 * NB;
    for (int j = tid; j < nitems; j += 256) {
        int ia, ib, ay;                                         // A block, B block (16: [R, u]), A from Y
        if (GAL) {
            if (j < NB * NB) { ia = j / NB; ib = j % NB; } else { ia = j - NB * NB; ib = 16; }
            ay = 0;
        } else {
            const int T = NB * (NB + 1) / 2;
            if (j < T) {
                ia = 0;
                while ((ia + 1) * (ia + 2) / 2 <= j) ++ia;
                ib = j - ia * (ia + 1) / 2; ay = 1;
            } else if (j < T + NB) { ia = j - T; ib = 16; ay = 1; }
            else { ia = j - T - NB; ib = 16; ay = 0; }
        }
        s_item[j] = (ay * BSEC + 16 * ia) | ((BSEC + 16 * ib) << 16);
        s_tile[j] = ia | (ib << 8) | (ay << 16);
    }
    if (tid < 4) s_u[tid < 2 ? tid : BNMAX + tid] = 0.0;

    for (int slot = blockIdx.x; slot < a.B; slot += gridDim.x) {
        const int smp = a.order ? a.order[slot] : slot;
        if (smp < 0 || smp >= a.B) continue;                     // workgroup-uniform
        const double mu1 = a.mu1[smp], mu2 = a.mu2[smp];
        double* hist = a.hist + (size_t)smp * (size_t)(a.nsteps + 1) * (size_t)N;
        __syncthreads();
        // ---- per-sample constants (compute_forcing_vector :427-461, f_gp of :556-558) and the initial state --------------
        for (int i = tid; i < BNMAX; i += 256) {
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
        if (tid < BMAX_R) s_q[tid] = 0.0;
        __syncthreads();

        int flags = 0, info_out = 0;
        bool aborted = false;
        PhaseClock<kPhaseClock, 4> clk;                          // diagnostic builds (tools/time_blocked_rom.py --phases)

        for (int step = 0; step < a.nsteps && info_out == 0 && !aborted; ++step) {
            // ---- g = M u^n + dt F (`M @ U[:, n] + At*F`, :746) -------------------------------------------------------------
            for (int i = tid; i < BNMAX; i += 256) {
                double g = 0.0;
                if (i < N) g = rom_mass_rhs_node(a.x, i, N, s_u[i + 1], s_u[i + 2], s_u[i + 3], s_fdt[i], h, a.nonuniform);
                s_g[i] = g;
            }
            __syncthreads();
            int k = 0;
            bool proj = true;
            while (true) {
                clk.lap(3);
                // ---- u = Phi q (:773) for iterations after the first and for U[:, n+1] (:779): 16 lanes per mesh row -------
                if (k > 0) {
                    const int c16 = lane & 15;
                    for (int i = 4 * w + (lane >> 4); i < N + 12; i += 16) {
                        const int ii = i < N ? i : N - 1;                // (lanes past the mesh redo the last row, unwritten)
                        const double* prow = a.PhiP + (size_t)(ii + 1) * RP + c16;
                        double s = 0.0;
#pragma unroll
                        for (int jj = 0; jj < 16; ++jj)
                            if (jj < NB) s = __builtin_fma(prow[16 * jj], s_q[16 * jj + c16], s);
                        s += dpp_mov<0x111>(s);            // row_shr 1, 2, 4, 8: lane 15 of the row holds the sum
                        s += dpp_mov<0x112>(s);
                        s += dpp_mov<0x114>(s);
                        s += dpp_mov<0x118>(s);
                        if (c16 == 15 && i < N) s_u[i + 2] = s;
                    }
                    __syncthreads();
                }
                if (!proj) break;                          // that was the lift for U[:, n+1] = Phi q (:779)
                clk.pass();
                // ---- A(u), R(u) of every row (:730-753) ---------------------------------------------------------------------
                {
                    const MeshConst mc = make_mesh_const(h, a.dt, a.E, a.supg);
                    for (int i = tid; i < a.NPAD; i += 256) {
                        const bool in = i < N;
                        double lo, di, up, R;
                        rom_assemble_row(i, N, s_u[i + 1], s_u[i + 2], (i + 1 < N) ? s_u[i + 3] : 0.0, in ? s_g[i] : 0.0,
                                         (in && i > 0) ? s_h[i - 1] : 0.0, (in && i < N - 1) ? s_h[i] : 0.0, mu1, mc,
                                         a.nonuniform, a.x, a.dt, a.E, lo, di, up, R);
                        *reinterpret_cast<double2*>(&s_cf[i][0]) = make_double2(lo, di);
                        *reinterpret_cast<double2*>(&s_cf[i][2]) = make_double2(up, R);
                    }
                }
                __syncthreads();
                clk.lap(0);
                // ---- projection: sweeps over the mesh, BT tiles per wave and sweep ------------------------------------------
                for (int base = 0; base < nitems; base += 4 * BT) {
                    const int left = nitems - base - w;
                    const int mine = left > 0 ? (left + 3) / 4 : 0;      // this wave's items in the sweep: base + 4 t + w
                    f64x4 acc[BT];
#pragma unroll
                    for (int t = 0; t < BT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
                    // thread c stages column c of the basis (rows r0 - 1 .. r0 + 8 = PhiP rows r0 .. r0 + 9); threads 0 .. 15
                    // also column c of the [R, u, 0 ...] block
                    double pf[BSR + 2];
                    const bool scol = tid < RP;
                    auto fetch = [&](int slab) {
#pragma unroll
                        for (int l = 0; l < BSR + 2; ++l)
                            pf[l] = scol ? a.PhiP[(size_t)(slab * BSR + l) * RP + tid] : 0.0;
                    };
                    fetch(0);
                    for (int slab = 0; slab < nslab; ++slab) {
                        double* const buf = s_reg + (slab & 1) * BBUF;
                        const int r0 = slab * BSR;
                        if (scol) {
#pragma unroll
                            for (int l = 0; l < BSR; ++l) {
                                const double2 c01 = *reinterpret_cast<const double2*>(&s_cf[r0 + l][0]);
                                const double up = s_cf[r0 + l][2];
                                buf[l * BSPS + tid] = pf[l + 1];
                                buf[BSEC + l * BSPS + tid] = __builtin_fma(up, pf[l + 2], __builtin_fma(c01.y, pf[l + 1], c01.x * pf[l]));
                            }
                        }
                        if (tid < 16) {
#pragma unroll
                            for (int l = 0; l < BSR; ++l)
                                buf[BSEC + l * BSPS + BMAX_R + tid] = tid == 0 ? s_cf[r0 + l][3] : (tid == 1 ? s_u[r0 + l + 2] : 0.0);
                        }
                        if (slab + 1 < nslab) fetch(slab + 1);   // lands while the matrix instructions below run
                        __syncthreads();
#pragma unroll
                        for (int t = 0; t < BT; ++t) {
                            if (t < mine) {
                                const int it = s_item[base + 4 * t + w];
                                const double* pa = buf + (it & 0xffff) + loff;
                                const double* pb = buf + (it >> 16) + loff;
#pragma unroll
                                for (int s = 0; s < BSR / 4; ++s)
                                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * s * BSPS], pb[4 * s * BSPS], acc[t], 0, 0, 0);
                            }
                        }
                    }
                    // ---- finished tiles -> workspace (Ar | -br), Phi^T u -> LDS ----------------------------------------------
#pragma unroll
                    for (int t = 0; t < BT; ++t) {
                        if (t < mine) {
                            const int tl = s_tile[base + 4 * t + w];
                            const int ta = tl & 0xff, tb = (tl >> 8) & 0xff, ay = tl >> 16;
                            const int col = lane & 15;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int gi = 16 * ta + (lane >> 4) + 4 * e;
                                double v = acc[t][e];
                                if (tb < 16) {
                                    const int gj = 16 * tb + col;
                                    if (gi == gj && gi >= r) v = 1.0;            // padding: identity rows
                                    M[(size_t)gi * MW + gj] = v;
                                    if (!GAL && ta != tb) M[(size_t)gj * MW + gi] = v;
                                } else {
                                    if (GAL || ay) M[(size_t)gi * MW + RP + col] = col == 0 ? -v : 0.0;
                                    if ((GAL || !ay) && col == 1) s_wtu[gi] = v;
                                }
                            }
                        }
                    }
                    __syncthreads();                           // slab buffers free for the next sweep; the tiles are stored
                }
                clk.lap(1);
                // ---- solve(Ar, -br) (:767): blocked guarded pivot-free Gauss-Jordan over 16-column panels -------------------
                double* const sL = s_reg;                      // [RP][BLS]  multipliers of every row (0 for the panel rows)
                double* const sU = s_reg + BMAX_R * BLS;       // [16][BUS]  the panel rows right of the panel (incl. -br)
                double* const sD = sU + 16 * BUS;              // [16][BLS]  L11 \ U11
                bool bad = false;
                int zstep = -1;                                // first exactly zero pivot (wave 0)
                for (int p = 0; p < NB; ++p) {
                    const int c0 = 16 * p;
                    if (w == 0) {
                        double row[16];
                        const int lr = lane & 15;
#pragma unroll
                        for (int j = 0; j < 16; ++j) row[j] = M[(size_t)(c0 + lr) * MW + c0 + j];
#pragma unroll
                        for (int kk = 0; kk < 16; ++kk) {
                            const double piv = readlane_f64(row[kk], kk);
                            double pv[16];
#pragma unroll
                            for (int j = kk + 1; j < 16; ++j) pv[j] = readlane_f64(row[j], kk);
                            if (piv == 0.0 && zstep < 0) zstep = c0 + kk;
                            if (lane > kk && lane < 16) {
                                const double av = row[kk];
                                const double m = (av == 0.0) ? 0.0 : av / piv;
                                bad = bad || !(fabs(m) <= 1.0);
#pragma unroll
                                for (int j = kk + 1; j < 16; ++j) row[j] = __builtin_fma(-m, pv[j], row[j]);
                                row[kk] = m;
                            }
                        }
                        if (lane < 16) {
#pragma unroll
                            for (int j = 0; j < 16; ++j) {
                                sD[lane * BLS + j] = row[j];
                                if (j >= lane) M[(size_t)(c0 + lane) * MW + c0 + j] = row[j];      // U11, for the last stage
                                sL[(c0 + lane) * BLS + j] = 0.0;
                            }
                        }
                    } else {
                        for (int e = tid - 64; e < RP * 16; e += 192) {
                            const int i = e >> 4, j = e & 15;
                            if (i < c0 || i >= c0 + 16) sL[i * BLS + j] = M[(size_t)i * MW + c0 + j];
                        }
                    }
                    __syncthreads();
                    // multipliers of row tid (m = a U11^-1) and the panel rows' column c0 + 16 + tid (L11^-1 A12)
                    if (tid < RP && (tid < c0 || tid >= c0 + 16)) {
                        double m[16];
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            double v = sL[tid * BLS + j];
#pragma unroll
                            for (int l = 0; l < j; ++l) v = __builtin_fma(-m[l], sD[l * BLS + j], v);
                            const double d = sD[j * BLS + j];
                            m[j] = (v == 0.0) ? 0.0 : v / d;
                            if (tid >= c0 + 16) bad = bad || !(fabs(m[j]) <= 1.0);
                        }
#pragma unroll
                        for (int j = 0; j < 16; ++j) sL[tid * BLS + j] = m[j];
                    }
                    if (tid < RP - c0) {
                        const int j = c0 + 16 + tid;
                        double x[16];
#pragma unroll
                        for (int kk = 0; kk < 16; ++kk) {
                            double v = M[(size_t)(c0 + kk) * MW + j];
#pragma unroll
                            for (int l = 0; l < kk; ++l) v = __builtin_fma(-sD[kk * BLS + l], x[l], v);
                            x[kk] = v;
                        }
#pragma unroll
                        for (int kk = 0; kk < 16; ++kk) {
                            sU[kk * BUS + tid] = x[kk];
                            M[(size_t)(c0 + kk) * MW + j] = x[kk];
                        }
                    }
                    __syncthreads();
                    // rank-16 update of every other row, columns right of the panel (the last tile column: -br)
                    const int ncol = NB - p, count = (NB - 1) * ncol;
                    for (int e0 = w; e0 < count; e0 += 4 * 8) {
                        f64x4 c[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int e = e0 + 4 * u;
                            if (e < count) {
                                const int ti0 = e / ncol, tj = e - ti0 * ncol, ti = ti0 < p ? ti0 : ti0 + 1;
                                const double* tp = tile_ptr(M, MW, ti, p + 1 + tj, lane);
#pragma unroll
                                for (int q = 0; q < 4; ++q) c[u][q] = tp[(size_t)4 * q * MW];
                            }
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int e = e0 + 4 * u;
                            if (e < count) {
                                const int ti0 = e / ncol, tj = e - ti0 * ncol, ti = ti0 < p ? ti0 : ti0 + 1;
#pragma unroll
                                for (int s = 0; s < 4; ++s) {
                                    const double am = -sL[(16 * ti + (lane & 15)) * BLS + 4 * s + (lane >> 4)];
                                    const double bu = sU[(4 * s + (lane >> 4)) * BUS + 16 * tj + (lane & 15)];
                                    c[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bu, c[u], 0, 0, 0);
                                }
                                double* tp = tile_ptr(M, MW, ti, p + 1 + tj, lane);
#pragma unroll
                                for (int q = 0; q < 4; ++q) tp[(size_t)4 * q * MW] = c[u][q];
                            }
                        }
                    }
                    __syncthreads();
                }
                // ---- block diagonal: 16 lanes per block, x = U11^-1 y --------------------------------------------------------
                {
                    const int b = tid >> 4, kk = tid & 15;
                    if (b < NB) {
                        const int gi = 16 * b + kk;
                        double urow[16];
#pragma unroll
                        for (int j = 0; j < 16; ++j) urow[j] = (j >= kk) ? M[(size_t)gi * MW + 16 * b + j] : 0.0;
                        double y = M[(size_t)gi * MW + RP], xk = 0.0;
#pragma unroll
                        for (int jj = 15; jj >= 0; --jj) {
                            const double xj = __shfl(y / urow[jj], jj, 16);
                            if (kk == jj) xk = xj;
                            if (kk < jj) y = __builtin_fma(-urow[jj], xj, y);
                        }
                        s_dq[gi] = xk;
                    }
                }
                if (w == 0 && lane == 0) s_zero = zstep;
                const bool anybad = __syncthreads_or(bad) != 0;
                clk.lap(2);
                const bool tripped = anybad || a.force_handback;                       // workgroup-uniform
                if (tripped) aborted = true;
                else if (s_zero >= 0) info_out = s_zero + 1;                            // exactly singular (LAPACK info)
                // ---- q = Phi^T u_k + dq, err = |dq| / |q|  (:770-776) -----------------------------------------------------------
                double dq = 0.0, qn = 0.0;
                if (tid < r) { dq = s_dq[tid]; qn = s_wtu[tid] + dq; }
                {
                    const double nd = wave_sum(dq * dq), nq = wave_sum(qn * qn);
                    if (lane == 0) { s_red[0][w] = nd; s_red[1][w] = nq; }
                }
                __syncthreads();
                const double nd = sqrt((s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]));
                const double nq = sqrt((s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]));
                const double err = nd / nq;
                ++k;
                const bool more = (err > a.tol) && (k < a.max_it) && !aborted && info_out == 0;
                if (!(err - err == 0.0)) flags |= BG_FLAG_NONFINITE;
                if (k >= a.max_it) flags |= BG_FLAG_HIT_CAP;
                if (tid < BMAX_R) s_q[tid] = qn;
                __syncthreads();
                if (aborted || info_out != 0) break;
                proj = more;                                   // after the last iteration: one lift-only pass
            }
            // ---- U[:, n+1] = U1 (:779): one coalesced row -------------------------------------------------------------------
            double* hrow = hist + (size_t)(step + 1) * N;
            for (int i = tid; i < N; i += 256) hrow[i] = s_u[i + 2];
            if (tid == 0) a.iters[(size_t)smp * a.nsteps + step] = k;
            clk.lap(3);
        }
        if (tid == 0) {
            a.flags[smp] = flags;
            a.info[smp] = aborted ? BG_INFO_NEEDS_PIVOTING : info_out;
            clk.store(a.iters + (size_t)smp * a.nsteps, a.nsteps);
        }
    }
}

}  // namespace

extern "C" {

int bg_rom_run_blocked_max_r(void) { return BMAX_R; }

// doubles of the padded basis bg_rom_run_blocked reads: (NPAD + 2) rows of RP, NPAD = N rounded up to 8, RP = r rounded up to 16
long long bg_rom_run_blocked_phi_elems(int N, int r)
{
    if (N < 3 || r < 1 || r > BMAX_R) return 0;
    return (long long)(((N + BSR - 1) / BSR) * BSR + 2) * blocked_rp(r);
}

// doubles of one workspace slot: the padded system [RP][RP + 16] (Ar, then -br and 15 zero columns)
long long bg_rom_run_blocked_work_elems(int N, int r)
{
    if (N < 3 || r < 1 || r > BMAX_R) return 0;
    const long long RP = blocked_rp(r);
    return RP * (RP + 16);
}

int bg_rom_run_blocked(int N, int B, int r, int nsteps, int projection, const double* x, const double* PhiP, const double* u0,
                       const double* mu1, const double* mu2, double dt, double E, double tol, int max_it, int options,
                       double* work, int slots, double* hist, int32_t* iters, int32_t* flags, int32_t* info,
                       const int32_t* order, void* stream)
{
    if (N < 3 || B < 0 || r < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > BNMAX) return BG_ERR_UNSUPPORTED_N;
    if (r > BMAX_R) return BG_ERR_UNSUPPORTED_R;
    if (B == 0) return BG_OK;
    if (!x || !PhiP || !u0 || !mu1 || !mu2 || !hist || !flags || !info || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    if (!work || slots < 1) return BG_ERR_WORKSPACE;
    BlockedRunArgs a;
    a.x = x; a.PhiP = PhiP; a.u0 = u0; a.mu1 = mu1; a.mu2 = mu2; a.work = work; a.hist = hist; a.iters = iters; a.flags = flags;
    a.info = info; a.order = order;
    a.dt = dt; a.E = E; a.tol = tol; a.work_elems = bg_rom_run_blocked_work_elems(N, r);
    a.N = N; a.NPAD = ((N + BSR - 1) / BSR) * BSR; a.B = B; a.r = r; a.RP = blocked_rp(r); a.nsteps = nsteps; a.max_it = max_it;
    a.supg = options & BG_OPT_SUPG; a.nonuniform = (options & BG_OPT_NONUNIFORM) ? 1 : 0;
    a.force_handback = (options & BG_OPT_FORCE_PIVOTED) ? 1 : 0;      // tests: every sample is handed back to the caller
    const int grid = B < slots ? B : slots;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        hipLaunchKernelGGL((rom_blocked_kernel<decltype(p)::galerkin>), dim3(grid), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
