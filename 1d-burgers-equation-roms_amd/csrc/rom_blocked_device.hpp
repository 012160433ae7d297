// rom_blocked_device.hpp -- what the two blocked POD-PROM time loops share (rom_blocked.hip: bg_rom_run_blocked, the mesh rows;
// rom_hyper_blocked.hip: bg_hyper_rom_run_blocked, a table of sampled rows): the sizes of the slab buffers and panels, the
// projection items dealt to the four waves, the v_mfma_f64_16x16x4 steps over one slab buffer, the store of the finished tiles
// into the workspace slot, and the blocked guarded pivot-free Gauss-Jordan over 16-column panels there.  What differs between
// the two -- where the rows of a slab come from, and whether the extra tile column carries u for Phi^T u -- stays with them.
// rom_hyper_blocked.hip calls all of it.  rom_blocked.hip takes the sizes and tile_ptr from here and keeps the text of the four
// routines in its kernel (it says why: called from there they changed that kernel's register allocation); the two texts are
// meant to stay word for word the same.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rom_device.hpp"

namespace bg {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int BMAX_R = 256;            // largest reduced dimension (16 tiles of 16)
constexpr int BSR = 8;                 // rows per slab (two k-steps of the 16x16x4 instruction)
constexpr int BSPS = BMAX_R + 16;      // doubles per LDS slab row: RP columns, then the [R, u, 0 ...] block at 256
constexpr int BSEC = BSR * BSPS;       // one section (Phi or Y) of a slab buffer
constexpr int BBUF = 2 * BSEC;         // one slab buffer: Phi rows, then Y rows
constexpr int BT = 38;                 // accumulator tiles per wave and sweep of rom_blocked_kernel (304 registers)
constexpr int BMAXITEMS = 16 * 16 + 16;
constexpr int BLS = 17;                // row stride of the multiplier panel in LDS
constexpr int BUS = BMAX_R + 16;       // row stride of the U12 panel in LDS
constexpr int BREGION = 2 * BBUF > BMAX_R * BLS + 16 * BUS + 16 * BLS ? 2 * BBUF : BMAX_R * BLS + 16 * BUS + 16 * BLS;

inline int blocked_rp(int r) { return ((r + 15) / 16) * 16; }

// the 16 x 16 tile (ta, tb) of the workspace: lane's four entries (row (lane >> 4) + 4 i, column lane & 15)
__device__ __forceinline__ double* tile_ptr(double* M, int MW, int ta, int tb, int lane)
{
    return M + (size_t)(16 * ta + (lane >> 4)) * MW + 16 * tb + (lane & 15);
}

// The projection items of a launch: Galerkin all NB^2 tiles of Phi^T Y, LSPG the lower triangle of Y^T Y, then one tile
// column against the extra block of the Y section ([R, u, 0 ...]): from Y for LSPG's br, from Phi for Galerkin's br and, with
// WTU, for Phi^T u of either projection.
template <bool GAL, bool WTU>
__device__ __forceinline__ int blocked_item_count(int NB)
{
    return GAL ? NB * NB + NB : NB * (NB + 1) / 2 + (WTU ? 2 : 1) * NB;
}

// s_item: A offset | B offset << 16 (doubles into a slab buffer);  s_tile: a | b << 8 | (A from Y) << 16;  b = 16: the extra block
template <bool GAL>
__device__ __forceinline__ void blocked_fill_items(int* s_item, int* s_tile, int nitems, int NB, int tid)
{
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
}

// the matrix steps of one slab buffer for the `mine` <= NT items base + 4 t + w of this wave (NT: its accumulator budget);
// loff: a lane's operand of a 16x16x4 step within a section, (lane >> 4) * BSPS + (lane & 15)
template <int NT>
__device__ __forceinline__ void blocked_slab_steps(f64x4 (&acc)[NT], const double* buf, const int* s_item, int base, int w, int mine,
                                                   int loff)
{
#pragma unroll
    for (int t = 0; t < NT; ++t) {
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

// finished tiles -> workspace (Ar | -br); WTU: Phi^T u (column 1 of the extra block) -> s_wtu
template <bool GAL, bool WTU, int NT>
__device__ __forceinline__ void blocked_store_tiles(const f64x4 (&acc)[NT], const int* s_tile, int base, int w, int mine, int lane,
                                                    double* M, int MW, int RP, int r, double* s_wtu)
{
#pragma unroll
    for (int t = 0; t < NT; ++t) {
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
                    if constexpr (WTU) {
                        if ((GAL || !ay) && col == 1) s_wtu[gi] = v;
                    }
                }
            }
        }
    }
}

// solve(Ar, -br) (:767): blocked guarded pivot-free Gauss-Jordan over 16-column panels in the workspace slot M [RP][MW], the
// panels in s_reg (BREGION doubles); x -> s_dq.  bad: this thread met a multiplier above 1 below the pivot; zstep: the first
// exactly zero pivot (wave 0), -1 if none.
__device__ __forceinline__ void blocked_solve(double* M, int MW, int RP, int NB, double* s_reg, double* s_dq, int tid, int lane, int w,
                                              bool& bad_out, int& zstep_out)
{
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
    bad_out = bad;
    zstep_out = zstep;
}

}  // namespace bg
