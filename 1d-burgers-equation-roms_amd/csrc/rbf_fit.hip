// rbf_fit.hip -- the offline fit of the POD-RBF closure (burgers_hip/pod.py build_rbf_closure): the kernel matrix of the
// scaled centres and a blocked Cholesky factorisation and solve of (K + ridge I) W = Y, all in fp64 and in 64 x 64 tiles.
//
// gram     bg_rbf_gram: one workgroup per tile (I, J); the two 64-centre coordinate blocks pass through LDS 32 coordinates
//          at a time, thread (column, row group) keeps 16 squared distances, r2 += d^2 by FMA in the order of k -- the sum
//          of csrc/rbf.hip, then the form of rbf_device.hpp.  (a - b)^2 = (b - a)^2, so tile (J, I) holds the transposed bits of tile (I, J).
// factor   bg_chol_factor: right-looking over 64-column blocks, three launches per block column k:
//            chol_panel<true>   one workgroup factors the diagonal tile and records info;
//            chol_panel<false>  one workgroup per tile below solves X L11^T = A21;
//            chol_update        one workgroup per tile pair I >= J > k: C_IJ -= L_Ik L_Jk^T.
//          A panel thread owns row i and the columns c = 4 q + g of its tile in registers (g = its wave).  Column j is
//          finished by its owner wave, goes to LDS, and after one barrier every thread subtracts its share: element (i, c)
//          receives the columns j = 0 .. c - 1 in that order, whatever the grid.  The update multiplies the two panels out
//          of LDS, on v_mfma_f64_16x16x4_f64 (a wave owns a 32 x 32 quarter, four accumulators seeded with C, the A operand
//          negated, 16 instructions of 4 terms in the order of k) or, with -DBG_CHOL_TILE_VALU, by 64 FMAs per element in
//          the order of k.  Either way an element's bits depend on its own row and column of tiles alone.
// solve    bg_chol_solve: forward over the block rows k = 0 .. and backward over k = last .. 0, two launches per block:
//          solve_diag (one workgroup per 16 right-hand sides substitutes through the diagonal tile) and solve_update (one
//          workgroup per tile row and 16 right-hand sides: B_I -= M X_k, 64 FMAs per element in the order of the rows of
//          block k).  A column's arithmetic does not involve the other columns.
// Ragged last tiles are masked in the kernels (zeros come in, nothing goes out).  No floating-point atomics, no workspace.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "rbf_device.hpp"

namespace {

constexpr int CH_MAX_N = 16384;
constexpr int TB = 64;                        // tile edge
constexpr int PP = TB + 1;                    // LDS pitch of the panel kernels: column-of-a-tile major, no bank conflicts
constexpr int UP = TB + 2;                    // LDS pitch of the update kernel: the MFMA operand reads hit 32 distinct banks
constexpr int SW = 16;                        // right-hand sides per workgroup of the solve kernels
constexpr int GK = 32;                        // coordinates per LDS pass of the gram kernel

// ---- kernel matrix ----------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void rbf_gram_kernel(int Ns, int n, const double* __restrict__ XtT, double* __restrict__ A,
                                                       size_t lda, double eps2, double diag)
{
    __shared__ double si[GK][TB], sj[GK][TB];
    const int t = threadIdx.x, tj = t & 63, tg = t >> 6;
    const int i0 = TB * blockIdx.y, j0 = TB * blockIdx.x;
    double r2[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) r2[q] = 0.0;
    for (int kc = 0; kc < n; kc += GK) {
        const int kn = min(GK, n - kc);
        __syncthreads();
        for (int e = t; e < kn * TB; e += 256) {
            const int k = e >> 6, c = e & 63;
            const double* row = XtT + (size_t)(kc + k) * (size_t)Ns;
            si[k][c] = i0 + c < Ns ? row[i0 + c] : 0.0;
            sj[k][c] = j0 + c < Ns ? row[j0 + c] : 0.0;
        }
        __syncthreads();
        for (int k = 0; k < kn; ++k) {
            const double xj = sj[k][tj];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const double d = si[k][16 * tg + q] - xj;
                r2[q] = __builtin_fma(d, d, r2[q]);
            }
        }
    }
    const int j = j0 + tj;
    if (j >= Ns) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = i0 + 16 * tg + q;
        if (i >= Ns) continue;
        const double p = bg::rbf_value(KIND, eps2, r2[q]);
        A[(size_t)i * lda + j] = i == j ? diag : p;
    }
}

// ---- factorisation ----------------------------------------------------------------------------------------------------
// DIAG: the diagonal tile at (k0, k0) is factored in place (lower triangle; the upper one is neither read nor written).
// otherwise: workgroup b solves X L11^T = A21 for the tile at rows k0 + 64 (b + 1).
template <bool DIAG>
__global__ __launch_bounds__(256) void chol_panel_kernel(int n, int k0, double* __restrict__ A, size_t lda,
                                                         int* __restrict__ info, int first)
{
    __shared__ double sx[TB][PP];             // sx[c][i]: the tile, then its finished columns
    __shared__ double sl[DIAG ? 1 : TB][DIAG ? 1 : PP];   // L11[c][j]
    __shared__ int s_bad[4];
    if (!(DIAG && first) && *info != 0) return;
    const int t = threadIdx.x, i = t & 63, g = t >> 6;
    const int nb = min(TB, n - k0);
    const int r0 = DIAG ? k0 : k0 + TB * ((int)blockIdx.x + 1);
    const int nr = min(TB, n - r0);
    for (int e = t; e < TB * TB; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        const bool in = rr < nr && cc < nb && (!DIAG || cc <= rr);
        sx[cc][rr] = in ? A[(size_t)(r0 + rr) * lda + k0 + cc] : (DIAG && rr == cc ? 1.0 : 0.0);
        if (!DIAG) sl[rr][cc] = rr < nb && cc <= rr ? A[(size_t)(k0 + rr) * lda + k0 + cc] : (rr == cc ? 1.0 : 0.0);
    }
    __syncthreads();
    double a[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = sx[4 * q + g][i];
    int bad = 0;
#pragma unroll
    for (int j = 0; j < TB; ++j) {
        if ((j & 3) == g) {                   // the wave that owns column j finishes it
            double x;
            if (DIAG) {
                const double d = __shfl(a[j >> 2], j);
                if ((!(d > 0.0) || isinf(d)) && bad == 0) bad = k0 + j + 1;
                const double r = sqrt(d);
                x = i == j ? r : (i > j ? a[j >> 2] / r : 0.0);
            } else {
                x = a[j >> 2] / sl[j][j];
            }
            sx[j][i] = x;
        }
        __syncthreads();
        const double xj = sx[j][i];
#pragma unroll
        for (int q = j >> 2; q < 16; ++q) {
            const int c = 4 * q + g;
            const double l = DIAG ? sx[j][c] : sl[c][j];
            if (c > j) a[q] = __builtin_fma(-xj, l, a[q]);
        }
    }
    if (DIAG && i == 0) s_bad[g] = bad;
    __syncthreads();
    for (int e = t; e < TB * TB; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        if (rr < nr && cc < nb && (!DIAG || cc <= rr)) A[(size_t)(r0 + rr) * lda + k0 + cc] = sx[cc][rr];
    }
    if (DIAG && t == 0) {
        int v = 0;
        for (int w = 0; w < 4; ++w)
            if (s_bad[w] != 0 && (v == 0 || s_bad[w] < v)) v = s_bad[w];
        if (first || v != 0) *info = v;
    }
}

// C_IJ -= L_Ik L_Jk^T for the tile pair (I, J) = (blockIdx.y, blockIdx.x), I >= J, counted from the first tile below k0.
__global__ __launch_bounds__(256) void chol_update_kernel(int n, int k0, double* __restrict__ A, size_t lda,
                                                          const int* __restrict__ info)
{
    __shared__ double sa[TB][UP], sb[TB][UP];
    if (*info != 0) return;
    const int J = blockIdx.x, I = blockIdx.y;
    if (J > I) return;
    const int t = threadIdx.x;
    const int i0 = k0 + TB * (I + 1), j0 = k0 + TB * (J + 1);
    const int ni = min(TB, n - i0), nj = min(TB, n - j0);
    for (int e = t; e < TB * TB; e += 256) {
        const int rr = e >> 6, kk = e & 63;
        sa[rr][kk] = rr < ni ? A[(size_t)(i0 + rr) * lda + k0 + kk] : 0.0;
        sb[rr][kk] = rr < nj ? A[(size_t)(j0 + rr) * lda + k0 + kk] : 0.0;
    }
    __syncthreads();
    const bool diag = I == J;
#ifndef BG_CHOL_TILE_VALU
    typedef double double4v __attribute__((ext_vector_type(4)));
    const int l = t & 63, w = t >> 6, rb = 32 * (w >> 1), cb = 32 * (w & 1);
    double4v acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = rb + 16 * u + (l >> 4) + 4 * q, col = cb + 16 * v + (l & 15);
                const bool in = row < ni && col < nj && (!diag || col <= row);
                acc[u][v][q] = in ? A[(size_t)(i0 + row) * lda + j0 + col] : 0.0;
            }
#pragma unroll
    for (int s = 0; s < TB / 4; ++s) {
        double fa[2], fb[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            fa[u] = -sa[rb + 16 * u + (l & 15)][4 * s + (l >> 4)];
            fb[u] = sb[cb + 16 * u + (l & 15)][4 * s + (l >> 4)];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[u], fb[v], acc[u][v], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = rb + 16 * u + (l >> 4) + 4 * q, col = cb + 16 * v + (l & 15);
                if (row < ni && col < nj && (!diag || col <= row)) A[(size_t)(i0 + row) * lda + j0 + col] = acc[u][v][q];
            }
#else
    const int tx = t & 15, ty = t >> 4;
    double c[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = ty + 16 * u, col = tx + 16 * v;
            const bool in = row < ni && col < nj && (!diag || col <= row);
            c[u][v] = in ? A[(size_t)(i0 + row) * lda + j0 + col] : 0.0;
        }
#pragma unroll 8
    for (int k = 0; k < TB; ++k) {
        double fa[4], fb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            fa[u] = -sa[ty + 16 * u][k];
            fb[u] = sb[tx + 16 * u][k];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) c[u][v] = __builtin_fma(fa[u], fb[v], c[u][v]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = ty + 16 * u, col = tx + 16 * v;
            if (row < ni && col < nj && (!diag || col <= row)) A[(size_t)(i0 + row) * lda + j0 + col] = c[u][v];
        }
#endif
}

// ---- solve ------------------------------------------------------------------------------------------------------------
// The rows k0 .. of 16 right-hand sides through the diagonal tile: L11 y = b (FWD) or L11^T x = y.  Thread (column c, row
// group h) owns the rows h + 16 u of column c; row j is finished by its owner, goes to LDS, and after one barrier every
// thread subtracts its share.
template <bool FWD>
__global__ __launch_bounds__(256) void solve_diag_kernel(int n, int nrhs, int k0, const double* __restrict__ L, size_t lda,
                                                         double* __restrict__ Bm, size_t ldb)
{
    __shared__ double sl[TB][PP];             // FWD: sl[j][r] = L11[r][j], otherwise sl[j][r] = L11[j][r]: the multipliers of row j
    __shared__ double sy[TB][SW];
    const int t = threadIdx.x, c = t & 15, h = t >> 4;
    const int c0 = SW * blockIdx.x, nc = min(SW, nrhs - c0), nb = min(TB, n - k0);
    for (int e = t; e < TB * TB; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        const double v = rr < nb && cc <= rr ? L[(size_t)(k0 + rr) * lda + k0 + cc] : (rr == cc ? 1.0 : 0.0);
        if (FWD) sl[cc][rr] = v; else sl[rr][cc] = v;
    }
    double b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = h + 16 * u;
        b[u] = r < nb && c < nc ? Bm[(size_t)(k0 + r) * ldb + c0 + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int so = 0; so < 4; ++so) {          // the owner's register index is static; the 16 rows of a group stay a loop
                                              // (all 64 steps unrolled crash the register coalescer of hipcc 7.2)
        const int uo = FWD ? so : 3 - so;
#pragma unroll 1
        for (int s = 0; s < 16; ++s) {
            const int j = 16 * uo + (FWD ? s : 15 - s);
            if ((j & 15) == h) sy[j][c] = b[uo] / sl[j][j];
            __syncthreads();
            const double y = sy[j][c];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = h + 16 * u;
                if (FWD ? r > j : r < j) b[u] = __builtin_fma(-sl[j][r], y, b[u]);
            }
        }
    }
    for (int e = t; e < TB * SW; e += 256) {
        const int r = e >> 4, cc = e & 15;
        if (r < nb && cc < nc) Bm[(size_t)(k0 + r) * ldb + c0 + cc] = sy[r][cc];
    }
}

// B_I -= M X_k for 16 right-hand sides, M = L_Ik (FWD, I = k + 1 + blockIdx.y) or L_kI^T (I = blockIdx.y < k).
template <bool FWD>
__global__ __launch_bounds__(256) void solve_update_kernel(int n, int nrhs, int k0, const double* __restrict__ L, size_t lda,
                                                           double* __restrict__ Bm, size_t ldb)
{
    __shared__ double sm[TB][PP];             // sm[k][r] = M[r][k]
    __shared__ double sx[TB][SW];
    const int t = threadIdx.x, r = t & 63, cg = t >> 6;
    const int c0 = SW * blockIdx.x, nc = min(SW, nrhs - c0), nb = min(TB, n - k0);
    const int i0 = FWD ? k0 + TB * ((int)blockIdx.y + 1) : TB * (int)blockIdx.y;
    const int ni = min(TB, n - i0);
    for (int e = t; e < TB * TB; e += 256) {
        const int rr = e >> 6, cc = e & 63;
        if (FWD) sm[cc][rr] = rr < ni ? L[(size_t)(i0 + rr) * lda + k0 + cc] : 0.0;        // L_Ik[rr][cc], cc < 64 <= columns of k
        else sm[rr][cc] = rr < nb ? L[(size_t)(k0 + rr) * lda + i0 + cc] : 0.0;            // L_kI[rr][cc]
    }
    for (int e = t; e < TB * SW; e += 256) {
        const int k = e >> 4, cc = e & 15;
        sx[k][cc] = k < nb && cc < nc ? Bm[(size_t)(k0 + k) * ldb + c0 + cc] : 0.0;
    }
    __syncthreads();
    double b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int cc = 4 * cg + u;
        b[u] = r < ni && cc < nc ? Bm[(size_t)(i0 + r) * ldb + c0 + cc] : 0.0;
    }
#pragma unroll 8
    for (int k = 0; k < TB; ++k) {
        const double m = -sm[k][r];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = __builtin_fma(m, sx[k][4 * cg + u], b[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int cc = 4 * cg + u;
        if (r < ni && cc < nc) Bm[(size_t)(i0 + r) * ldb + c0 + cc] = b[u];
    }
}

}  // namespace

extern "C" int bg_chol_max_n(void) { return CH_MAX_N; }

extern "C" int bg_rbf_gram(int Ns, int n, int kind, double eps, double ridge, const double* XtT, double* A, int lda, void* stream)
{
    if (Ns < 0 || n < 1 || lda < Ns) return BG_ERR_BAD_ARG;
    if (kind != BG_RBF_GAUSSIAN && kind != BG_RBF_IMQ) return BG_ERR_BAD_ARG;
    if (!(ridge >= 0.0) || isinf(ridge)) return BG_ERR_BAD_ARG;
    if (Ns == 0) return BG_OK;
    if (Ns > CH_MAX_N) return BG_ERR_UNSUPPORTED_R;
    if (!XtT || !A) return BG_ERR_BAD_ARG;
    const int nt = (Ns + TB - 1) / TB;
    const dim3 grid(nt, nt), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (kind == BG_RBF_GAUSSIAN)
        hipLaunchKernelGGL(rbf_gram_kernel<BG_RBF_GAUSSIAN>, grid, block, 0, st, Ns, n, XtT, A, (size_t)lda, eps * eps, 1.0 + ridge);
    else
        hipLaunchKernelGGL(rbf_gram_kernel<BG_RBF_IMQ>, grid, block, 0, st, Ns, n, XtT, A, (size_t)lda, eps * eps, 1.0 + ridge);
    return bg::check_launch();
}

extern "C" int bg_chol_factor(int n, double* A, int lda, int* info, void* stream)
{
    if (n < 0 || lda < n) return BG_ERR_BAD_ARG;
    if (n == 0) return BG_OK;
    if (n > CH_MAX_N) return BG_ERR_UNSUPPORTED_R;
    if (!A || !info) return BG_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nt = (n + TB - 1) / TB;
    for (int k = 0; k < nt; ++k) {
        const int k0 = TB * k, below = nt - k - 1;
        hipLaunchKernelGGL(chol_panel_kernel<true>, dim3(1), dim3(256), 0, st, n, k0, A, (size_t)lda, info, k == 0 ? 1 : 0);
        if (below > 0) {
            hipLaunchKernelGGL(chol_panel_kernel<false>, dim3(below), dim3(256), 0, st, n, k0, A, (size_t)lda, info, 0);
            hipLaunchKernelGGL(chol_update_kernel, dim3(below, below), dim3(256), 0, st, n, k0, A, (size_t)lda, info);
        }
        const int rc = bg::check_launch();
        if (rc != BG_OK) return rc;
    }
    return BG_OK;
}

extern "C" int bg_chol_solve(int n, int nrhs, const double* L, int lda, double* Bm, int ldb, void* stream)
{
    if (n < 0 || nrhs < 0 || lda < n || ldb < nrhs) return BG_ERR_BAD_ARG;
    if (n == 0 || nrhs == 0) return BG_OK;
    if (n > CH_MAX_N) return BG_ERR_UNSUPPORTED_R;
    if (!L || !Bm) return BG_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nt = (n + TB - 1) / TB, chunks = (nrhs + SW - 1) / SW;
    for (int k = 0; k < nt; ++k) {
        const int k0 = TB * k, below = nt - k - 1;
        hipLaunchKernelGGL(solve_diag_kernel<true>, dim3(chunks), dim3(256), 0, st, n, nrhs, k0, L, (size_t)lda, Bm, (size_t)ldb);
        if (below > 0)
            hipLaunchKernelGGL(solve_update_kernel<true>, dim3(chunks, below), dim3(256), 0, st, n, nrhs, k0, L, (size_t)lda, Bm, (size_t)ldb);
        const int rc = bg::check_launch();
        if (rc != BG_OK) return rc;
    }
    for (int k = nt - 1; k >= 0; --k) {
        const int k0 = TB * k;
        hipLaunchKernelGGL(solve_diag_kernel<false>, dim3(chunks), dim3(256), 0, st, n, nrhs, k0, L, (size_t)lda, Bm, (size_t)ldb);
        if (k > 0)
            hipLaunchKernelGGL(solve_update_kernel<false>, dim3(chunks, k), dim3(256), 0, st, n, nrhs, k0, L, (size_t)lda, Bm, (size_t)ldb);
        const int rc = bg::check_launch();
        if (rc != BG_OK) return rc;
    }
    return BG_OK;
}
