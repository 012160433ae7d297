// rom_closure_device.hpp -- the mesh side of the closure ROM time loops (one workgroup per sample): what a reduced
// coordinate q_p and the nbar x 4 NB closure table s_J in LDS drive, whatever closure filled them.
// Used by rom_rbf_loop_device.hpp (POD-RBF: bg_rbf_rom_run, bg_rbf_rom_run_long, bg_hyper_rbf_rom_run) and
// rom_ann_wide_loop_device.hpp (POD-ANN: bg_ann_rom_run_wide, bg_hyper_ann_rom_run_wide).  What only their hyper-reduced forms
// need -- the table side, which describes that form -- is rom_hyper_table_device.hpp's, included here; the narrow POD-ANN loop
// (rom_ann_loop_device.hpp: its tangent and decode are one MFMA sweep, its dt F is in registers) and quad_device.hpp take that
// header alone.
// The pieces take LDS arrays and scalars, not a kernel-args struct.  NT: threads of the workgroup, NW = NT / 64 its waves,
// NIT: rows per thread of the strided loops, UT_LD: row stride of UT ([n + nbar][UT_LD]: U_p^T, then U_s^T, zero from N).
// The per-row loops are kept rolled (#pragma unroll 1): unrolled they take registers from the projection.
// The kernels keep the LDS overlays, the opaque re-derivation of the thread indices in front of the register-heavy
// phases, mfma_passes, pivoted_solve and the issue priorities.
#pragma once
#include "rom_fused_device.hpp"
#include "rom_hyper_table_device.hpp"

namespace bg {
namespace fused {

// The halo rows of a lane's block of S tangent rows: the last row of the block below and the first row of the block above,
// published by their owners in s_ehi / s_elo (the tangent is formed in registers, see tangent_fragments); zero outside the
// mesh.  LAST: the last owner (16 NW - 1).
template <int NB, int LAST = 63>
struct HaloEdges {
    const double (*elo)[4 * NB];
    const double (*ehi)[4 * NB];
    int owner, t;
    template <int S>
    __device__ __forceinline__ double operator()(int side, int c, const double (&)[NB][S], int = 0) const
    {
        if (side == 0) {
            const double v = ehi[owner > 0 ? owner - 1 : 0][4 * c + t];
            return owner > 0 ? v : 0.0;
        }
        const double v = elo[owner < LAST ? owner + 1 : LAST][4 * c + t];
        return owner < LAST ? v : 0.0;
    }
};

// ---- per-sample constants (compute_forcing_vector :427-461, f_gp of :556-558) and the initial state, row i: dt F into
// s_fdt, the SUPG term's element loads hf into s_h, u0 into s_u (offset 2) and, HIST, into row 0 of the sample's history
// (the hyper-reduced forms keep no history of u: hist is not read).  The rolled loop over a thread's rows stays in the
// kernels: inside this function it moved the SGPR spills of rom_rbf_fused's S = 4 instantiations (213 -> 242).
template <bool HIST = true>
__device__ __forceinline__ void sample_setup_row(int i, const double* x, const double* u0, int smp, double* hist, int N,
                                                 double mu2, double h, int nonuniform, double dt, double* s_u, double* s_fdt,
                                                 double* s_h)
{
    double frPrev = 0.0, fl = 0.0, hf = 0.0, u = 0.0;
    if (i < N) {
        rom_nodal_forcing(x, i, N, mu2, h, nonuniform, frPrev, fl, hf);
        u = u0[(size_t)smp * N + i];
        if constexpr (HIST) hist[i] = u;
    }
    s_fdt[i] = dt * (frPrev + fl);
    s_h[i] = hf;
    s_u[i + 2] = u;
}

// ---- q = U_p^T u into s_q (zero from n): per-wave partial sums in s_part, summed in a fixed order.  row(i, u_i) runs
// once per row of the same trip, ahead of its FMAs (rom_ann_wide forms g there).  Ends with a barrier.
template <int NIT, int NT, int NW, int UT_LD, int RW, class Row>
__device__ __forceinline__ void project_q(const double* __restrict__ UT, const double* s_u, int n, int tid, int lane, int w,
                                          double (*s_part)[RW], double* s_q, const Row& row)
{
    static_assert(NW == 4 || NW == 8, "the fixed summation orders of four and of eight waves");
    double part[RW];
#pragma unroll
    for (int c = 0; c < RW; ++c) part[c] = 0.0;
#pragma unroll 1
    for (int ii = 0; ii < NIT; ++ii) {
        const int i = tid + NT * ii;
        const double uc = s_u[i + 2];    // zero beyond N
        row(i, uc);
#pragma unroll
        for (int c = 0; c < RW; ++c)
            if (c < n) part[c] = __builtin_fma(UT[(size_t)c * UT_LD + i], uc, part[c]);
    }
#pragma unroll
    for (int c = 0; c < RW; ++c) {
        if (c < n) {
            const double sm = wave_sum(part[c]);
            if (lane == 0) s_part[w][c] = sm;
        }
    }
    __syncthreads();
    if constexpr (NW == 4) {
        if (tid < RW) s_q[tid] = (tid < n) ? (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]) : 0.0;
    } else {
        if (tid < RW)
            s_q[tid] = (tid < n) ? ((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])) +
                                       ((s_part[4][tid] + s_part[5][tid]) + (s_part[6][tid] + s_part[7][tid])) : 0.0;
    }
    __syncthreads();
}

// ---- tangent W = U_p + U_s J in this lane's projection fragments: rows rowbase .. + S - 1, column 4 c + t (the layout of
// mfma_pass), no N x n copy in LDS; rows beyond N are zero (UT is zero there).  s_J[j][c] = d f_j / d q_c, zero from c = n.
template <int S, int NB, int UT_LD>
__device__ __forceinline__ void tangent_fragments(double (&frag)[NB][S], const double* __restrict__ UT,
                                                  const double (*__restrict__ s_J)[4 * NB], int n, int nbar, int rowbase, int t)
{
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
        for (int s = 0; s < S; ++s) frag[c][s] = 0.0;
    const double* __restrict__ us = UT + (size_t)n * UT_LD + rowbase;
#pragma unroll 4
    for (int j = 0; j < nbar; ++j) {
        double uv[S];
#pragma unroll
        for (int s = 0; s < S; s += 2) {
            const double2 v = *reinterpret_cast<const double2*>(us + (size_t)j * UT_LD + s);
            uv[s] = v.x; uv[s + 1] = v.y;
        }
        double jv[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) jv[c] = s_J[j][4 * c + t];
#pragma unroll
        for (int c = 0; c < NB; ++c)
#pragma unroll
            for (int s = 0; s < S; ++s) frag[c][s] = __builtin_fma(uv[s], jv[c], frag[c][s]);
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        const int col = 4 * c + t;
        const double* __restrict__ up = UT + (size_t)(col < n ? col : 0) * UT_LD + rowbase;
#pragma unroll
        for (int s = 0; s < S; s += 2) {
            const double2 v = *reinterpret_cast<const double2*>(up + s);
            frag[c][s] += col < n ? v.x : 0.0;
            frag[c][s + 1] += col < n ? v.y : 0.0;
        }
    }
}

// the first and last tangent row of this lane's block, for the neighbouring owners (HaloEdges)
template <int S, int NB>
__device__ __forceinline__ void publish_edges(const double (&frag)[NB][S], double (*s_elo)[4 * NB], double (*s_ehi)[4 * NB],
                                              int owner, int t)
{
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        s_elo[owner][4 * c + t] = frag[c][0];
        s_ehi[owner][4 * c + t] = frag[c][S - 1];
    }
}

// ---- assembly: A(u_k), R(u_k) per row into s_coef (lower, diagonal, upper, residual)
template <int NPAD, int NT>
__device__ __forceinline__ void assemble_rows(double (*s_coef)[4], const double* s_u, const double* s_g, const double* s_h,
                                              const double* x, int N, double h, double dt, double E, int supg, int nonuniform,
                                              double mu1, int tid)
{
    for (int i = tid; i < NPAD; i += NT) {
        double lo, di, up, R;
        const bool in = i < N;
        const MeshConst mc = make_mesh_const(h, dt, E, supg);
        rom_assemble_row(i, N, s_u[i + 1], s_u[i + 2], (i + 1 < N) ? s_u[i + 3] : 0.0, in ? s_g[i] : 0.0,
                         (in && i > 0) ? s_h[i - 1] : 0.0, (in && i < N - 1) ? s_h[i] : 0.0, mu1, mc, nonuniform, x, dt, E,
                         lo, di, up, R);
        s_coef[i][0] = lo; s_coef[i][1] = di; s_coef[i][2] = up; s_coef[i][3] = R;
    }
}

// ---- q += dq with dq = s_x of the solve; returns rule(|dq|, |q_new|), the error of the stopping test, in every thread.
// A barrier on either side of the write of s_q.
template <int RW, class Rule>
__device__ __forceinline__ double update_q(double* s_q, const double* s_x, int n, int lane, int w, const Rule& rule)
{
    const double dq = (lane < n) ? s_x[lane] : 0.0;
    const double qn = (lane < n) ? s_q[lane] + dq : 0.0;
    double nd, nq;
    wave_sum2(dq * dq, qn * qn, nd, nq);
    nd = sqrt(nd); nq = sqrt(nq);
    const double err = rule(nd, nq);
    __syncthreads();                         // every wave has read s_q and s_x
    if (w == 0 && lane < RW) s_q[lane] = qn;
    __syncthreads();
    return err;
}

// ---- decode u = U_p q + U_s f into s_u (zero from N).  Ends with a barrier.
template <int NIT, int NT, int UT_LD>
__device__ __forceinline__ void decode_u(double* s_u, const double* __restrict__ UT, const double* s_q, const double* s_f,
                                         int N, int n, int nbar, int tid)
{
#pragma unroll 1
    for (int ii = 0; ii < NIT; ++ii) {
        const int i = tid + NT * ii;
        double up = 0.0, us = 0.0;
#pragma unroll 4
        for (int c = 0; c < n; ++c) up = __builtin_fma(UT[(size_t)c * UT_LD + i], s_q[c], up);
        const double* __restrict__ ucol = UT + (size_t)n * UT_LD + i;
#pragma unroll 8
        for (int j = 0; j < nbar; ++j) us = __builtin_fma(ucol[(size_t)j * UT_LD], s_f[j], us);
        s_u[i + 2] = (i < N) ? up + us : 0.0;
    }
    __syncthreads();
}

// one row of the sample's history from s_u
template <int NT>
__device__ __forceinline__ void write_hist_row(double* hrow, const double* s_u, int N, int tid)
{
    for (int i = tid; i < N; i += NT) hrow[i] = s_u[i + 2];
}

}  // namespace fused
}  // namespace bg
