// rom_hyper_table_device.hpp -- the table side of the hyper-reduced device loops that run a full loop's body on the table of
// a row sampling: bg_hyper_rbf_rom_run (rom_rbf_loop_device.hpp), bg_hyper_ann_rom_run_wide (rom_ann_wide_loop_device.hpp),
// bg_hyper_ann_rom_run (rom_ann_loop_device.hpp) and bg_hyper_quad_rom_run (quad_device.hpp).  (The stencil-based loops of
// rom_hyper.hip share a body of their own.)
//
// The hyper-reduced form.  Both projections are sums over mesh rows, Ar = sum_i w_i^T y_i and br = sum_i w_i^T R_i, and row i
// needs the state, the tangent and the coordinates at nodes i - 1, i, i + 1 only.  The caller packs the sorted distinct stencil
// nodes of the m sampled rows (node[k], k < nodes <= 3 m) with their coordinates and the rows of the basis at them; the three
// stencil nodes of a sampled row are consecutive integers and therefore consecutive table entries, so the table is a mesh on
// which a sampled row's neighbours are its table neighbours, and the whole body of the full loop runs on it with `nodes` for
// N: tangent and decode are formed at the table nodes, forcing and mass row read the table coordinates as a non-uniform
// mesh x.  What differs from the full loop:
//   - a table node that is only a neighbour assembles as a row outside the mesh (an identity row) and every coefficient is
//     multiplied by the row's weight xi (Galerkin) or sqrt(xi) (LSPG), 0 there -- its row vanishes from both sums; whether a
//     sampled row is the Dirichlet row or the last row is decided by node[k] against the MESH's node count (a sampled row 0
//     is table node 0 and a sampled row N - 1 the last table node, so forcing and mass row may ask the table index).  Mesh
//     row and factor of a table node are the same for every sample: formed once per workgroup (hyper_scatter_rows,
//     hyper_table_node), held in LDS or in registers;
//   - the run starts from q_p = q0 (the caller's U_p^T u0) and u0 gathered at the table nodes, and q_p carries over between
//     iterations and steps: there is no U_p^T u^n (equal to the previous q_p for orthonormal [U_p U_s]; the quadratic
//     manifold's reason is in quad_device.hpp);
//   - the outputs are q_p and, in the closure loops, the closure value q_s = N(q_p) of every step's decode (row 0: zero, no
//     closure value belongs to u0); no vector of mesh length is touched.
// As in rom_closure_device.hpp the pieces take LDS arrays and scalars, not a kernel-args struct; NT: threads of the workgroup.
// The set-up row of a sample is rom_closure_device.hpp's sample_setup_row<false>.  What stays in the kernels, because moved
// it changed what the compiler made of them (profiles/hyper_table_side_resource_usage.md): the mass right-hand side sweep
// of a step (in the POD-RBF loop it is one loop for both forms) and the step write of the wide POD-ANN loop.
#pragma once
#include <stdint.h>

#include "rom_device.hpp"

namespace bg {

// The argument tail of the four loops, after the full loop's own block (whose x, u0 and basis are the table's)
struct HyperTableArgs {
    const int32_t* node;    // [nodes] ascending mesh nodes of the table
    const int32_t* pos;     // [nrows] table position of every sampled row
    const double* xi;       // [nrows] weights
    const double* q0;       // [B][n]
};
// ... of the three closure loops: their N stays the mesh's node count (it decides the last row), hist is qhist [B][nsteps+1][n]
struct HyperClosureTableArgs : HyperTableArgs {
    double* qshist;         // [B][nsteps+1][nbar]
    int nodes, nrows;       // table nodes, sampled rows
};

// s_smp[k] = 1 + the sampled row at table node k, or 0, for k < npad (npad >= nodes).  A barrier after either loop.
template <int NT>
__device__ __forceinline__ void hyper_scatter_rows(int* s_smp, int npad, const int32_t* pos, int nrows, int nodes, int tid)
{
    for (int k = tid; k < npad; k += NT) s_smp[k] = 0;
    __syncthreads();
    for (int j = tid; j < nrows; j += NT) {
        const int p = pos[j];
        if ((unsigned)p < (unsigned)nodes) s_smp[p] = j + 1;
    }
    __syncthreads();
}

// Table node k with j = s_smp[k]: its mesh row (meshN: only a neighbour, or beyond the table -- an identity row) and its
// weight factor.
template <bool GAL>
__device__ __forceinline__ void hyper_table_node(int j, int k, const int32_t* node, const double* xi, int meshN, int nodes,
                                                 int& row, double& mul)
{
    const int ir = j ? node[k] : meshN;
    // (a sampled row whose neighbour the table does not hold -- not a table the contract allows -- is left out)
    if ((unsigned)ir >= (unsigned)meshN || (ir > 0 && k == 0) || (ir < meshN - 1 && k == nodes - 1)) j = 0;
    const double w = j ? xi[j - 1] : 0.0;
    row = j ? ir : meshN;
    mul = GAL ? w : sqrt(w);
}

// Weighted row of table node i as mesh row ir (hyper_table_node) with weight factor wm: the table coordinates x as the
// x[ir - 1], x[ir], x[ir + 1] of the row routine, the weight in the coefficients.  um, uc, ur: u at the table nodes i - 1, i,
// i + 1.  g, hL, hR: M u^n + dt F at i and the SUPG loads of the elements on either side; the row routine reads them only
// where the row has the term (g: ir < meshN, hL: also ir > 0, hR: also ir < meshN - 1), so a caller may guard its reads so.
// wm is read after the row is formed (by value, ahead of it, the wide POD-ANN kernels spilled more).
__device__ __forceinline__ void hyper_assemble_row(int i, int ir, int meshN, const double& wm, double um, double uc, double ur,
                                                   double g, double hL, double hR, double mu1, const MeshConst& mc, const double* x,
                                                   double dt, double E, double& lo, double& di, double& up, double& R)
{
    rom_assemble_row(ir, meshN, um, uc, ur, g, hL, hR, mu1, mc, 1, x + (ir < meshN ? i - ir : 0), dt, E, lo, di, up, R);
    lo = wm * lo; di = wm * di; up = wm * up; R = wm * R;
}

// ... of every table node into s_coef (lower, diagonal, upper, residual), the map in LDS; the loop is kept rolled
template <int NPAD, int NT>
__device__ __forceinline__ void hyper_assemble_rows(double (*s_coef)[4], const int* s_hnode, const double* s_hmul, const double* s_u,
                                                    const double* s_g, const double* s_h, const double* x, int meshN, double h,
                                                    double dt, double E, int supg, double mu1, int tid)
{
#pragma unroll 1
    for (int i = tid; i < NPAD; i += NT) {
        const int ir = s_hnode[i];
        double lo, di, up, R;
        const bool in = ir < meshN;
        const MeshConst mc = make_mesh_const(h, dt, E, supg);
        hyper_assemble_row(i, ir, meshN, s_hmul[i], s_u[i + 1], s_u[i + 2], s_u[i + 3], in ? s_g[i] : 0.0,
                           (in && ir > 0) ? s_h[i - 1] : 0.0, (in && ir < meshN - 1) ? s_h[i] : 0.0, mu1, mc, x, dt, E, lo, di, up, R);
        s_coef[i][0] = lo; s_coef[i][1] = di; s_coef[i][2] = up; s_coef[i][3] = R;
    }
}

// Start of sample smp: q_p = q0 into s_q (zero from n, RW entries) and row 0 of the sample's qhist, a zero row 0 of its
// qshist.  Here and in hyper_write_step qhist is the sample's block (the kernels' `hist`), q0 and qshist are the whole
// arrays: the addresses are formed where the kernels formed them.  `zero` is 0.0, handed in by the kernel that wants it opaque.
template <int NT, int RW>
__device__ __forceinline__ void hyper_sample_start(const double* q0, double* s_q, double* qhist, double* qshist, int smp, int nsteps,
                                                   int n, int nbar, int tid, double zero)
{
    if (tid < RW) {
        const double q = tid < n ? q0[(size_t)smp * n + tid] : zero;
        s_q[tid] = q;
        if (tid < n) qhist[tid] = q;
    }
    for (int j = tid; j < nbar; j += NT) qshist[(size_t)smp * (size_t)(nsteps + 1) * (size_t)nbar + j] = zero;
}

// The outputs of step `step` of sample smp: q_p = s_q into row step + 1 of the sample's qhist, the closure value of the step's
// decode, q_s[j] = s_f[FS j], into that row of its qshist (FS > 1: the narrow POD-ANN loop reads it from a column of s_dN)
template <int NT, int FS = 1>
__device__ __forceinline__ void hyper_write_step(double* qhist, double* qshist, int smp, int nsteps, int step, const double* s_q,
                                                 const double* s_f, int n, int nbar, int tid)
{
    if (tid < n) qhist[(size_t)(step + 1) * n + tid] = s_q[tid];
    double* qs = qshist + ((size_t)smp * (size_t)(nsteps + 1) + (size_t)(step + 1)) * (size_t)nbar;
    for (int j = tid; j < nbar; j += NT) qs[j] = s_f[FS * j];
}

}  // namespace bg
