// quad_hyper.hip -- bg_hyper_quad_rom_run: the HYPER-REDUCED quadratic-manifold PROM time loop.  Both projections of
// pod_quadratic_manifold (reference FEM/fem_burgers.py:1081-1175) are assembled from m sampled mesh rows with weights
// xi >= 0,  Ar = sum_j xi_j w_j^T y_j,  br = sum_j xi_j w_j^T R_j  with T = Phi + H dQ/dq, y_j = (A T)[i_j] and w_j = T[i_j]
// (Galerkin) or y_j (LSPG), so a pass streams the H3 rows of the at most 3 m stencil nodes of those rows whatever the
// mesh, and the kernel never touches a vector of mesh length.
//
// The loop is quad_device.hpp's own body (read its header first; rom_hyper_table_device.hpp describes the hyper-reduced
// form) on the compacted mesh of the stencil nodes: tangent stream, decode, projection, the pivoted solve and the stopping
// test are unchanged.  This file keeps the two descriptions and the entry points:
//   nodes <= 512   per-node arrays g, dt F in LDS as bg_quad_rom_run holds them; mesh row and factor of the table nodes
//                  (12 B per node) in the 8 KB that layout leaves free: 161 840 B of the compute unit's 163 840
//   nodes <= 768   g, dt F in the owning wave's registers as bg_quad_rom_run_long holds them (12 doubles each)
#include "quad_device.hpp"

namespace {

using namespace bg;

constexpr int HQ_MAX_ROWS = 256;               // sampled rows
constexpr int HQ_MAX_NODES = 3 * HQ_MAX_ROWS;  // table nodes: every sampling of HQ_MAX_ROWS rows runs
constexpr int HQ_SHORT = 512;                  // table nodes of the first description
#ifndef BG_QUAD_HYPER_WINDOW
#define BG_QUAD_HYPER_WINDOW 14
#endif

// At file scope, as quad_fused.hip's: a description cannot declare __shared__ arrays inside the kernel template, and each
// kernel gets an allocation of the arrays it names only.
__shared__ __attribute__((aligned(16))) double s_g[QG][HQ_SHORT];          // M u^n + dt F
__shared__ __attribute__((aligned(16))) double s_fdt[QG][HQ_SHORT];        // dt F
__shared__ double s_mul_short[HQ_SHORT], s_mul_long[HQ_MAX_NODES];         // xi | sqrt(xi) of the row at a table node
__shared__ int s_row_short[HQ_SHORT], s_row_long[HQ_MAX_NODES];            // its mesh row (meshN: none)

struct QuadHyperShort : QuadSkippingOrder {
    using Args = HyperQuadRunArgs;
    static constexpr bool hyper = true;
    static constexpr int rows = HQ_SHORT;
    static constexpr int window = BG_QUAD_HYPER_WINDOW;
    static __device__ __forceinline__ int& hyper_row(int k) { return s_row_short[k]; }
    static __device__ __forceinline__ double& hyper_mul(int k) { return s_mul_short[k]; }

    struct Nodes {                      // s_g, s_fdt
        static constexpr bool staged = false;
        __device__ __forceinline__ void put_fdt(double*, int w, int i, double v) { s_fdt[w][i] = v; }
        __device__ __forceinline__ void init(int, double) {}
        __device__ __forceinline__ double fdt(int w, int i, int) const { return s_fdt[w][i]; }
        __device__ __forceinline__ void set_g(int w, int i, int, double v) { s_g[w][i] = v; }
        __device__ __forceinline__ double g(int w, int i, int N, int) const { return (i < N) ? s_g[w][i] : 0.0; }
    };
};

struct QuadHyperLong : QuadSkippingOrder {
    using Args = HyperQuadRunArgs;
    static constexpr bool hyper = true;
    static constexpr int rows = HQ_MAX_NODES;
    static constexpr int window = BG_QUAD_HYPER_WINDOW;
    static __device__ __forceinline__ int& hyper_row(int k) { return s_row_long[k]; }
    static __device__ __forceinline__ double& hyper_mul(int k) { return s_mul_long[k]; }
    using Nodes = QuadRegisterNodes<rows>;
};

constexpr size_t hq_lds(int rows, bool nodes_in_lds)
{
    return sizeof(double) * (QG * QTJ + QG * (rows + 4) + QG * QRS * 4 + QG * QN + QG + (nodes_in_lds ? 2 * QG * rows : 0) + rows) +
           sizeof(int) * (QG + rows);
}
static_assert(hq_lds(HQ_SHORT, true) <= 160 * 1024 && hq_lds(HQ_MAX_NODES, false) <= 160 * 1024, "LDS per workgroup");
static_assert(QTJ >= HQ_MAX_NODES, "dt F is staged in the wave's tangent rows on its way into registers");

bool hq_covers(int nodes) { return nodes >= 1 && nodes <= HQ_MAX_NODES; }

}  // namespace

extern "C" {

int bg_hyper_quad_rom_limits(int* max_n, int* max_m, int* max_nodes)
{
    if (max_n) *max_n = QN;
    if (max_m) *max_m = HQ_MAX_ROWS;
    if (max_nodes) *max_nodes = HQ_MAX_NODES;
    return BG_OK;
}

// persistent workgroups per compute unit of the instantiation that runs a table of `nodes` nodes (0: no such table)
int bg_hyper_quad_rom_workgroups_per_cu(int nodes) { return hq_covers(nodes) ? 1 : 0; }

// Element counts of the two operand copies bg_hyper_quad_rom_run reads, for a table of `nodes` nodes; 0 outside 1 .. 768.
long long bg_hyper_quad_rom_phif_elems(int nodes) { return hq_covers(nodes) ? (long long)((nodes + 3) / 4) * QNB * 16 : 0; }
long long bg_hyper_quad_rom_h3f_elems(int nodes) { return hq_covers(nodes) ? (long long)((nodes + 3) / 4) * QP2 * 64 * 2 : 0; }

int bg_hyper_quad_rom_run(int N, int B, int n, int m, int nodes, int nsteps, int projection, const double* xn, const int32_t* node,
                          const int32_t* pos, const double* xi, const double* Phif, const double* H3f, const double* q0,
                          const double* u0n, const double* mu1, const double* mu2, double dt, double E, double tol, int max_it,
                          int options, double* qhist, int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order,
                          void* stream)
{
    (void)options;                                  // the table is a non-uniform mesh and this stepper has no SUPG term
    if (N < 3 || B < 0 || n < 1 || m < 1 || nodes < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > bg_fom_max_n()) return BG_ERR_UNSUPPORTED_N;
    if (n > QN || m > HQ_MAX_ROWS || nodes > HQ_MAX_NODES) return BG_ERR_UNSUPPORTED_R;
    if (m > N || nodes > N || nodes < m || nodes > 3 * m) return BG_ERR_BAD_ARG;
    if (B == 0) return BG_OK;
    if (!node || !xn || !pos || !xi || !Phif || !H3f || !q0 || !u0n || !mu1 || !mu2 || !qhist || !flags || !info ||
        (nsteps > 0 && !iters))
        return BG_ERR_BAD_ARG;
    if ((uintptr_t)H3f & 15) return BG_ERR_BAD_ARG;
    HyperQuadRunArgs a;
    a.x = xn; a.PhiT = nullptr; a.Phif = Phif; a.H3f = H3f; a.u0 = u0n; a.mu1 = mu1; a.mu2 = mu2; a.hist = qhist; a.iters = iters;
    a.flags = flags; a.info = info; a.order = order; a.dt = dt; a.E = E; a.tol = tol; a.N = nodes; a.NPAD = ((nodes + 63) / 64) * 64;
    a.NG = (nodes + 3) / 4; a.B = B; a.n = n; a.nsteps = nsteps; a.max_it = max_it; a.nonuniform = 1;
    a.node = node; a.pos = pos; a.xi = xi; a.q0 = q0; a.meshN = N; a.nrows = m;
    return nodes <= HQ_SHORT ? quad_rom_dispatch<QuadHyperShort>(a, projection, stream)
                             : quad_rom_dispatch<QuadHyperLong>(a, projection, stream);
}

}  // extern "C"
