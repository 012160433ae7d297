// quad_long.hip -- bg_quad_rom_run_long: the quadratic-manifold PROM time loop of quad_device.hpp (read its header first)
// for LONG meshes, 513 <= N <= 1024, n <= 40.  reference: FEMBurgers.pod_quadratic_manifold, FEM/fem_burgers.py:1081-1175.
//
// What differs from bg_quad_rom_run is where the per-node arrays live.  quad_fused.hip keeps u, g = M u^n + dt F and dt F of its four samples in LDS (3 x 16 KB at 512 rows) beside the 95 KB ring of tangent rows: 154 KB.  At 1024 rows that would be 203 KB, beyond
// the compute unit's 160 KB.  A wave owns its sample, the assembly of slab s reads g at row 64 s + lane and the step
// start forms g at rows lane + 64 m: the SAME lane holds a row in both places.  So g and dt F stay in the owning wave's
// registers, 16 doubles per lane each; the assembly picks g[slab] with a chain of selects on the wave-uniform slab
// number (32 v_cndmask per slab).  Only u (which neighbours and the tangent stream's lanes touch) stays in LDS.
// LDS: tangent ring 96 896 B + u 32 896 B + coefficients of one slab 8 192 B + q, flags: 139 KB.
// Further differences: order entries outside [0, B) are skipped (a group with no valid entry costs nothing, a wave
// without one computes on a copy of sample 0 and stores nothing); N <= 512 is refused (bg_quad_rom_run covers it).
#include "quad_device.hpp"

namespace {

using namespace bg;

constexpr int QNMAX = 1024;            // mesh rows
constexpr int QNMIN = 513;             // below: bg_quad_rom_run
#ifndef BG_QUAD_LONG_WINDOW
#define BG_QUAD_LONG_WINDOW 14
#endif

struct QuadLong : QuadSkippingOrder {       // pick_sample: order entries outside [0, B) are skipped
    using Args = QuadRunArgs;
    static constexpr bool hyper = false;
    static constexpr int rows = QNMAX;
    static constexpr int window = BG_QUAD_LONG_WINDOW;
    using Nodes = QuadRegisterNodes<rows>;  // both arrays in the owning wave's registers
};

static_assert(sizeof(double) * (QG * QTJ + QG * (QNMAX + 4) + QG * QRS * 4 + QG * QN + QG) + sizeof(int) * QG <= 160 * 1024, "LDS per workgroup");
static_assert(QTJ >= QNMAX, "dt F is staged in the wave's tangent rows on its way into registers");

bool quad_long_covers(int N) { return N >= QNMIN && N <= QNMAX; }

}  // namespace

extern "C" {

int bg_quad_rom_run_long_max_n(void) { return QNMAX; }
int bg_quad_rom_run_long_max_r(void) { return QN; }
int bg_quad_rom_run_long_workgroups_per_cu(void) { return 1; }

// Element counts of the three operand copies bg_quad_rom_run_long reads (the caller builds them once per basis); 0 outside 513 .. 1024.
long long bg_quad_rom_run_long_phit_elems(int N) { return quad_long_covers(N) ? (long long)QN * (((N + 63) / 64) * 64) : 0; }
long long bg_quad_rom_run_long_phif_elems(int N) { return quad_long_covers(N) ? (long long)((N + 3) / 4) * QNB * 16 : 0; }
long long bg_quad_rom_run_long_h3f_elems(int N) { return quad_long_covers(N) ? (long long)((N + 3) / 4) * QP2 * 64 * 2 : 0; }

int bg_quad_rom_run_long(int N, int B, int n, int nsteps, int projection, const double* x, const double* PhiT, const double* Phif,
                         const double* H3f, const double* u0, const double* mu1, const double* mu2, double dt, double E, double tol,
                         int max_it, int options, double* hist, int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order,
                         void* stream)
{
    if (N < 3 || B < 0 || n < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (!quad_long_covers(N)) return BG_ERR_UNSUPPORTED_N;
    if (n > QN) return BG_ERR_UNSUPPORTED_R;
    if (B == 0) return BG_OK;
    if (!x || !PhiT || !Phif || !H3f || !u0 || !mu1 || !mu2 || !hist || !flags || !info || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    if (((uintptr_t)H3f | (uintptr_t)PhiT) & 15) return BG_ERR_BAD_ARG;
    return quad_rom_launch<QuadLong>(N, B, n, nsteps, projection, x, PhiT, Phif, H3f, u0, mu1, mu2, dt, E, tol, max_it, options, hist, iters,
                                 flags, info, order, stream);
}

}  // extern "C"
