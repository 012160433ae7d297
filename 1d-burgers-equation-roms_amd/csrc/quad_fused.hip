// quad_fused.hip -- bg_quad_rom_run: the quadratic-manifold PROM time loop of quad_device.hpp (read its header first) for
// meshes of up to 512 nodes.  u, g = M u^n + dt F and dt F of the workgroup's four samples are kept in LDS (3 x 16 KB)
// beside the 95 KB ring of tangent rows: 154 KB of the compute unit's 160.
#include "quad_device.hpp"

namespace {

using namespace bg;

constexpr int QNMAX = 512;             // mesh rows
#ifndef BG_QUAD_WINDOW
#define BG_QUAD_WINDOW 14
#endif

// [sample][row], in LDS.  At file scope: the kernel is a template of quad_device.hpp, and a description cannot declare
// __shared__ arrays inside it; each kernel that uses them gets its own allocation.
__shared__ __attribute__((aligned(16))) double s_g[QG][QNMAX];             // M u^n + dt F
__shared__ __attribute__((aligned(16))) double s_fdt[QG][QNMAX];           // dt F

struct QuadFused {
    using Args = QuadRunArgs;
    static constexpr bool hyper = false;
    static constexpr int rows = QNMAX;
    static constexpr int window = BG_QUAD_WINDOW;

    // wave w of group grp takes order[4 grp + w]; a padding wave (beyond B) computes on a copy of the last sample
    static __device__ __forceinline__ bool pick_sample(const QuadRunArgs& a, int grp, int w, bool& valid, int& sb)
    {
        const int slot = grp * QG + w;
        valid = slot < a.B;
        const int slotc = valid ? slot : a.B - 1;
        sb = a.order ? a.order[slotc] : slotc;
        return true;
    }

    struct Nodes {                      // s_g, s_fdt
        static constexpr bool staged = false;
        __device__ __forceinline__ void put_fdt(double*, int w, int i, double v) { s_fdt[w][i] = v; }
        __device__ __forceinline__ void init(int, double) {}
        __device__ __forceinline__ double fdt(int w, int i, int) const { return s_fdt[w][i]; }
        __device__ __forceinline__ void set_g(int w, int i, int, double v) { s_g[w][i] = v; }
        __device__ __forceinline__ double g(int w, int i, int N, int) const { return (i < N) ? s_g[w][i] : 0.0; }
    };
};

}  // namespace

extern "C" {

// Largest n and N of bg_quad_rom_run.
int bg_quad_rom_max_n(void) { return QN; }

// Element counts of the two operand copies bg_quad_rom_run reads (the caller builds them once per basis).
long long bg_quad_rom_h3f_elems(int N) { return N < 2 ? 0 : (long long)((N + 3) / 4) * QP2 * 64 * 2; }
long long bg_quad_rom_phif_elems(int N) { return N < 2 ? 0 : (long long)((N + 3) / 4) * QNB * 16; }

int bg_quad_rom_run(int N, int B, int n, int nsteps, int projection, const double* x, const double* PhiT, const double* Phif,
                    const double* H3f, const double* u0, const double* mu1, const double* mu2, double dt, double E, double tol,
                    int max_it, int options, double* hist, int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order,
                    void* stream)
{
    if (N < 2 || B < 0 || n < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > QNMAX) return BG_ERR_UNSUPPORTED_N;
    if (n > QN) return BG_ERR_UNSUPPORTED_R;
    if (B == 0) return BG_OK;
    if (!x || !PhiT || !Phif || !H3f || !u0 || !mu1 || !mu2 || !hist || !flags || !info || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    return quad_rom_launch<QuadFused>(N, B, n, nsteps, projection, x, PhiT, Phif, H3f, u0, mu1, mu2, dt, E, tol, max_it, options, hist, iters,
                                 flags, info, order, stream);
}

}  // extern "C"
