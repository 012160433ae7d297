// rom_long_device.hpp -- what the two LDS-streaming loops for LONG meshes (513 <= N <= 1024, up to 40 modes) share:
// bg_rom_run_long (rom_long.hip, POD) and bg_local_rom_run_long (rom_local_long.hip, local POD).  The loop itself is
// rom_stream_device.hpp's; here are the layout constants, the part of the description K both use (LongLayout: the reduced
// system parked WHOLE in LDS over the dead slabs and solved by rom_fused_device.hpp's routines) and the kernel body with
// its LDS arrays (BG_LONG_KERNEL_BODY).  The hyper-reduced loop (rom_hyper.hip) has a body of its own over the same
// LongLayout: its items, parking and solve are these.
// LDS: 8 B per mesh row for each of u, g, h_f, dt F (32 KB at 1024 rows), the coefficients of ONE slab (2 KB), two slabs
// of 66 x 42 doubles (43.3 KB) -- 77.7 KB, so two workgroups share a compute unit (local POD: + 64 doubles for q_g).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rom_fused_device.hpp"
#include "rom_stream_device.hpp"

namespace bg {

constexpr int LNMAX = 1024;            // mesh rows
constexpr int LR = 40;                 // padded reduced dimension: column 10 t + c  <->  (lane index t, block c)
constexpr int LNB = 10;                // 4-column blocks
constexpr int LPS = 42;                // doubles per row of the LDS slabs (16-byte aligned rows)
constexpr int LSW = LR + 4;            // doubles per row of the parked system: Ar | br | Phi^T u
#ifndef BG_LONG_WG_PER_CU
#define BG_LONG_WG_PER_CU 2
#endif
constexpr int LWG_PER_CU = BG_LONG_WG_PER_CU;

struct LongLayout {
    static constexpr int NB = LNB, PS = LPS, SW = LSW, NMAX = LNMAX;
    static constexpr bool cf_by_mesh_row = false;       // lo, di, up, R of the slab at hand only: 2 KB instead of 32
    static constexpr bool mirror_lspg = true;           // the solves read the system through a plain accessor
    static constexpr bool has_repair = true;

    // solve(Ar, -br) (:767) by rom_fused_device.hpp's routines, one value of dq and q per lane.  BG_OPT_FORCE_PIVOTED: the
    // entry point skips the fast launch and the repair kernel takes every sample.
    // r: the live unknowns of this step.  Both solves put a unit diagonal and a zero right-hand side on the unknowns at and
    // beyond r (coop_gj_solve_of, pivoted_solve_of), so their correction is exactly zero and q is zero there: what local POD
    // needs when the step's cluster is narrower than the padded 40.
    // solve_add: q = base + dq into L.q, |dq|^2 and |q|^2; `base` is this lane's value (0 at and beyond r), read by the caller
    // before the solve's first barrier.  The streaming loops add dq to the parked Phi^T u (solve_update), the hyper-reduced
    // loop (rom_hyper.hip) to q itself.
    template <bool PIV, int W>
    static __device__ __forceinline__ void solve_add(const StreamLds& L, int r, int lane, double base, bool& aborted, int& info_out,
                                                     double& nd, double& nq)
    {
        const double* S = L.slab;
        auto entry = [&](int i, int j) -> double { return S[i * LSW + j]; };      // (Ar | br)[i][j]
        double xout;
        if constexpr (PIV) {
            if (W == 0) fused::pivoted_solve_of<LNB>(entry, L.x, &L.bad[4], lane, r);
            __syncthreads();
            xout = (lane < LR) ? L.x[lane] : 0.0;
            if (L.bad[4] != 0 && info_out == 0) info_out = L.bad[4];
        } else {
            bool tripped;
            xout = fused::coop_gj_solve_of<LNB>(entry, reinterpret_cast<double (*)[4][64]>(L.m), L.diag, L.y, L.bad, W, lane, r, tripped);
            if (tripped) aborted = true;
        }
        const double dq = (lane < r) ? xout : 0.0;
        const double qn = base + dq;
        wave_sum2(dq * dq, qn * qn, nd, nq);
        if (W == 0 && lane < LR) L.q[lane] = qn;
    }

    template <bool GAL, bool PIV, int W, class Lap>
    static __device__ __forceinline__ void solve_update(const StreamRunArgs&, const StreamLds& L, int r, int lane, bool& aborted,
                                                        int& info_out, double& nd, double& nq, const Lap&)
    {
        const double wtu = (lane < r) ? L.slab[lane * LSW + LR + 1] : 0.0;       // Phi^T u
        solve_add<PIV, W>(L, r, lane, wtu, aborted, info_out, nd, nq);
    }
};

// The body of both kernels: the LDS arrays and the four-way branch on the wave, for the description K, the kernel's template
// parameters GAL and PIV and its argument `a`.  QG: doubles of q_g in LDS (local POD), else 0.  A macro, so that the arrays
// are declared in the kernel itself: declared in a device function that both kernels call, the same arrays changed the
// register allocation of the POD kernels (193 -> 189 spilled SGPRs), and those are meant to stay what they were.
#define BG_LONG_KERNEL_BODY(K, QG)                                                                                                  \
    constexpr int SLAB = StreamDims<K>::SLAB;                                                                                       \
    __shared__ __attribute__((aligned(16))) double s_slab[2 * SLAB];              /* two slab buffers; later the system */          \
    __shared__ __attribute__((aligned(16))) double s_u[LNMAX + 4];                /* u at offset 2, zero halo on each side */       \
    __shared__ double s_g[LNMAX], s_h[LNMAX], s_fdt[LNMAX];                                                                         \
    __shared__ __attribute__((aligned(16))) double s_cf[SRS][4];                  /* lo, di, up, R per row of the slab */           \
    __shared__ __attribute__((aligned(16))) double s_q[LR];                                                                         \
    __shared__ int s_bad[8];                                                      /* [4] guard of each wave, [4] info of the pivoted solve */ \
    __shared__ double s_qg[(QG) > 0 ? (QG) : 1];                                  /* (unused, and dropped, when QG = 0) */          \
    static_assert(sizeof(double) * (2 * SLAB + LNMAX + 4 + 3 * LNMAX + 4 * SRS + LR + (QG)) + 32 <= 160 * 1024 / LWG_PER_CU,        \
                  "LDS per workgroup");                                                                                             \
    /* over the dead slabs: the system [LR][LSW], then the multipliers of two panels, the diagonal, y and x */                      \
    double* const s_m = s_slab + LR * LSW;                                                                                          \
    double* const s_diag = s_m + 512;                                                                                               \
    static_assert(LR * LSW + 512 + 3 * 64 <= 2 * SLAB, "the solve's arrays fit over the slabs");                                    \
    rom_stream_waves<K, GAL, PIV>(a, StreamLds{s_slab, s_u, s_g, s_h, s_fdt, s_cf, s_q, s_m, s_diag, s_diag + 64, s_diag + 128,     \
                                               s_bad, (QG) > 0 ? s_qg : nullptr})

}  // namespace bg
