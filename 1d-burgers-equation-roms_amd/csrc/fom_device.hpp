// fom_device.hpp -- building blocks of the Burgers FOM Picard iteration.
//
// Row distribution: thread p of a sample's threads owns the R consecutive mesh rows
// [p*R, p*R+R); rows >= N are identity rows.  All per-row state lives in registers (fully
// unrolled, compile-time R).  The forcing set-up, the mass right-hand side and the assembly are
// written over a topology (fom_wide.hpp: one wavefront or one workgroup per sample) that supplies
// the neighbours' values; the PCR and the tridiagonal solve below them are the one-wavefront form
// (N <= 64*R), which the workgroup form of fom_wide.hpp builds on.
//
// Arithmetic restated from the reference (FEM/fem_burgers.py), closed form for
// 2-node elements on a uniform mesh:
//   convection  :389-425   c1 = (2ul+ur)/6, c2 = (ul+2ur)/6
//   forcing     :427-461   2-pt Gauss of 0.02*exp(mu2 x)
//   SUPG        :500-581   s_e = tau*(ubar*du - (f1+f2)/2), tau = 0.5h/(2 max(|ubar|,1e-10))
//   system      :676-689   A = M + dt C + dt E K, row 0 <- e0, b = M u^n + dt F - dt S, b0 = mu1
#pragma once
#include "wave_ops.hpp"

// reciprocal used inside the Picard iteration (see wave_ops.hpp: rcp = 2 Newton steps, rcp1 = 1)
#ifndef BG_RCP
#define BG_RCP rcp1
#endif

// pcr64 ends after the stride-8 step once every coupling of the wave is below rounding (see pcr64); 0: always six steps
#ifndef BG_PCR_EARLY_EXIT
#define BG_PCR_EARLY_EXIT 1
#endif

// pcr64 closes the interface system by Jacobi sweeps after its stride-1 step once every coupling of the wave is small
// enough for six of them (see pcr64); 0: every wave goes on to the stride-2 step, the listing before the sweeps
#ifndef BG_PCR_JACOBI_EXIT
#define BG_PCR_JACOBI_EXIT 1
#endif
// fewest rows per lane at which that exit is compiled in (1: everywhere)
#ifndef BG_PCR_JACOBI_MIN_ROWS
#define BG_PCR_JACOBI_MIN_ROWS 12
#endif

// where the caller asks for it (pcr64<ROWS, true>), pcr64 closes an interface system that couples upwards only by six
// one-sided sweeps and one fold of the lower coupling (see pcr64_onesided); 0: the listing before that route
#ifndef BG_PCR_ONESIDED_EXIT
#define BG_PCR_ONESIDED_EXIT 1
#endif

// fom_sample forms the off-diagonals and SUPG terms of the NEXT iterate in front of the stopping test, where one wave per
// sample has nothing else to issue between the dependent rounds of the norm reduction (see fom_sample; topologies with
// rotates_picard only); 0: every iteration starts with them, the listing of the loop before the rotation
#ifndef BG_PICARD_ROTATE
#define BG_PICARD_ROTATE 1
#endif

// fom_sample starts every time step with lean iterations, which solve for the new iterate itself, A v = b, and not for the
// increment, A du = b - A u, and stays with them while the stopping test is missed by more than a factor of
// BG_PICARD_LEAN_FACTOR (see assemble_p2 and fom_sample); 0: every iteration solves for the increment
#ifndef BG_PICARD_LEAN
#define BG_PICARD_LEAN 1
#endif
#ifndef BG_PICARD_LEAN_FACTOR
#define BG_PICARD_LEAN_FACTOR 16.0
#endif

namespace bg {

constexpr double GP_A = 0.78867513459481287;  // (1 + 1/sqrt(3)) / 2
constexpr double GP_B = 0.21132486540518713;  // (1 - 1/sqrt(3)) / 2

struct MeshConst {
    double h;      // uniform element length
    double aoff;   // h/6 - dt*E/h     (off-diagonal base)
    double dd2;    // 2*(h/3 + dt*E/h) (interior diagonal base)
    double dd1;    // h/3 + dt*E/h     (last-row diagonal base)
    double dt6;    // dt/6
    double kap;    // 0.25*dt  (0 when SUPG is off)
    double h6;     // h/6
};

__device__ __forceinline__ MeshConst make_mesh_const(double h, double dt, double E, int supg)
{
    MeshConst c;
    c.h = h;
    double eh = dt * E / h;
    c.aoff = h / 6.0 - eh;
    c.dd1 = h / 3.0 + eh;
    c.dd2 = 2.0 * c.dd1;
    c.dt6 = dt / 6.0;
    c.kap = supg ? 0.25 * dt : 0.0;
    c.h6 = h / 6.0;
    return c;
}

// Per-sample constants: hfs[j] = h*(f(gp1)+f(gp2)) of the element to the right of local
// row j, and fdt[j] = dt*F_i of row i = row0+j.
template <int R>
__device__ __forceinline__ void forcing_setup(const double* __restrict__ x, int N, int row0, double mu2,
                                              double h, double dt, double (&hfs)[R], double (&fdt)[R])
{
    double frPrev = 0.0;   // right-node load of element row0-1
    {
        int e = row0 - 1;
        if (e >= 0 && e < N - 1) {
            double xl = x[e], xr = x[e + 1];
            double f1 = 0.02 * exp(mu2 * (GP_A * xl + GP_B * xr));
            double f2 = 0.02 * exp(mu2 * (GP_B * xl + GP_A * xr));
            frPrev = (f1 * GP_B + f2 * GP_A) * (0.5 * h);
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        int e = row0 + j;
        double fl = 0.0, fr = 0.0, fs = 0.0;
        if (e < N - 1) {
            double xl = x[e], xr = x[e + 1];
            double f1 = 0.02 * exp(mu2 * (GP_A * xl + GP_B * xr));
            double f2 = 0.02 * exp(mu2 * (GP_B * xl + GP_A * xr));
            fl = (f1 * GP_A + f2 * GP_B) * (0.5 * h);
            fr = (f1 * GP_B + f2 * GP_A) * (0.5 * h);
            fs = f1 + f2;
        }
        hfs[j] = h * fs;
        fdt[j] = (e < N) ? dt * (frPrev + fl) : 0.0;
        frPrev = fr;
    }
}

// Everything from here to the PCR is written over a topology `tp` (WaveTopo / WgTopo, fom_wide.hpp): tp.g is this thread's
// index among the sample's threads, its rows are [tp.g*R, tp.g*R + R), and tp hands over the neighbours' values: uL / uR,
// u of the row below this thread's first row / above its last row (0 outside the mesh), and seL, se of the element below.
//
// g = M u^n + dt F  (constant over the Picard iterations of one time step).
// gstore(j, value): where row j of g goes (registers, or LDS when a kernel parks it there)
template <int R, bool FULL, class Topo, typename GStore>
__device__ __forceinline__ void mass_rhs(Topo& tp, const MeshConst& c, int N, const double (&u)[R],
                                         const double (&fdt)[R], GStore&& gstore)
{
    double uL, uR;
    tp.halo(u[0], u[R - 1], uL, uR);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const double um = (j == 0) ? uL : u[j - 1];
        const double up = (j == R - 1) ? uR : u[j + 1];
        const int i = tp.g * R + j;
        double m = __builtin_fma(4.0, u[j], um) + up;
        // the last real row has no right element; with FULL it can only be row R-1 of the last thread (as in assemble_p2)
        if (FULL ? (j == R - 1) : true) {
            const bool is_last = FULL ? tp.last() : (i == N - 1);
            m = is_last ? __builtin_fma(2.0, u[j], um) : m;
        }
        double v = __builtin_fma(c.h6, m, fdt[j]);
        gstore(j, (!FULL && i >= N) ? 0.0 : v);
    }
    tp.halo_done();
}

// SUPG element terms se[j] = t[j] / mx[j], mx[j] = max(|w_j|, 2e-10) >= 2e-10.  The R quotients of a thread do not depend on one
// another, so every full group of four shares ONE reciprocal (v_rcp_f64 is quarter rate: 16.4 cycles against 4.3 for a
// multiply) through a product tree:
//   r = 1 / (m0 m1 m2 m3),  r01 = r (m2 m3) = 1 / (m0 m1),  r23 = r (m0 m1),  1/m0 = r01 m1,  1/m1 = r01 m0,  ...
// 16 instructions per group, as many as four rcp1 with their multiplies, three of them no longer reciprocals.  The R % 4
// elements left over keep t * rcp1(mx).  Four roundings on top of rcp1's 2.1e-15: under 2.6e-15 relative.
// Range: the product of a group must stay finite, which every mx <= 1e77 (|u| <~ 5e76) guarantees; it cannot underflow
// (>= 1.6e-39).  Past that the group's reciprocal is 0, its Newton step NaN, and the sample ends flagged
// BG_FLAG_NONFINITE like any other non-finite state (include/burgers_hip.h, bg_fom_run).
template <int R>
__device__ __forceinline__ void supg_terms(const double (&mx)[R], const double (&t)[R], double (&se)[R])
{
    constexpr int G = R / 4 * 4;
#pragma unroll
    for (int j = 0; j < G; j += 4) {
        const double p01 = mx[j] * mx[j + 1], p23 = mx[j + 2] * mx[j + 3];
        const double r = BG_RCP(p01 * p23);
        const double r01 = r * p23, r23 = r * p01;
        se[j] = t[j] * (r01 * mx[j + 1]);
        se[j + 1] = t[j + 1] * (r01 * mx[j]);
        se[j + 2] = t[j + 2] * (r23 * mx[j + 3]);
        se[j + 3] = t[j + 3] * (r23 * mx[j + 2]);
    }
#pragma unroll
    for (int j = G; j < R; ++j) se[j] = t[j] * BG_RCP(mx[j]);
}

// One assembly: diagonals lo/di/up of A(u) and the right-hand side, in two halves around the exchange of se.
// p1: off-diagonals and the SUPG element terms se[];  p2: diagonal, right-hand side, special rows.
// `first` / `last_lane` mark the threads that own global row 0 / (FULL only) the last row.
// ITER chooses the right-hand side at compile time.  The matrix is the same, bit for bit, so every exit of pcr64, whose
// ballots read the couplings only, goes the way it went.
//   false  rhs = b - A u (= -R of the reference): the solve gives the increment.  The diagnostic assembly (bg_fom_assemble)
//          and the iterations of fom_sample near convergence.
//   true   rhs = b: the solve gives the new iterate itself, A v = b, and the three FMAs per row of A u are not issued.  b is
//          mu1 on the Dirichlet row, has no right element on the last row and is 0 on a padded row, whose solution is then
//          0, as u is there.  The lean iterations of fom_sample, far from convergence (fom.hip).
// What a lean solve costs: the solve's errors are relative to what it solves for.  The exits of pcr64 truncate by half an
// ulp of the largest interface unknown, the Wang sweeps round at the size of their unknowns and rcp1 is 2.1e-15 off: that
// is 1e-15 |u| to 1e-14 |u| per solve for the iterate, where for the increment it is the same fraction of |du|, which
// shrinks with the iteration.  A lean iteration is therefore as accurate as the pivot-free solve and not corrected below
// that by the next one, and the du = v - u of its stopping test carries the same absolute error, to be compared with the
// tol |u| = 1e-6 |u| it is tested against.  A time step that ENDED on a lean iteration would carry 1e-15 to 1e-14 into the
// history, where the increment form leaves 1e-16: over the 500 steps of tests/test_fom_gpu.py's committed N = 512 run that
// moved the wave and the workgroup form 3e-12 max|u| apart, against the 1e-12 the suite allows them.  So
// fom_sample goes lean only far from convergence, and a step's last iterations solve for the increment.
template <int R, typename HF>
__device__ __forceinline__ void assemble_p1(const MeshConst& c, const double (&u)[R], double uL, double uR,
                                            HF&& hf, double (&lo)[R], double (&up)[R], double (&se)[R])
{
    double mx[R], t[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const double ur = (j == R - 1) ? uR : u[j + 1];
        const double w = u[j] + ur;
        const double dif = ur - u[j];
        up[j] = __builtin_fma(c.dt6, w + u[j], c.aoff);
        if (j + 1 < R) lo[j + 1] = __builtin_fma(-c.dt6, w + ur, c.aoff);
        mx[j] = fmax(fabs(w), 2.0e-10);
        t[j] = __builtin_fma(w, dif, -hf(j));
    }
    supg_terms<R>(mx, t, se);
    lo[0] = __builtin_fma(-c.dt6, __builtin_fma(2.0, u[0], uL), c.aoff);
}

// Elements [J0, J1) of assemble_p1 alone, for a caller that places other work between the chunks (fom_sample weaves the
// norm reduction in): one group of four of supg_terms (J0 a multiple of four, J1 = J0 + 4 <= R), or the R % 4 elements left
// over (J1 = R).  The arithmetic of every element is assemble_p1's and supg_terms'; lo[0] stays with the caller.
template <int R, int J0, int J1, typename HF>
__device__ __forceinline__ void assemble_p1_rows(const MeshConst& c, const double (&u)[R], double uR, HF&& hf,
                                                 double (&lo)[R], double (&up)[R], double (&se)[R])
{
    constexpr int G = R / 4 * 4;
    static_assert(J0 % 4 == 0 && J0 < J1 && J1 <= R && (J0 < G ? J1 == J0 + 4 : J1 == R), "one supg group or the remainder");
    double mx[4], t[4];
#pragma unroll
    for (int j = J0; j < J1; ++j) {
        const double ur = (j == R - 1) ? uR : u[j + 1];
        const double w = u[j] + ur;
        const double dif = ur - u[j];
        up[j] = __builtin_fma(c.dt6, w + u[j], c.aoff);
        if (j + 1 < R) lo[j + 1] = __builtin_fma(-c.dt6, w + ur, c.aoff);
        mx[j - J0] = fmax(fabs(w), 2.0e-10);
        t[j - J0] = __builtin_fma(w, dif, -hf(j));
    }
    if constexpr (J0 < G) {
        const double p01 = mx[0] * mx[1], p23 = mx[2] * mx[3];
        const double r = BG_RCP(p01 * p23);
        const double r01 = r * p23, r23 = r * p01;
        se[J0] = t[0] * (r01 * mx[1]);
        se[J0 + 1] = t[1] * (r01 * mx[0]);
        se[J0 + 2] = t[2] * (r23 * mx[3]);
        se[J0 + 3] = t[3] * (r23 * mx[2]);
    } else {
#pragma unroll
        for (int j = J0; j < J1; ++j) se[j] = t[j - J0] * BG_RCP(mx[j - J0]);
    }
}

template <int R, bool FULL, bool ITER, typename GF>
__device__ __forceinline__ void assemble_p2(const MeshConst& c, int N, int row0, bool first, bool last_lane,
                                            double mu1, const double (&u)[R], double uL, double uR, double seL,
                                            GF&& g, const double (&se)[R], double (&lo)[R],
                                            double (&di)[R], double (&up)[R], double (&rhs)[R])
{
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const double um = (j == 0) ? uL : u[j - 1];
        const double ur = (j == R - 1) ? uR : u[j + 1];
        const double sm = (j == 0) ? seL : se[j - 1];
        const int i = row0 + j;
        double d = __builtin_fma(c.dt6, um - ur, c.dd2);
        double b = __builtin_fma(-c.kap, sm, g(j));
        double bb = __builtin_fma(c.kap, se[j], b);
        double l = lo[j], p = up[j];
        // special rows: last real row has no right element; rows >= N are identity
        const bool is_last = FULL ? (j == R - 1 && last_lane) : (i == N - 1);
        if (FULL ? (j == R - 1) : true) {
            double dl = __builtin_fma(c.dt6, __builtin_fma(2.0, u[j], um), c.dd1);
            d = is_last ? dl : d;
            p = is_last ? 0.0 : p;
            bb = is_last ? b : bb;
        }
        if (!FULL) {
            const bool pad = i >= N;
            d = pad ? 1.0 : d;
            p = pad ? 0.0 : p;
            l = pad ? 0.0 : l;
            bb = pad ? 0.0 : bb;   // u is 0 on padded rows, so rhs becomes 0 (ITER: so the solution is 0)
        }
        if (j == 0) {           // Dirichlet row (global row 0)
            d = first ? 1.0 : d;
            p = first ? 0.0 : p;
            l = first ? 0.0 : l;
            bb = first ? mu1 : bb;
        }
        double r = bb;
        if constexpr (!ITER) {
            r = __builtin_fma(-l, um, r);
            r = __builtin_fma(-d, u[j], r);
            r = __builtin_fma(-p, ur, r);
        }
        lo[j] = l; di[j] = d; up[j] = p; rhs[j] = r;
    }
}

// The two halves as calls of their own.  The head reads u, hf and the mesh constants only: not g, which changes per time
// step, and nothing of the solve.  So the head of an iterate can be formed as soon as the iterate exists, ahead of the
// stopping test, and serves whichever comes next: the next iteration, or the first iteration of the next time step, which
// starts from the same u (BG_PICARD_ROTATE, fom.hip).  The head hands uL, uR, se, lo and up to the tail.
// assemble below is head followed by tail, but written out: through the two calls the compiler commutes the operands of
// w = u[j] + ur in the kernels of 2 to 6 rows per lane (same bits, another listing).
template <int R, class Topo, typename HF>
__device__ __forceinline__ void assemble_head(Topo& tp, const MeshConst& c, const double (&u)[R], HF&& hf, double& uL,
                                              double& uR, double (&se)[R], double (&lo)[R], double (&up)[R])
{
    tp.halo(u[0], u[R - 1], uL, uR);
    assemble_p1<R>(c, u, uL, uR, hf, lo, up, se);
}

template <int R, bool FULL, bool ITER, class Topo, typename GF>
__device__ __forceinline__ void assemble_tail(Topo& tp, const MeshConst& c, int N, double mu1, const double (&u)[R],
                                              GF&& g, double uL, double uR, const double (&se)[R], double (&lo)[R],
                                              double (&di)[R], double (&up)[R], double (&rhs)[R])
{
    const double seL = tp.below_se(se[R - 1]);
    assemble_p2<R, FULL, ITER>(c, N, tp.g * R, tp.first(), tp.last(), mu1, u, uL, uR, seL, g, se, lo, di, up, rhs);
}

template <int R, bool FULL, bool ITER, class Topo, typename GF, typename HF>
__device__ __forceinline__ void assemble(Topo& tp, const MeshConst& c, int N, double mu1, const double (&u)[R], GF&& g,
                                         HF&& hf, double (&lo)[R], double (&di)[R], double (&up)[R], double (&rhs)[R])
{
    double uL, uR, se[R];
    tp.halo(u[0], u[R - 1], uL, uR);
    assemble_p1<R>(c, u, uL, uR, hf, lo, up, se);
    const double seL = tp.below_se(se[R - 1]);
    assemble_p2<R, FULL, ITER>(c, N, tp.g * R, tp.first(), tp.last(), mu1, u, uL, uR, seL, g, se, lo, di, up, rhs);
}

// ------------------------------------------------------------------------------------
// General (non-uniform) mesh variants.  Element e = (i, i+1) has length h_e = x[i+1]-x[i];
// the lane keeps h_e/6 and dt*E/h_e of its R right-hand elements plus the one left of its
// first row (index 0).  Same closed forms as above with per-element constants
// (SURVEY.md Appendix A); rows >= N are identity rows.  Slower than the uniform path
// (more live registers); used only when the host reports a non-uniform mesh.
// ------------------------------------------------------------------------------------
template <int R>
struct ElemGeom {
    double h6[R + 1];   // h_e / 6        (index j+1: element right of local row j; index 0: left of row 0)
    double eh[R + 1];   // dt * E / h_e
};

template <int R>
__device__ __forceinline__ void geom_setup(const double* __restrict__ x, int N, int row0, double dt, double E,
                                           ElemGeom<R>& gm)
{
#pragma unroll
    for (int j = 0; j <= R; ++j) {
        const int e = row0 + j - 1;                       // element (e, e+1)
        double h = 1.0;
        if (e >= 0 && e < N - 1) h = x[e + 1] - x[e];
        gm.h6[j] = (e >= 0 && e < N - 1) ? h / 6.0 : 0.0;
        gm.eh[j] = (e >= 0 && e < N - 1) ? dt * E / h : 0.0;
    }
}

template <int R>
__device__ __forceinline__ void forcing_setup_general(const double* __restrict__ x, int N, int row0, double mu2,
                                                      double dt, double (&hfs)[R], double (&fdt)[R])
{
    double frPrev = 0.0;
#pragma unroll
    for (int j = -1; j < R; ++j) {
        const int e = row0 + j;
        double fl = 0.0, fr = 0.0, hf = 0.0;
        if (e >= 0 && e < N - 1) {
            const double xl = x[e], xr = x[e + 1], h = xr - xl;
            const double f1 = 0.02 * exp(mu2 * (GP_A * xl + GP_B * xr));
            const double f2 = 0.02 * exp(mu2 * (GP_B * xl + GP_A * xr));
            fl = (f1 * GP_A + f2 * GP_B) * (0.5 * h);
            fr = (f1 * GP_B + f2 * GP_A) * (0.5 * h);
            hf = h * (f1 + f2);
        }
        if (j >= 0) {
            hfs[j] = hf;
            fdt[j] = (e < N) ? dt * (frPrev + fl) : 0.0;
        }
        frPrev = fr;
    }
}

template <int R, class Topo>
__device__ __forceinline__ void mass_rhs_general(Topo& tp, const ElemGeom<R>& gm, int N, const double (&u)[R],
                                                 const double (&fdt)[R], double (&g)[R])
{
    double uL, uR;
    tp.halo(u[0], u[R - 1], uL, uR);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const double um = (j == 0) ? uL : u[j - 1];
        const double up = (j == R - 1) ? uR : u[j + 1];
        const int i = tp.g * R + j;
        // (M u)_i = h_{i-1}/6 (u_{i-1} + 2 u_i) + h_i/6 (2 u_i + u_{i+1}); h6 is 0 outside the mesh
        double v = gm.h6[j] * __builtin_fma(2.0, u[j], um);
        v = __builtin_fma(gm.h6[j + 1], __builtin_fma(2.0, u[j], up), v);
        g[j] = (i >= N) ? 0.0 : v + fdt[j];
    }
    tp.halo_done();
}

// assemble_general in the same two halves.  p1: off-diagonals and the SUPG element terms se[];
// p2: diagonal, right-hand side (ITER as in assemble_p2), special rows.  `first` marks the thread that owns global row 0.
template <int R>
__device__ __forceinline__ void assemble_general_p1(const ElemGeom<R>& gm, double dt, const double (&u)[R], double uL,
                                                    double uR, const double (&hfs)[R], double (&lo)[R],
                                                    double (&up)[R], double (&se)[R])
{
    const double dt6 = dt / 6.0;
    double mx[R], t[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const double ur = (j == R - 1) ? uR : u[j + 1];
        const double w = u[j] + ur;
        const double dif = ur - u[j];
        const double aoff = gm.h6[j + 1] - gm.eh[j + 1];
        up[j] = __builtin_fma(dt6, w + u[j], aoff);
        if (j + 1 < R) lo[j + 1] = __builtin_fma(-dt6, w + ur, aoff);
        mx[j] = fmax(fabs(w), 2.0e-10);
        t[j] = __builtin_fma(w, dif, -hfs[j]);
    }
    supg_terms<R>(mx, t, se);
    lo[0] = __builtin_fma(-dt6, __builtin_fma(2.0, u[0], uL), gm.h6[0] - gm.eh[0]);
}

template <int R, bool ITER>
__device__ __forceinline__ void assemble_general_p2(const ElemGeom<R>& gm, double dt, double kap, int N, int row0,
                                                    bool first, double mu1, const double (&u)[R], double uL,
                                                    double uR, double seL, const double (&g)[R],
                                                    const double (&se)[R], double (&lo)[R], double (&di)[R],
                                                    double (&up)[R], double (&rhs)[R])
{
    const double dt6 = dt / 6.0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const double um = (j == 0) ? uL : u[j - 1];
        const double ur = (j == R - 1) ? uR : u[j + 1];
        const double sm = (j == 0) ? seL : se[j - 1];
        const int i = row0 + j;
        const double ddl = __builtin_fma(2.0, gm.h6[j], gm.eh[j]);          // h/3 + dt E/h of the left element
        const double ddr = __builtin_fma(2.0, gm.h6[j + 1], gm.eh[j + 1]);  // ... of the right element
        double d = __builtin_fma(dt6, um - ur, ddl + ddr);
        double b = __builtin_fma(-kap, sm, g[j]);
        double bb = __builtin_fma(kap, se[j], b);
        double l = lo[j], p = up[j];
        const bool is_last = (i == N - 1);
        const double dl = __builtin_fma(dt6, __builtin_fma(2.0, u[j], um), ddl);
        d = is_last ? dl : d;
        p = is_last ? 0.0 : p;
        bb = is_last ? b : bb;
        const bool pad = i >= N;
        d = pad ? 1.0 : d;
        p = pad ? 0.0 : p;
        l = pad ? 0.0 : l;
        bb = pad ? 0.0 : bb;
        if (j == 0) {
            d = first ? 1.0 : d;
            p = first ? 0.0 : p;
            l = first ? 0.0 : l;
            bb = first ? mu1 : bb;
        }
        double r = bb;
        if constexpr (!ITER) {
            r = __builtin_fma(-l, um, r);
            r = __builtin_fma(-d, u[j], r);
            r = __builtin_fma(-p, ur, r);
        }
        lo[j] = l; di[j] = d; up[j] = p; rhs[j] = r;
    }
}

// ... and as head and tail (see assemble_head)
template <int R, class Topo>
__device__ __forceinline__ void assemble_general_head(Topo& tp, const ElemGeom<R>& gm, double dt, const double (&u)[R],
                                                      const double (&hfs)[R], double& uL, double& uR, double (&se)[R],
                                                      double (&lo)[R], double (&up)[R])
{
    tp.halo(u[0], u[R - 1], uL, uR);
    assemble_general_p1<R>(gm, dt, u, uL, uR, hfs, lo, up, se);
}

template <int R, bool ITER, class Topo>
__device__ __forceinline__ void assemble_general_tail(Topo& tp, const ElemGeom<R>& gm, double dt, double kap, int N,
                                                      double mu1, const double (&u)[R], const double (&g)[R], double uL,
                                                      double uR, const double (&se)[R], double (&lo)[R],
                                                      double (&di)[R], double (&up)[R], double (&rhs)[R])
{
    const double seL = tp.below_se(se[R - 1]);
    assemble_general_p2<R, ITER>(gm, dt, kap, N, tp.g * R, tp.first(), mu1, u, uL, uR, seL, g, se, lo, di, up, rhs);
}

template <int R, bool ITER, class Topo>
__device__ __forceinline__ void assemble_general(Topo& tp, const ElemGeom<R>& gm, double dt, double kap, int N,
                                                 double mu1, const double (&u)[R], const double (&g)[R],
                                                 const double (&hfs)[R], double (&lo)[R], double (&di)[R],
                                                 double (&up)[R], double (&rhs)[R])
{
    double uL, uR, se[R];
    tp.halo(u[0], u[R - 1], uL, uR);
    assemble_general_p1<R>(gm, dt, u, uL, uR, hfs, lo, up, se);
    const double seL = tp.below_se(se[R - 1]);
    assemble_general_p2<R, ITER>(gm, dt, kap, N, tp.g * R, tp.first(), mu1, u, uL, uR, seL, g, se, lo, di, up, rhs);
}

// One PCR step on normalised equations A x[j-s] + x[j] + C x[j+s] = D; neighbours come from
// DPP moves (CTRL_DN: from lower lanes, CTRL_UP: from higher lanes, applied REPS times, zero
// filled out of range, which is the identity equation).  LAST skips the A/C update.
// The new right-hand side Dn is a function of its own, because on its short exit pcr64 needs nothing else of a step
// (a LAST step whose new diagonal is exactly 1, see there).
template <int CTRL_DN, int CTRL_UP, int REPS>
__device__ __forceinline__ double pcr_step_rhs(double A, double C, double D)
{
    const double Dm = dpp_shift<CTRL_DN, REPS>(D), Dp = dpp_shift<CTRL_UP, REPS>(D);
    return __builtin_fma(-Dp, C, __builtin_fma(-Dm, A, D));
}

// One Jacobi sweep x <- D - A x[j-s] - C x[j+s] on the same equations.  pcr_step_rhs shifts the vector it updates; the
// sweep shifts the iterate x and keeps D as the base (from x = D the two are the same operation).
template <int CTRL_DN, int CTRL_UP, int REPS>
__device__ __forceinline__ double pcr_jacobi_sweep(double A, double C, double D, double x)
{
    const double xm = dpp_shift<CTRL_DN, REPS>(x), xp = dpp_shift<CTRL_UP, REPS>(x);
    return __builtin_fma(-xp, C, __builtin_fma(-xm, A, D));
}

template <int CTRL_DN, int CTRL_UP, int REPS, bool LAST>
__device__ __forceinline__ void pcr_step(double& A, double& C, double& D)
{
    const double Cm = dpp_shift<CTRL_DN, REPS>(C), Ap = dpp_shift<CTRL_UP, REPS>(A);
    double Bn = __builtin_fma(-Cm, A, 1.0);
    Bn = __builtin_fma(-Ap, C, Bn);
    const double Dn = pcr_step_rhs<CTRL_DN, CTRL_UP, REPS>(A, C, D);
    const double rb = BG_RCP(Bn);
    D = Dn * rb;
    if (!LAST) {
        const double Am = dpp_shift<CTRL_DN, REPS>(A), Cp = dpp_shift<CTRL_UP, REPS>(C);
        A = -(Am * A) * rb;
        C = -(Cp * C) * rb;
    }
}

// ---- Wang partition inside one lane, in pieces (shared by the one-wave and the workgroup-wide solver) ----
// wang_reduce: phase 1 eliminates the sub-diagonal downwards (lo[] becomes the left spike f[], di[] becomes
// 1/pivot), phase 2 the super-diagonal upwards from row R-3 (gs[] is the right spike).  Returns the last pivot.
template <int R>
__device__ __forceinline__ double wang_reduce(double (&lo)[R], double (&di)[R], const double (&up)[R],
                                              double (&rhs)[R], double (&gs)[R])
{
    static_assert(R > 1, "R == 1 has no interior rows");
    double dp = di[0];
    di[0] = BG_RCP(dp);
#pragma unroll
    for (int j = 1; j < R; ++j) {
        const double m = lo[j] * di[j - 1];
        dp = __builtin_fma(-m, up[j - 1], di[j]);
        di[j] = BG_RCP(dp);
        rhs[j] = __builtin_fma(-m, rhs[j - 1], rhs[j]);
        lo[j] = -m * lo[j - 1];
    }
    gs[R - 2] = up[R - 2];
#pragma unroll
    for (int j = R - 3; j >= 0; --j) {
        const double t = up[j] * di[j + 1];
        rhs[j] = __builtin_fma(-t, rhs[j + 1], rhs[j]);
        lo[j] = __builtin_fma(-t, lo[j + 1], lo[j]);
        gs[j] = -t * gs[j + 1];
    }
    return dp;
}

// Interface equation A x[p-1] + x[p] + C x[p+1] = D of this lane's last row, closed with the next lane's
// normalised row 0 (F0, G0, R0 = lo[0]/di[0], gs[0]/di[0], rhs[0]/di[0] over there; zeros past the last lane).
template <int R>
__device__ __forceinline__ void wang_interface(const double (&lo)[R], const double (&up)[R], const double (&rhs)[R],
                                               double dp, double F0, double G0, double R0, double& A, double& C,
                                               double& D)
{
    const double ul = up[R - 1];
    const double B = __builtin_fma(-ul, F0, dp);
    const double rb = BG_RCP(B);
    A = lo[R - 1] * rb;
    C = -(ul * G0) * rb;
    D = __builtin_fma(-ul, R0, rhs[R - 1]) * rb;
}

// Back-substitution: X = this lane's last unknown, XL = the previous lane's.  Solution lands in rhs[].
// SCALE = false leaves the last multiply of the rows j < R-1 to the caller: x_j = rhs[j] * di[j], and rhs[R-1] = X as
// always.  fom_sample forms x_j - u_j from the two factors in one FMA and writes x_j over u_j after it (fom.hip).
template <int R, bool SCALE = true>
__device__ __forceinline__ void wang_finish(const double (&lo)[R], const double (&di)[R], double (&rhs)[R],
                                            const double (&gs)[R], double X, double XL)
{
#pragma unroll
    for (int j = 0; j < R - 1; ++j) {
        double v = __builtin_fma(-lo[j], XL, rhs[j]);
        v = __builtin_fma(-gs[j], X, v);
        rhs[j] = SCALE ? v * di[j] : v;
    }
    rhs[R - 1] = X;
}

// PCR over 64 normalised equations, one per lane; returns x of this lane's equation.
// ds_bpermute costs ~24 cycles per dword on gfx950 against ~6 for a DPP move, so: strides 1 and 2 use
// wave_shr/wave_shl:1 (once / twice, zero filled), then ONE lane transpose (lane' = 16*(j&3) + (j>>2)) turns
// the four interleaved stride-4 systems into the four 16-lane DPP rows, where strides 4,8,16,32 are
// row_shr/shl 1,2,4,8 with zero fill at the row ends (= the system ends).
//
// Early exit (BG_PCR_EARLY_EXIT): a step multiplies the couplings pairwise (A' = -A_m A / B), so they are
// squared per step, and on diagonally dominant systems the late steps change nothing.  After the stride-4
// step the wave asks whether EVERY lane has |A| <= tau and |C| <= tau, tau = 2^-31.  If so, the stride-8
// step runs in its LAST form and strides 16 and 32 are dropped.  With all couplings <= m going into a step,
// B_n >= 1 - 2 m^2 and the couplings coming out are <= m^2 / (1 - 2 m^2); with m <= 2^-31 they are
// <= 2^-62 (1 + eps) after the LAST step.  Each dropped step would have changed D_j by at most twice that
// times max|D|, so the truncated solve differs from the full one by < 2^-60 max_j |X_j|: below half an ulp
// of the largest interface unknown.  The test is written so that a NaN or inf coupling fails it, and it is
// one ballot, uniform over the wave (the DPP moves below it need all 64 lanes): a wave with one lane over
// tau, or a non-finite one, takes the full path, whose arithmetic is that of -DBG_PCR_EARLY_EXIT=0.
//
// B_n == 1 on the short exit.  That LAST step computes D = D_n * rcp1(B_n), B_n = fma(-A_p, C, fma(-C_m, A, 1)).
// Every coupling that passed the ballot is finite and <= 2^-31 (a neighbour out of range is the zero fill), so
// each product is <= 2^-62, and 1 - x rounds to 1 for |x| < 2^-54 (half the spacing of the doubles below 1):
// both FMAs return exactly 1.0, rcp1(1.0) is exactly 1.0 (v_rcp_f64 of a power of two is exact, the Newton
// step then adds r * 0), and D_n * 1.0 is D_n, bit for bit.  So the short exit forms D_n alone: no DPP moves of
// the couplings, no reciprocal, no multiply, and the chain in front of the back-transpose is two DPP moves and
// two FMAs long (budget and measurements: DESIGN.md K1).
//
// Jacobi exit (BG_PCR_JACOBI_EXIT): after the stride-1 step the equations read A x[j-2] + x[j] + C x[j+2] = D, that is
// (I + N) x = D with ||N||_inf <= 2 m for couplings <= m, and where the mesh gives a lane many rows m is already small
// (9.3e-4 at 16 rows per lane on the flagship workload).  The wave asks once whether EVERY lane has
// |A| <= tau_J and |C| <= tau_J, tau_J = 2^-9, a NaN or inf coupling failing the test as it does the one against tau.
// If so it runs K = 6 sweeps x <- D - A x[j-2] - C x[j+2] from x = D and returns x: no update of A and C, no
// reciprocal, no transpose in either direction and no LDS instruction, two double moves by two lanes and two FMAs a
// sweep.  x_0 = D is off by N x, a sweep multiplies the error by -N, so with rho = 2 tau_J = 2^-8 the result is off by
// <= rho^(K+1) max|x| <= 2^-56 max|D| / (1 - 2^-8): below half an ulp of the largest interface unknown, the standard of
// the exit against tau.  One threshold and one K for every workload.  A wave with one lane over tau_J, or a non-finite
// one, runs everything after the stride-1 step as before (pcr64_from_stride2), both exits of the tau test included.
//
// What "half an ulp of the largest interface unknown" is in absolute terms depends on the caller's unknown, for all three
// exits (tau, Jacobi, one-sided): 1e-16 |du| where the Picard loop solves for the increment, 1e-16 |u| in its lean
// iterations, which solve for the iterate (assemble_p2, ITER).  The thresholds read the couplings only and stay as they are.
__device__ __forceinline__ double pcr64_from_stride2(double A, double C, double D)
{
    const int lane = lane_id();
    pcr_step<0x138, 0x130, 2, false>(A, C, D);
    {
        const int src = ((4 * (lane & 15) + (lane >> 4)) << 2);
        A = from_lane_rot(A, src); C = from_lane_rot(C, src); D = from_lane_rot(D, src);
    }
    pcr_step<0x111, 0x101, 1, false>(A, C, D);
#if BG_PCR_EARLY_EXIT
    constexpr double tau = 0x1p-31;
    const bool coupled = !(__builtin_fabs(A) <= tau && __builtin_fabs(C) <= tau);
    const bool full = __builtin_amdgcn_ballot_w64(coupled) != 0;
    // The short exit's whole stride-8 step (D = Dn, see above) is formed ahead of the branch and the old D kept, so
    // that the full path is one `if` without an `else`, which starts again from the old D, and the short path falls
    // through one not-taken scalar branch (an if / else cost the short path three more branches and measured 0.5 %
    // slower).
    const double D4 = D;
    D = pcr_step_rhs<0x112, 0x102, 1>(A, C, D4);
    if (__builtin_expect(full, 0)) {
        D = D4;
        pcr_step<0x112, 0x102, 1, false>(A, C, D);
        pcr_step<0x114, 0x104, 1, false>(A, C, D);
        pcr_step<0x118, 0x108, 1, true>(A, C, D);
    }
#else
    pcr_step<0x112, 0x102, 1, false>(A, C, D);
    pcr_step<0x114, 0x104, 1, false>(A, C, D);
    pcr_step<0x118, 0x108, 1, true>(A, C, D);
#endif
    return from_lane_rot(D, (16 * (lane & 3) + (lane >> 2)) << 2);
}

// Everything after the stride-1 step where the Jacobi exit is compiled in: the ballot against tau_J, the six two-sided
// sweeps, otherwise pcr64_from_stride2.
__device__ __forceinline__ double pcr64_jacobi(double A, double C, double D)
{
    constexpr double tau_j = 0x1p-9;
    constexpr int sweeps = 6;
    const bool coupled = !(__builtin_fabs(A) <= tau_j && __builtin_fabs(C) <= tau_j);
    const bool eliminate = __builtin_amdgcn_ballot_w64(coupled) != 0;
    // As with the exit against tau: the sweeps stand ahead of the branch and the elimination is one `if` without
    // an `else`, out of line, which starts again from A, C, D of the stride-1 step.
    double X = D;
#pragma unroll
    for (int k = 0; k < sweeps; ++k) X = pcr_jacobi_sweep<0x138, 0x130, 2>(A, C, D, X);
    if (__builtin_expect(eliminate, 0)) X = pcr64_from_stride2(A, C, D);
    return X;
}

// One-sided exit (BG_PCR_ONESIDED_EXIT, callers that pass ONESIDED): a convection-dominated matrix couples an interface
// to one side only.  Inside a lane the flagship's left spike decays by 0.49 per row and its right one by 0.80, so after
// the stride-1 step |A| <= 3.9e-10 where |C| reaches 9.3e-4.  An A that small moves x by 1e-10 relative:
// it has to be applied once, to a modestly accurate x, and not in every sweep.  The wave asks once whether EVERY lane has
// |A| <= tau_A = 2^-28 and |C| <= tau_J = 2^-9 (negated form: a NaN or inf coupling fails).  If so it runs, from y = D,
//   two sweeps  y <- D - C y[j+2],   then side by side the fold  D' = D - A y[j-2]  and a third sweep  y <- D - C y[j+2],
//   then three sweeps  y <- D' - C y[j+2]  from the current y
// and returns y: seven moves of one double by two lanes and seven FMAs, against twelve and twelve of the six two-sided
// sweeps, in a chain six sweeps long.  The fold reads the second iterate and not the third, so that it does not stand in
// that chain: a sweep is one dependent move by two lanes and one FMA, with one wave per SIMD nothing else fills the wait
// between them, and with the fold behind the third sweep the route measured no faster than the six two-sided sweeps, whose
// two moves fill each other's waits.
// Bound, with c = max|C| <= 2^-9, a = max|A| <= 2^-28, U = (I + C S+)^-1 and the exact x = U (D - A S- x): a sweep
// contracts towards U D by c and y_0 = D is c |D| / (1 - c) off it, so y_2 is within c^3 |D| / (1 - c) of U D and, x - U D
// being a |x|, within (c^3 + a) |D| (1 + o(1)) of x.  The fold therefore misses D - A S- x by <= a (c^3 + a) |D| =
// 1.5 * 2^-55 |D|.  y_3 is within c^4 |D| of U D and so within (c^4 + a) |D| of the fixed point U D' of the last three
// sweeps, which leave c^3 of that, 2^-55 |D|.  Together 2.5 * 2^-55 (1 + o(1)) |D| and, with |D| <= (1 + c + a) max|x|,
// < 2^-53 max|x|: below half an ulp of the largest interface unknown, the standard of both exits above.  A wave with one
// lane over either threshold (a leftward flow with |C| <= tau_A included: the mirrored route is not built) restarts from
// A, C, D of the stride-1 step and runs pcr64_jacobi, in one `if` without an `else`, out of line, with the route
// standing ahead of that branch as the sweeps do there.
__device__ __forceinline__ double pcr64_onesided(double A, double C, double D)
{
    constexpr double tau_a = 0x1p-28, tau_j = 0x1p-9;
    const bool twosided = !(__builtin_fabs(A) <= tau_a && __builtin_fabs(C) <= tau_j);
    const bool fallback = __builtin_amdgcn_ballot_w64(twosided) != 0;
    double y = D;
#pragma unroll
    for (int k = 0; k < 2; ++k) y = __builtin_fma(-dpp_shift<0x130, 2>(y), C, D);
    const double Df = __builtin_fma(-dpp_shift<0x138, 2>(y), A, D);
    y = __builtin_fma(-dpp_shift<0x130, 2>(y), C, D);
#pragma unroll
    for (int k = 0; k < 3; ++k) y = __builtin_fma(-dpp_shift<0x130, 2>(y), C, Df);
    if (__builtin_expect(fallback, 0)) y = pcr64_jacobi(A, C, D);
    return y;
}

// ROWS = rows per lane of the caller's partition: a wave that fails the test has paid for the sweeps, so the exit is
// compiled in where the mesh gives a lane at least BG_PCR_JACOBI_MIN_ROWS rows (DESIGN.md K1 has the measurements).
// ONESIDED = the caller's systems are expected to pass the one-sided ballot (a wave that fails it has paid for that
// route before it takes the other): the kernels that have it are listed in DESIGN.md K1.
template <int ROWS, bool ONESIDED = false>
__device__ __forceinline__ double pcr64(double A, double C, double D)
{
    pcr_step<0x138, 0x130, 1, false>(A, C, D);
    if constexpr (BG_PCR_JACOBI_EXIT && ROWS >= BG_PCR_JACOBI_MIN_ROWS) {
        if constexpr (BG_PCR_ONESIDED_EXIT && ONESIDED) return pcr64_onesided(A, C, D);
        else return pcr64_jacobi(A, C, D);
    } else {
        return pcr64_from_stride2(A, C, D);
    }
}

// Pivot-free tridiagonal solve across the wave (Wang partition + PCR on the 64
// interface unknowns).  In: lo/di/up/rhs.  Out: solution in rhs.  lo, di are clobbered.  ONESIDED: see pcr64.
// SCALE = false: the solution is rhs[j] * di[j] for j < R-1 and rhs[R-1] (see wang_finish; R = 1 has no such rows).
template <int R, bool ONESIDED = false, bool SCALE = true>
__device__ __forceinline__ void tridiag_solve(double (&lo)[R], double (&di)[R], const double (&up)[R],
                                              double (&rhs)[R])
{
    if constexpr (R == 1) {
        const double rb = BG_RCP(di[0]);
        rhs[0] = pcr64<R>(lo[0] * rb, up[0] * rb, rhs[0] * rb);
    } else {
        double gs[R];
        const double dp = wang_reduce<R>(lo, di, up, rhs, gs);
        const double F0 = from_lane_above(lo[0] * di[0]);
        const double G0 = from_lane_above(gs[0] * di[0]);
        const double R0 = from_lane_above(rhs[0] * di[0]);
        double A, C, D;           // normalised interface equation: A x[p-1] + x[p] + C x[p+1] = D
        wang_interface<R>(lo, up, rhs, dp, F0, G0, R0, A, C, D);
        const double X = pcr64<R, ONESIDED>(A, C, D);
        wang_finish<R, SCALE>(lo, di, rhs, gs, X, from_lane_below(X));
    }
}

}  // namespace bg
