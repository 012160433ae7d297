// rom_hyper.hip -- the whole HYPER-REDUCED POD-PROM time loop of one sample on one compute unit (bg_hyper_rom_run): the
// reduced system is assembled from m sampled mesh rows with weights xi >= 0 (ECSW-style: Ar = sum_j xi_j w_j^T y_j,
// br = sum_j xi_j w_j^T R_j over the sampled rows only; w_j = Phi[i_j] for Galerkin, y_j = (A Phi)[i_j] for LSPG), so an
// iteration costs O(m r^2) whatever the mesh size, and the kernel never touches a vector of mesh length.
// reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785, with the sums over mesh rows restricted and weighted.
//
// Row i of the assembly needs the state, the basis and the coordinates at nodes i - 1, i, i + 1 only.  The caller packs
// the stencil rows of the basis once: PhiS [MPAD][3][42], MPAD = m rounded up to 32, rows Phi[i-1], Phi[i], Phi[i+1] of
// sampled row j at 3 j .. 3 j + 2 (zero rows outside the mesh and beyond m, zero columns beyond r; the 42-double row is the
// LDS row of rom_long.hip, so a slab is one contiguous piece of the table).  The table is shared by all samples and
// L2-resident (up to 258 KB); it streams through LDS 32 sampled rows at a time, double buffered, by LDS DMA, as K12 streams
// PhiP (rom_stream_device.hpp).  Per slab:
//   four lanes per sampled row lift the stencil u_{i-1}, u_i, u_{i+1} = PhiS q (the very first iteration of a run reads u0s
//   instead, as the reference starts from u0 and not from Phi Phi^T u0) and assemble A(u), R(u) of row i (rom_assemble_row);
//   the first iteration of a step also forms g_i = (M u^n + dt F)_i from the same stencil, which is u^n then.  The weight goes
//   into the coefficients: lo, di, up, R times xi (Galerkin) or sqrt(xi) (LSPG), so the matrix instructions are the
//   unweighted loop's  ->  each wave forms the rows of Y it multiplies (stream_step_mfma: the block pairs dealt to the four
//   waves)  ->  v_mfma_f64_4x4x4_4b.  Two workgroup barriers per slab.
// Then the system is parked over the dead slabs and solved by rom_fused_device.hpp's r <= 40 routines, q <- q + dq (equal to
// the reference's Phi^T u_k + dq for an orthonormal basis, since u_k = Phi q), the stopping test |dq| / |q|.  There is no
// lift-only sweep: the output is q itself, [B][nsteps + 1][r].  Pivoting is repaired inside the call as in bg_rom_run_long.
//
// The arithmetic of an iteration is the full loops' own code: the lift of a row and the operands Y, P of a row step are
// rom_stream_device.hpp's stream_lift_rows and stream_row_operands (there the three rows are neighbours in the slab, here
// 3 j .. 3 j + 2 of it), the matrix steps and the parking its stream_step_mfma and stream_park, the solve
// rom_long_device.hpp's LongLayout::solve_add (dq added to q, where the streaming loops add it to the parked Phi^T u),
// mass row and assembly rom_device.hpp's rom_mass_rhs_node and rom_assemble_row, reading the stencil coordinates xs as a
// mesh x.  This file's own: the contiguous slab DMA, the weights, the start from u0s, the frame of the loop, and the
// per-sample forcing loads (hyper_row_forcing, which says why).
//
// Local POD (bg_hyper_local_rom_run) is the same body with LOCAL = true: one table per cluster, the nearest-centre pick at the
// top of every time step from reduced coordinates, and the change of basis q <- Phi_c^T Phi_p q when the cluster changes
// (the additions sit under `if constexpr (LOCAL)`, described at HyperLocalRunArgs).  Its kernel and entry point are compiled
// in a translation unit of their own, rom_hyper_local.hip, which includes this file with BG_ROM_HYPER_LOCAL_TU defined, as
// rom_local_fused.hip does with rom_fused.hip: the four kernels here are meant to stay exactly what they were.
//
// The larger bases (bg_hyper_rom_run_wide, 40 < r <= 96, m <= 512) are the same body with another description K in the place of
// LongLayout (HyperDims says what the body asks of one): rom_hyper_wide.hip, which includes this file with
// BG_ROM_HYPER_WIDE_TU defined for the same reason.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rom_long_device.hpp"

namespace {

using namespace bg;

// What the body needs of a description K besides rom_stream_device.hpp's list: the sampled rows per slab and how many
// values of q a lane carries through the solve (1: K::solve_add(L, r, lane, base, ...) as LongLayout's;
// 2: rows lane and 64 + lane, K::solve_add<GAL, W>(L, r, lane, base0, base1, force, aborted, nd, nq), and under PIV
// K::solve_add_pivoted<GAL, W>(L, r, lane, base0, base1, info_out, nd, nq)).
template <class K>
struct HyperDims;
template <>
struct HyperDims<LongLayout> {
    static constexpr int HS = 32, per_lane = 1;
};
template <class K>
constexpr int hyper_slab = 3 * HyperDims<K>::HS * K::PS;      // doubles of one slab buffer: three stencil rows per sampled row

constexpr int HS = HyperDims<LongLayout>::HS;                  // sampled rows per slab
constexpr int HMMAX = 256;                                     // sampled rows held
constexpr int HSLAB = hyper_slab<LongLayout>;
constexpr int HWG_PER_CU = 2;

struct HyperRunArgs {
    const int32_t* rows;    // [m]
    const double* xi;       // [m]
    const double* xs;       // [m][3]
    const double* PhiS;     // [MPAD][3][LPS]
    const double* q0;       // [B][r]
    const double* u0s;      // [B][m][3]
    const double* mu1;      // [B]
    const double* mu2;      // [B]
    double* qhist;          // [B][nsteps+1][r]
    int32_t* iters;         // [B][nsteps]
    int32_t* flags;         // [B]
    int32_t* info;          // [B]
    const int32_t* order;   // [B] or null
    double dt, E, tol;
    int N, B, r, m, nsteps, max_it, supg, nonuniform, force_pivoted;
};

// Local POD (LOCAL; reference FEMBurgers.local_prom_burgers, FEM/fem_burgers.py:979-1079, with the sums over mesh rows
// restricted and weighted by ONE sampling for all clusters).  The state of a sample is (p, q): the cluster held and the
// coordinates in its basis, u = Phi_p q.  PhiS is the stack [C][MPAD][3][LPS] of the clusters' stencil tables (`table` doubles
// each), q0 the projections [B][C][r] of u0 on every basis.  At the top of step n >= 1: q_g = pick[p] q (= U_g^T u^n), the
// nearest centre c (local_nearest_centre, the pick of the full local loops), and if c != p
//   one lift-only sweep over the OLD table leaves u^n at the stencil nodes of every sampled row in LDS (H.g, H.u0, H.ur), which
//   the first iteration of the step reads where the first iteration of a run reads u0s -- the reference assembles g, A and R
//   at U0 = u^n, which is not in the new span, while Y and W are the new basis's;
//   q <- trans[c][p] q, the base of the update: the reference's q = Phi_c^T U0 + dq.
// From the second iteration on, and in steps without a switch, the step is the POD loop's with the width widths[c]: the solve
// gives the unknowns at and beyond it a unit diagonal and a zero correction (LongLayout::solve_add).  Step 0 picks from qg0.
struct HyperLocalRunArgs : HyperRunArgs {
    const int32_t* widths;  // [C], 1 .. r (clamped to r)
    const double* trans;    // [C][C][LR][LR]: trans[c][p] = Phi_c^T Phi_p, zero rows and columns beyond the widths
    const double* pick;     // [C][mg][LR]: pick[p] = U_g^T Phi_p, zero columns beyond the width
    const double* centres;  // [C][mg]
    const double* qg0;      // [B][mg] = U_g^T u0
    int32_t* clusters;      // [B][nsteps] or null
    long long table;        // doubles of one cluster's table in PhiS
    int C, mg;
};

struct HyperLds {
    double* g; double* fdt; double* hl; double* hr; double* w;      // [HMMAX] per sampled row: M u^n + dt F, dt F, h_f left / right, weight factor
    int* row;                                                        // [HMMAX] mesh row (N beyond m: an identity row with weight 0)
    double* u0; double* ur; double* qg;                              // LOCAL: [HMMAX] u^n at nodes i, i + 1 after a switch (i - 1 in g); [64] q_g
};

// Loads of the forcing term at a sampled row with the stencil coordinates xm, x0, xp: dt F_i, and h_e (f(gp1) + f(gp2)) of
// the left and right element; 0 where the mesh has no such element.  The formulas are rom_nodal_forcing's (rom_device.hpp);
// the last bit is not.  Both functions leave sums of two products (`GP_A * xm + GP_B * x0`, `f1 * GP_B + f2 * GP_A`) to the
// compiler's contraction: here it fuses the product with x0 in both elements, there the product with the element's left
// node, and in the full loops it leaves frPrev unfused (profiles/hyper_stream_isa.md).  Calling rom_nodal_forcing from here
// changed q in its last bits in every all-rows run (profiles/hyper_stream_ab.md).  One routine for both needs the fused
// product spelled with __builtin_fma, and that changes one side's results.
__device__ __forceinline__ void hyper_row_forcing(double xm, double x0, double xp, int i, int N, double mu2, double h, int nonuniform,
                                                  double dt, double& fdt, double& hl, double& hr)
{
    double frPrev = 0.0, fl = 0.0;
    hl = 0.0; hr = 0.0;
    if (i > 0) {
        const double he = nonuniform ? x0 - xm : h;
        const double f1 = 0.02 * exp(mu2 * (GP_A * xm + GP_B * x0));
        const double f2 = 0.02 * exp(mu2 * (GP_B * xm + GP_A * x0));
        frPrev = (f1 * GP_B + f2 * GP_A) * (0.5 * he);
        hl = he * (f1 + f2);
    }
    if (i < N - 1) {
        const double he = nonuniform ? xp - x0 : h;
        const double f1 = 0.02 * exp(mu2 * (GP_A * x0 + GP_B * xp));
        const double f2 = 0.02 * exp(mu2 * (GP_B * x0 + GP_A * xp));
        fl = (f1 * GP_A + f2 * GP_B) * (0.5 * he);
        hr = he * (f1 + f2);
    }
    fdt = dt * (frPrev + fl);
}

// The body for wave W of the workgroup (a template parameter of the whole body, as in rom_stream_body: every wave keeps
// its own quarter of the block pairs in accumulators that never change registers).  The description K: LongLayout as it
// stands (the items, matrix steps, parking and solve of the r <= 40 streaming loops), or rom_hyper_wide.hip's for r <= 96.
template <bool GAL, bool PIV, int W, bool LOCAL = false, class A = HyperRunArgs, class K = LongLayout>
__device__ __forceinline__ void hyper_body(const A& a, const StreamLds& L, const HyperLds& H)
{
    static_assert(!LOCAL || HyperDims<K>::per_lane == 1, "the local additions are written for one value of q per lane");
    constexpr int NB = K::NB, R = 4 * NB, PS = K::PS;
    constexpr int HS = HyperDims<K>::HS, HSLAB = hyper_slab<K>, HCHUNKS = (HSLAB * 8 + 1023) / 1024;
    constexpr int NACC = StreamItems<K, GAL>::per_wave;
    constexpr int w = W;
    double* const s_slab = L.slab;
    double (*const s_cf)[4] = L.cf;
    double* const s_q = L.q;
    double* const S = s_slab;                                    // [R][LSW]: Ar | br (over the dead slabs)

    const int tid = threadIdx.x;
    const int N = a.N, m = a.m;
    const int nslab = (m + HS - 1) / HS;
    // Uniform meshes (BG_OPT_NONUNIFORM clear): the spacing from the outermost stencil nodes -- (x[N-1] - x[0]) / (N - 1), what
    // the other loops use, when rows 0 and N - 1 are both sampled.
    const int i_first = a.rows[0], i_last = a.rows[m - 1];
    const int lo_off = i_first > 0 ? 0 : 1, hi_off = i_last < N - 1 ? 2 : 1;
    const double h = (a.xs[3 * (m - 1) + hi_off] - a.xs[lo_off]) / (double)((i_last + hi_off) - (i_first + lo_off));
    // ---- per-row constants of the sampling, the same for every sample ----------------------------------------------------
    for (int j = tid; j < nslab * HS; j += 256) {
        const double xi = (j < m) ? a.xi[j] : 0.0;
        H.row[j] = (j < m) ? a.rows[j] : N;
        H.w[j] = GAL ? xi : sqrt(xi);
    }

    for (int slot = blockIdx.x; slot < a.B; slot += gridDim.x) {
        const int smp = a.order ? a.order[slot] : slot;
        if (smp < 0 || smp >= a.B) continue;                     // workgroup-uniform
        if (PIV && !a.force_pivoted && a.info[smp] != BG_INFO_NEEDS_PIVOTING) continue;      // workgroup-uniform
        const double mu1 = a.mu1[smp], mu2 = a.mu2[smp];
        double* qhist = a.qhist + (size_t)smp * (size_t)(a.nsteps + 1) * (size_t)a.r;
        const double* u0s = a.u0s + (size_t)smp * (size_t)m * 3;
        __syncthreads();
        // LOCAL: the cluster held with its table and width (workgroup-uniform: every wave computes the same pick); otherwise the
        // arguments are read where they are used, as before there was a pick
        int cl = 0, r_local = 0;
        const double* PhiL = nullptr;
        auto step_table = [&]() -> const double* { if constexpr (LOCAL) return PhiL; else return a.PhiS; };
        auto step_width = [&]() -> int { if constexpr (LOCAL) return r_local; else return a.r; };
        auto q0_row = [&]() -> const double* {
            if constexpr (LOCAL) return a.q0 + ((size_t)smp * a.C + cl) * a.r; else return a.q0 + (size_t)smp * a.r;
        };
        auto hold_cluster = [&](int c) {
            if constexpr (LOCAL) {
                cl = c;
                PhiL = a.PhiS + (size_t)c * (size_t)a.table;
                r_local = a.widths[c] < a.r ? a.widths[c] : a.r;      // (clamped: the tables are LR wide, a.r <= LR)
            }
        };
        if constexpr (LOCAL) {
            if (tid < a.mg) H.qg[tid] = a.qg0[(size_t)smp * a.mg + tid];
        }
        // ---- per-sample constants (compute_forcing_vector :427-461, f_gp of :556-558) and the initial coordinates -------
        for (int j = tid; j < nslab * HS; j += 256) {
            double fdt = 0.0, hl = 0.0, hr = 0.0;
            if (j < m) hyper_row_forcing(a.xs[3 * j], a.xs[3 * j + 1], a.xs[3 * j + 2], H.row[j], N, mu2, h, a.nonuniform, a.dt, fdt, hl, hr);
            H.fdt[j] = fdt; H.hl[j] = hl; H.hr[j] = hr;
        }
        if constexpr (LOCAL) {                                    // the cluster of u0 (:1011-1012) and its projection of u0
            __syncthreads();
            hold_cluster(local_nearest_centre(H.qg, a.centres, a.C, a.mg, tid & 63));
        }
        if (tid < R) {
            const double q = (tid < a.r) ? q0_row()[tid] : 0.0;
            s_q[tid] = q;
            if (tid < a.r) qhist[tid] = q;
        }
        __syncthreads();

        int flags = 0, info_out = 0;
        bool aborted = false;
        // LDS DMA of slab `slab` (rows 3 HS slab .. of the table, contiguous) into buffer `buf`: wave w moves the 1-KB pieces
        // w, w + 4, ...; lanes beyond the slab's end write nothing (the next buffer starts there)
        auto slab_dma = [&](int slab, int buf) {
            const char* src = reinterpret_cast<const char*>(step_table() + (size_t)slab * HSLAB);
            const int ln = tid & 63;
            for (int j = w; j < HCHUNKS; j += 4) {
                const int o = 1024 * j + 16 * ln;
                if (o < HSLAB * 8)
                    __builtin_amdgcn_global_load_lds((gbl_void_t*)(src + o), (lds_void_t*)(reinterpret_cast<char*>(s_slab + buf * HSLAB) + 1024 * j), 16, 0, 0);
            }
        };

        for (int step = 0; step < a.nsteps && info_out == 0 && !aborted; ++step) {
            bool switched = false;
            if constexpr (LOCAL) {
                if (step > 0) {
                    // ---- q_g = pick[p] q (U_g^T u^n, :1011) by four lanes per global mode, then kmeans.predict (:1012) ------------
                    {
                        const int j = tid >> 2, pt = tid & 3;
                        double s = 0.0;
                        if (j < a.mg) {
                            const double* pr = a.pick + ((size_t)cl * a.mg + j) * R + NB * pt;
#pragma unroll
                            for (int c = 0; c < NB; ++c) s = __builtin_fma(pr[c], s_q[NB * pt + c], s);
                        }
                        s += dpp_mov<0xB1>(s); s += dpp_mov<0x4E>(s);
                        if (pt == 0 && j < a.mg) H.qg[j] = s;
                    }
                    __syncthreads();
                    const int c = local_nearest_centre(H.qg, a.centres, a.C, a.mg, tid & 63);
                    if (c != cl) {                                 // workgroup-uniform
                        // ---- u^n = Phi_p q at the stencil nodes: one lift-only sweep over the old table (no DMA is in flight) ----
                        const int q4 = tid >> 2, pt = tid & 3;
                        slab_dma(0, 0);
                        for (int slab = 0; slab < nslab; ++slab) {
                            const int cur = slab & 1;
                            const double* s_P = s_slab + cur * HSLAB;
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's DMA pieces of the slab have landed
                            __syncthreads();                                          // ... and everybody's; the other buffer is no longer read
                            if (slab + 1 < nslab) slab_dma(slab + 1, cur ^ 1);
                            if (q4 < HS) {                                            // (wave-uniform: the first HS / 16 waves)
                                double um, u0, ur;
                                stream_lift_rows<NB, PS>(s_P + 3 * q4 * PS + NB * pt, s_q + NB * pt, um, u0, ur);
                                if (pt == 0) { const int j = slab * HS + q4; H.g[j] = um; H.u0[j] = u0; H.ur[j] = ur; }
                            }
                        }
                        // ---- q <- Phi_c^T Phi_p q by four lanes per row of trans[c][p] (zero rows beyond the new width) ------------
                        double t = 0.0;
                        if (q4 < R) {
                            const double* tr = a.trans + (((size_t)c * a.C + cl) * R + q4) * R + NB * pt;
#pragma unroll
                            for (int e = 0; e < NB; ++e) t = __builtin_fma(tr[e], s_q[NB * pt + e], t);
                        }
                        t += dpp_mov<0xB1>(t); t += dpp_mov<0x4E>(t);
                        __syncthreads();                           // the sweep is over: the slabs and the old q are no longer read
                        if (pt == 0 && q4 < R) s_q[q4] = t;        // (read again behind the barriers of the first iteration)
                        hold_cluster(c);
                        switched = true;
                    }
                }
                if (tid == 0 && a.clusters) a.clusters[(size_t)smp * a.nsteps + step] = cl;
            }
            int k = 0;
            while (true) {
                // per-lane indices from an opaque copy of the thread index (see rom_stream_body)
                int tid_i = tid;
                asm volatile("" : "+v"(tid_i));
                const int lane = tid_i & 63, pk = lane >> 4, pblk = (lane >> 2) & 3, pt = lane & 3;
                // the first iteration of a run assembles at u0 itself (:725); LOCAL: the first after a switch at the old basis's u^n
                const bool lift = LOCAL ? ((step > 0 && !switched) || k > 0) : (step > 0 || k > 0);
                double acc[NACC];
#pragma unroll
                for (int p = 0; p < NACC; ++p) acc[p] = 0.0;
                slab_dma(0, 0);                                // (not across the pass boundary: the parked system lies over both buffers)
                for (int slab = 0; slab < nslab; ++slab) {
                    const int cur = slab & 1;
                    const double* s_P = s_slab + cur * HSLAB;                 // local row 3 l + s: stencil row s of sampled row HS slab + l
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's DMA pieces of the slab have landed
                    __syncthreads();                                          // ... and everybody's; the other buffer and s_cf are no longer read
                    if (slab + 1 < nslab) slab_dma(slab + 1, cur ^ 1);        // the next slab lands while this one is worked on
                    // ---- four lanes per sampled row: the stencil of u = PhiS q (:773), then A(u), R(u) of the row -----------------
                    const int q4 = tid_i >> 2;
                    if (q4 < HS) {                                            // (wave-uniform: the first HS / 16 waves)
                        const int j = slab * HS + q4;
                        double um, u0, ur;
                        if (lift) {                                            // rows outside the mesh are zero rows of PhiS
                            stream_lift_rows<NB, PS>(s_P + 3 * q4 * PS + NB * pt, s_q + NB * pt, um, u0, ur);
                        } else {
                            um = u0 = ur = 0.0;
                            if (pt == 0 && j < m) {
                                if (LOCAL && step > 0) { um = H.g[j]; u0 = H.u0[j]; ur = H.ur[j]; }      // (H.g[j] becomes g below)
                                else { um = u0s[3 * j]; u0 = u0s[3 * j + 1]; ur = u0s[3 * j + 2]; }
                            }
                        }
                        if (pt == 0) {
                            const int i = H.row[j];
                            const bool in = i < N;
                            if (i == 0) um = 0.0;                                      // slots outside the mesh are ignored
                            if (i + 1 >= N) ur = 0.0;
                            // the stencil coordinates as the x[i-1], x[i], x[i+1] of the shared row routines (read when the
                            // mesh is not uniform, each behind the test that the node exists)
                            const double* xv = a.xs + ((ptrdiff_t)3 * (in ? j : 0) + 1 - (in ? i : 0));
                            double gi = 0.0;
                            if (k == 0) {                                              // u is u^n: g = M u^n + dt F (:746)
                                if (in) gi = rom_mass_rhs_node(xv, i, N, um, u0, ur, H.fdt[j], h, a.nonuniform);
                                H.g[j] = gi;
                            } else {
                                gi = H.g[j];
                            }
                            const MeshConst mc = make_mesh_const(h, a.dt, a.E, a.supg);
                            double lo, di, up, R_i;
                            rom_assemble_row(i, N, um, u0, ur, gi, (in && i > 0) ? H.hl[j] : 0.0, (in && i < N - 1) ? H.hr[j] : 0.0, mu1, mc,
                                             a.nonuniform, xv, a.dt, a.E, lo, di, up, R_i);
                            const double wj = H.w[j];
                            *reinterpret_cast<double2*>(&s_cf[q4][0]) = make_double2(wj * lo, wj * di);
                            *reinterpret_cast<double2*>(&s_cf[q4][2]) = make_double2(wj * up, wj * R_i);
                        }
                    }
                    __syncthreads();                                          // the slab's coefficients are in LDS
                    // ---- projection: steps of 16 sampled rows; lane (k, blk, t): row 16 st + 4 k + blk, columns NB t + c ----------
#pragma unroll 1
                    for (int st = 0; st < HS / 16; ++st) {
                        const int rl = 16 * st + 4 * pk + pblk;
                        const double2 c01 = *reinterpret_cast<const double2*>(&s_cf[rl][0]);
                        const double2 c23 = *reinterpret_cast<const double2*>(&s_cf[rl][2]);
                        double Y[NB], P[NB];
                        stream_row_operands<NB, PS>(s_P + 3 * rl * PS + NB * pt, c01, c23, Y, P);
                        const double X = (pt == 0) ? c23.y : 0.0;             // extra B block [R, 0, 0, 0] (no Phi^T u here)
                        stream_step_mfma<K, GAL, W>(Y, P, X, acc);
                    }
                }
                __syncthreads();                               // the last slab's rows are no longer read (the system is parked over them)
                stream_park<K, GAL, W>(acc, S, lane);
                __syncthreads();
                // ---- solve(Ar, -br) (:767), q <- q + dq, err = |dq| / |q|  (:770-776) -------------------------------------------
                double nd, nq;
                if constexpr (HyperDims<K>::per_lane == 1) {
                    const double qk = (lane < step_width()) ? s_q[lane] : 0.0;    // read before the solve's first barrier
                    K::template solve_add<PIV, W>(L, step_width(), lane, qk, aborted, info_out, nd, nq);
                } else {
                    const double qk0 = (lane < step_width()) ? s_q[lane] : 0.0, qk1 = (64 + lane < step_width()) ? s_q[64 + lane] : 0.0;
                    if constexpr (PIV) K::template solve_add_pivoted<GAL, W>(L, step_width(), lane, qk0, qk1, info_out, nd, nq);
                    else K::template solve_add<GAL, W>(L, step_width(), lane, qk0, qk1, a.force_pivoted != 0, aborted, nd, nq);
                }
                nd = sqrt(nd); nq = sqrt(nq);
                const double err = nd / nq;
                ++k;
                const bool more = (err > a.tol) && (k < a.max_it) && info_out == 0 && !aborted;
                if (!(err - err == 0.0)) flags |= BG_FLAG_NONFINITE;
                if (k >= a.max_it) flags |= BG_FLAG_HIT_CAP;
                __syncthreads();
                if (!more) break;
            }
            if (aborted) break;
            // ---- the reduced coordinates of U[:, n+1] = Phi q (:779) ---------------------------------------------------------
            if (tid < a.r) qhist[(size_t)(step + 1) * a.r + tid] = s_q[tid];
            if (tid == 0) a.iters[(size_t)smp * a.nsteps + step] = k;
        }
        if (tid == 0) {
            a.flags[smp] = flags;
            a.info[smp] = aborted ? BG_INFO_NEEDS_PIVOTING : info_out;
        }
    }
}

// The repair kernel (PIV) keeps one workgroup per CU: its one-wave pivoted solve holds a 41-double row per lane.
template <bool GAL, bool PIV>
__global__ __launch_bounds__(256, PIV ? 1 : HWG_PER_CU) void rom_hyper_kernel(HyperRunArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_slab[2 * HSLAB];             // two slab buffers; later the system
    __shared__ double s_g[HMMAX], s_fdt[HMMAX], s_hl[HMMAX], s_hr[HMMAX], s_w[HMMAX];
    __shared__ int s_row[HMMAX];
    __shared__ __attribute__((aligned(16))) double s_cf[HS][4];                   // weighted lo, di, up, R per row of the slab
    __shared__ __attribute__((aligned(16))) double s_q[LR];
    __shared__ int s_bad[8];                                                      // [4] guard of each wave, [4] info of the pivoted solve
    static_assert(sizeof(double) * (2 * HSLAB + 5 * HMMAX + 4 * HS + LR) + 4 * HMMAX + 32 <= 160 * 1024 / HWG_PER_CU, "LDS per workgroup");
    static_assert(HMMAX % HS == 0 && HS % 16 == 0 && HS <= 64, "whole slabs of whole 16-row steps, at most one row per quad");
    // over the dead slabs: the system [LR][LSW], then the multipliers of two panels, the diagonal, y and x
    double* const s_m = s_slab + LR * LSW;
    double* const s_diag = s_m + 512;
    static_assert(LR * LSW + 512 + 3 * 64 <= 2 * HSLAB, "the solve's arrays fit over the slabs");
    const StreamLds L{s_slab, nullptr, nullptr, nullptr, nullptr, s_cf, s_q, s_m, s_diag, s_diag + 64, s_diag + 128, s_bad, nullptr};
    const HyperLds H{s_g, s_fdt, s_hl, s_hr, s_w, s_row, nullptr, nullptr, nullptr};
    switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {       // wave-uniform by construction
        case 0: hyper_body<GAL, PIV, 0>(a, L, H); break;
        case 1: hyper_body<GAL, PIV, 1>(a, L, H); break;
        case 2: hyper_body<GAL, PIV, 2>(a, L, H); break;
        default: hyper_body<GAL, PIV, 3>(a, L, H); break;
    }
}

// The argument checks of bg_hyper_rom_run and bg_hyper_rom_run_wide (bases of up to r_max modes on up to m_max sampled rows) and
// the kernel's arguments, as stream_run_args for the streaming loops.  BG_OK with B == 0 means there is nothing to launch.
inline int hyper_run_args(HyperRunArgs& a, int r_max, int m_max, int N, int B, int r, int m, int nsteps, int projection,
                          const int32_t* rows, const double* xi, const double* xs, const double* PhiS, const double* q0, const double* u0s,
                          const double* mu1, const double* mu2, double dt, double E, double tol, int max_it, int options, double* qhist,
                          int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order)
{
    if (N < 3 || B < 0 || r < 1 || m < 1 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (projection != BG_PROJ_GALERKIN && projection != BG_PROJ_LSPG) return BG_ERR_PROJECTION;
    if (N > bg_fom_max_n()) return BG_ERR_UNSUPPORTED_N;
    if (r > r_max || m > m_max) return BG_ERR_UNSUPPORTED_R;
    if (m > N) return BG_ERR_BAD_ARG;
    if (B == 0) return BG_OK;
    if (!rows || !xi || !xs || !PhiS || !q0 || !u0s || !mu1 || !mu2 || !qhist || !flags || !info || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    if ((uintptr_t)PhiS & 15) return BG_ERR_BAD_ARG;
    a.rows = rows; a.xi = xi; a.xs = xs; a.PhiS = PhiS; a.q0 = q0; a.u0s = u0s; a.mu1 = mu1; a.mu2 = mu2; a.qhist = qhist;
    a.iters = iters; a.flags = flags; a.info = info; a.order = order;
    a.dt = dt; a.E = E; a.tol = tol; a.N = N; a.B = B; a.r = r; a.m = m; a.nsteps = nsteps; a.max_it = max_it;
    a.supg = options & BG_OPT_SUPG; a.nonuniform = (options & BG_OPT_NONUNIFORM) ? 1 : 0;
    a.force_pivoted = (options & BG_OPT_FORCE_PIVOTED) ? 1 : 0;
    return BG_OK;
}

}  // namespace

#if !defined(BG_ROM_HYPER_LOCAL_TU) && !defined(BG_ROM_HYPER_WIDE_TU) && !defined(BG_ROM_HYPER_BLOCKED_TU)
extern "C" {

int bg_hyper_rom_limits(int* max_r, int* max_m)
{
    if (!max_r || !max_m) return BG_ERR_BAD_ARG;
    *max_r = LR;
    *max_m = HMMAX;
    return BG_OK;
}

// doubles of the packed stencil table bg_hyper_rom_run reads: three rows of 42 per sampled row, m rounded up to 32 (any r <= 40)
long long bg_hyper_rom_table_elems(int m, int r)
{
    if (m < 1 || m > HMMAX || r < 1 || r > LR) return 0;
    return (long long)((m + HS - 1) / HS) * HSLAB;
}

int bg_hyper_rom_run(int N, int B, int r, int m, int nsteps, int projection, const int32_t* rows, const double* xi, const double* xs,
                     const double* PhiS, const double* q0, const double* u0s, const double* mu1, const double* mu2, double dt, double E,
                     double tol, int max_it, int options, double* qhist, int32_t* iters, int32_t* flags, int32_t* info,
                     const int32_t* order, void* stream)
{
    HyperRunArgs a;
    const int rc = hyper_run_args(a, LR, HMMAX, N, B, r, m, nsteps, projection, rows, xi, xs, PhiS, q0, u0s, mu1, mu2, dt, E, tol, max_it,
                                  options, qhist, iters, flags, info, order);
    if (rc != BG_OK || B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        return launch_fast_then_repair(B, HWG_PER_CU, a.force_pivoted != 0, [&](auto piv, int grid) {
            hipLaunchKernelGGL((rom_hyper_kernel<decltype(p)::galerkin, decltype(piv)::value>), dim3(grid), dim3(256), 0, st, a);
        });
    });
}

}  // extern "C"
#endif  // none of BG_ROM_HYPER_LOCAL_TU, BG_ROM_HYPER_WIDE_TU, BG_ROM_HYPER_BLOCKED_TU
