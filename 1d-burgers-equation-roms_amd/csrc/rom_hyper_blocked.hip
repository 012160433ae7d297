// rom_hyper_blocked.hip -- bg_hyper_rom_run_blocked: the HYPER-REDUCED POD-PROM time loop of one sample on one compute unit for
// the thesis' FINEST bases, 96 < r <= 256 (r = 160 and 227: POD/modes/U_modes_tol_1e-05.npy, _1e-06.npy), on up to 1024 sampled
// mesh rows.  reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785, with the sums over mesh rows restricted to m
// sampled rows and weighted (bg_hyper_rom_run's semantics, rom_hyper.hip).
//
// The arithmetic is bg_rom_run_blocked's (rom_blocked.hip, rom_blocked_device.hpp): the padded system Ar | br is a grid of
// 16 x 16 tiles in a per-workgroup slot of a caller-provided workspace, the tiles are dealt to the four waves, every wave sweeps
// the rows for its own tiles on v_mfma_f64_16x16x4, HBT tiles per wave and sweep, and the system is solved there by the blocked
// guarded pivot-free Gauss-Jordan over 16-column panels.  What is swept is the table of sampled rows instead of the mesh:
//   lift     the stencil state u_{i-1}, u_i, u_{i+1} = PhiS q of every sampled row: 16 lanes per row, three 16-lane DPP sums.  The
//            very first iteration of a run reads u0s instead (the reference starts from u0, not from Phi Phi^T u0).
//   assembly one slab of 8 sampled rows at a time, by 8 threads, a slab ahead of the matrix instructions: A(u), R(u) of the row
//            (rom_assemble_row, reading the stencil coordinates xs as a three-node mesh), in the first iteration of a step also
//            g_i = (M u^n + dt F)_i from the same stencil (rom_mass_rhs_node).  The weight goes into the coefficients: lo, di, up,
//            R times xi (Galerkin) or sqrt(xi) (LSPG), so the matrix instructions are the unweighted loop's.  Only the slab's
//            coefficients are kept (two buffers of 8 x 4 doubles): with them per row m = 1024 would not fit.
//   projection  thread c loads column c of the three table rows of each sampled row of the NEXT slab into registers while the
//            matrix instructions of this one run, then writes Phi[i] and Y = lo Phi[i-1] + di Phi[i] + up Phi[i+1] of its column
//            into the other LDS buffer; the extra tile column carries [R, 0 ...] (no Phi^T u: the update is q <- q + dq).
//   solve    blocked_solve; a multiplier above 1 below the pivot marks the sample BG_INFO_NEEDS_PIVOTING and ends it (the caller
//            redoes it), an exactly zero pivot over a zero column gives info = k + 1.  There is no repair kernel.
// Then q <- q + dq and the stopping test |dq| / |q|.  The output is q itself, [B][nsteps + 1][r]; there is no lift-only sweep and
// no vector of mesh length anywhere: 3 <= N <= bg_fom_max_n().
//
// The table is PhiS [MPAD][3][RP], MPAD = m rounded up to 8, RP = r rounded up to 16 (at most 6 MB, L2 / Infinity Cache resident,
// shared by all samples).  LDS at m = 1024, one workgroup per compute unit:
//   slab buffers / panels of the solve   8 976 doubles    71 808 B
//   g, dt F, h_f left and right, weight  5 x 1024 doubles 40 960 B
//   mesh row of every sampled row        1024 ints         4 096 B
//   stencil state                        1024 x 3 doubles 24 576 B
//   q, dq                                2 x 256 doubles   4 096 B
//   items and tiles                      2 x 272 ints      2 176 B
//   two slabs' coefficients, norms, zero pivot               584 B
//                                                        148 296 B of 163 840 B (148 552 B as the compiler lays them out)
#define BG_ROM_HYPER_BLOCKED_TU
#include "rom_hyper.hip"

#include "abi_common.hpp"
#include "rom_blocked_device.hpp"

namespace {

constexpr int HBMMAX = 1024;           // sampled rows held
// Accumulator tiles per wave and sweep.  rom_blocked_kernel's BT = 38 does not fit here: the loader holds three table rows per
// sampled row of a slab (48 registers against its 20), and with 36 tiles the Galerkin kernel already spills to scratch.  At 35
// neither kernel uses scratch (the Galerkin one parks 4 VGPRs in AGPRs: 35 is the edge).  The number of sweeps is BT's for
// every width but LSPG with 241 <= r <= 256 (152 items: two sweeps).
constexpr int HBT = 35;

struct HyperBlockedRunArgs : HyperRunArgs {   // PhiS: [MPAD][3][RP]
    double* work;           // [slots][RP][RP + 16]
    long long work_elems;
    int RP, MPAD;
};

template <bool GAL>
__global__ __launch_bounds__(256, 1) void rom_hyper_blocked_kernel(HyperBlockedRunArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_reg[BREGION];   // slab buffers (projection) / panels (solve)
    __shared__ double s_g[HBMMAX], s_fdt[HBMMAX], s_hl[HBMMAX], s_hr[HBMMAX], s_w[HBMMAX];
    __shared__ int s_row[HBMMAX];                                     // mesh row (N beyond m: an identity row with weight 0)
    __shared__ double s_us[HBMMAX][3];                                // u at the stencil nodes i - 1, i, i + 1 of every sampled row
    __shared__ __attribute__((aligned(16))) double s_cf[2][BSR][4];  // weighted lo, di, up, R per row of this slab and the next
    __shared__ double s_q[BMAX_R], s_dq[BMAX_R];
    __shared__ double s_red[2][4];
    __shared__ int s_item[BMAXITEMS];
    __shared__ int s_tile[BMAXITEMS];
    __shared__ int s_zero;
    static_assert(sizeof(double) * (BREGION + 5 * HBMMAX + 3 * HBMMAX + 2 * BSR * 4 + 2 * BMAX_R + 8) + 4 * (HBMMAX + 2 * BMAXITEMS + 1)
                  <= 160 * 1024, "LDS per workgroup");
    static_assert(HBMMAX % BSR == 0, "whole slabs");

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, m = a.m, r = a.r, RP = a.RP, NB = RP / 16, MW = RP + 16, MPAD = a.MPAD;
    const int nslab = MPAD / BSR;
    double* const M = a.work + (size_t)blockIdx.x * (size_t)a.work_elems;
    const int loff = (lane >> 4) * BSPS + (lane & 15);          // a lane's operand of a 16x16x4 step within a section
    // the spacing of a uniform mesh from the outermost stencil nodes, as hyper_body takes it
    const int i_first = a.rows[0], i_last = a.rows[m - 1];
    const int lo_off = i_first > 0 ? 0 : 1, hi_off = i_last < N - 1 ? 2 : 1;
    const double h = (a.xs[3 * (m - 1) + hi_off] - a.xs[lo_off]) / (double)((i_last + hi_off) - (i_first + lo_off));

    const int nitems = blocked_item_count<GAL, false>(NB);
    blocked_fill_items<GAL>(s_item, s_tile, nitems, NB, tid);
    // ---- per-row constants of the sampling, the same for every sample ----------------------------------------------------
    for (int j = tid; j < MPAD; j += 256) {
        const double xi = (j < m) ? a.xi[j] : 0.0;
        s_row[j] = (j < m) ? a.rows[j] : N;
        s_w[j] = GAL ? xi : sqrt(xi);
    }

    for (int slot = blockIdx.x; slot < a.B; slot += gridDim.x) {
        const int smp = a.order ? a.order[slot] : slot;
        if (smp < 0 || smp >= a.B) continue;                     // workgroup-uniform
        const double mu1 = a.mu1[smp], mu2 = a.mu2[smp];
        double* qhist = a.qhist + (size_t)smp * (size_t)(a.nsteps + 1) * (size_t)r;
        const double* u0s = a.u0s + (size_t)smp * (size_t)m * 3;
        __syncthreads();
        // ---- per-sample constants (compute_forcing_vector :427-461, f_gp of :556-558) and the initial coordinates -------
        for (int j = tid; j < MPAD; j += 256) {
            double fdt = 0.0, hl = 0.0, hr = 0.0;
            if (j < m) hyper_row_forcing(a.xs[3 * j], a.xs[3 * j + 1], a.xs[3 * j + 2], s_row[j], N, mu2, h, a.nonuniform, a.dt, fdt, hl, hr);
            s_fdt[j] = fdt; s_hl[j] = hl; s_hr[j] = hr;
        }
        if (tid < BMAX_R) {
            const double q = (tid < r) ? a.q0[(size_t)smp * r + tid] : 0.0;
            s_q[tid] = q;
            if (tid < r) qhist[tid] = q;
        }
        __syncthreads();

        int flags = 0, info_out = 0;
        bool aborted = false;

        for (int step = 0; step < a.nsteps && info_out == 0 && !aborted; ++step) {
            int k = 0;
            while (true) {
                // ---- the stencil of u = PhiS q (:773) of every sampled row: 16 lanes per row; the first iteration of a run
                // assembles at u0 itself (:725)
                if (step > 0 || k > 0) {
                    const int c16 = lane & 15;
                    for (int j = 4 * w + (lane >> 4); j < MPAD; j += 16) {      // (wave-uniform: MPAD is a multiple of 4)
                        const double* prow = a.PhiS + (size_t)3 * j * RP + c16;
                        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
                        for (int b = 0; b < 16; ++b)
                            if (b < NB) {
                                const double qb = s_q[16 * b + c16];
                                s0 = __builtin_fma(prow[16 * b], qb, s0);
                                s1 = __builtin_fma(prow[RP + 16 * b], qb, s1);
                                s2 = __builtin_fma(prow[2 * RP + 16 * b], qb, s2);
                            }
                        s0 += dpp_mov<0x111>(s0); s1 += dpp_mov<0x111>(s1); s2 += dpp_mov<0x111>(s2);      // row_shr 1, 2, 4, 8:
                        s0 += dpp_mov<0x112>(s0); s1 += dpp_mov<0x112>(s1); s2 += dpp_mov<0x112>(s2);      // lane 15 of the row holds
                        s0 += dpp_mov<0x114>(s0); s1 += dpp_mov<0x114>(s1); s2 += dpp_mov<0x114>(s2);      // the sums
                        s0 += dpp_mov<0x118>(s0); s1 += dpp_mov<0x118>(s1); s2 += dpp_mov<0x118>(s2);
                        if (c16 == 15) { s_us[j][0] = s0; s_us[j][1] = s1; s_us[j][2] = s2; }
                    }
                } else {
                    for (int e = tid; e < 3 * MPAD; e += 256) (&s_us[0][0])[e] = (e < 3 * m) ? u0s[e] : 0.0;
                }
                __syncthreads();
                // A(u), R(u) of the rows of one slab into s_cf[slab & 1], by the threads 0 .. 7; `first`: u is u^n and g is not
                // formed yet (the first sweep of the first iteration of a step)
                auto assemble = [&](int slab, bool first) {
                    if (tid < BSR) {
                        const int j = slab * BSR + tid;
                        const int i = s_row[j];
                        const bool in = i < N;
                        double um = s_us[j][0], u0 = s_us[j][1], ur = s_us[j][2];
                        if (i == 0) um = 0.0;                                      // slots outside the mesh are ignored
                        if (i + 1 >= N) ur = 0.0;
                        // the stencil coordinates as the x[i-1], x[i], x[i+1] of the shared row routines (read when the mesh is
                        // not uniform, each behind the test that the node exists)
                        const double* xv = a.xs + ((ptrdiff_t)3 * (in ? j : 0) + 1 - (in ? i : 0));
                        double gi = 0.0;
                        if (first) {                                               // g = M u^n + dt F (:746)
                            if (in) gi = rom_mass_rhs_node(xv, i, N, um, u0, ur, s_fdt[j], h, a.nonuniform);
                            s_g[j] = gi;
                        } else {
                            gi = s_g[j];
                        }
                        const MeshConst mc = make_mesh_const(h, a.dt, a.E, a.supg);
                        double lo, di, up, R_i;
                        rom_assemble_row(i, N, um, u0, ur, gi, (in && i > 0) ? s_hl[j] : 0.0, (in && i < N - 1) ? s_hr[j] : 0.0, mu1, mc,
                                         a.nonuniform, xv, a.dt, a.E, lo, di, up, R_i);
                        const double wj = s_w[j];
                        *reinterpret_cast<double2*>(&s_cf[slab & 1][tid][0]) = make_double2(wj * lo, wj * di);
                        *reinterpret_cast<double2*>(&s_cf[slab & 1][tid][2]) = make_double2(wj * up, wj * R_i);
                    }
                };
                // ---- projection: sweeps over the sampled rows, HBT tiles per wave and sweep ----------------------------------
                for (int base = 0; base < nitems; base += 4 * HBT) {
                    const int left = nitems - base - w;
                    const int mine = left > 0 ? (left + 3) / 4 : 0;      // this wave's items in the sweep: base + 4 t + w
                    const bool first = k == 0 && base == 0;
                    f64x4 acc[HBT];
#pragma unroll
                    for (int t = 0; t < HBT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
                    // thread c stages column c of the three table rows of every sampled row of a slab
                    double pf[BSR][3];
                    const bool scol = tid < RP;
                    auto fetch = [&](int slab) {
                        const double* src = a.PhiS + (size_t)3 * slab * BSR * RP + tid;
#pragma unroll
                        for (int l = 0; l < BSR; ++l)
#pragma unroll
                            for (int s = 0; s < 3; ++s) pf[l][s] = scol ? src[(size_t)(3 * l + s) * RP] : 0.0;
                    };
                    // slab -1: only the fetch and the assembly of slab 0 (one site for both, so that they are inlined once)
                    for (int slab = -1; slab < nslab; ++slab) {
                        double* const buf = s_reg + (slab & 1) * BBUF;
                        if (slab >= 0) {
                            const double (*cf)[4] = s_cf[slab & 1];
                            if (scol) {
#pragma unroll
                                for (int l = 0; l < BSR; ++l) {
                                    const double2 c01 = *reinterpret_cast<const double2*>(&cf[l][0]);
                                    const double up = cf[l][2];
                                    buf[l * BSPS + tid] = pf[l][1];
                                    buf[BSEC + l * BSPS + tid] = __builtin_fma(up, pf[l][2], __builtin_fma(c01.y, pf[l][1], c01.x * pf[l][0]));
                                }
                            }
                            if (tid < 16) {
#pragma unroll
                                for (int l = 0; l < BSR; ++l) buf[BSEC + l * BSPS + BMAX_R + tid] = tid == 0 ? cf[l][3] : 0.0;
                            }
                        }
                        if (slab + 1 < nslab) {
                            fetch(slab + 1);                   // lands while the matrix instructions below run
                            assemble(slab + 1, first);         // into the other coefficient buffer, last read before the barrier of slab - 1
                        }
                        __syncthreads();
                        if (slab >= 0) blocked_slab_steps(acc, buf, s_item, base, w, mine, loff);
                    }
                    blocked_store_tiles<GAL, false>(acc, s_tile, base, w, mine, lane, M, MW, RP, r, nullptr);
                    __syncthreads();                           // slab buffers free for the next sweep; the tiles are stored
                }
                // ---- solve(Ar, -br) (:767) ------------------------------------------------------------------------------------
                bool bad;
                int zstep;
                blocked_solve(M, MW, RP, NB, s_reg, s_dq, tid, lane, w, bad, zstep);
                if (w == 0 && lane == 0) s_zero = zstep;
                const bool anybad = __syncthreads_or(bad) != 0;
                const bool tripped = anybad || a.force_pivoted;                        // workgroup-uniform
                if (tripped) aborted = true;
                else if (s_zero >= 0) info_out = s_zero + 1;                            // exactly singular (LAPACK info)
                // ---- q <- q + dq, err = |dq| / |q|  (:770-776) ----------------------------------------------------------------
                double dq = 0.0, qn = 0.0;
                if (tid < r) { dq = s_dq[tid]; qn = s_q[tid] + dq; }
                {
                    const double nd = wave_sum(dq * dq), nq = wave_sum(qn * qn);
                    if (lane == 0) { s_red[0][w] = nd; s_red[1][w] = nq; }
                }
                __syncthreads();
                const double nd = sqrt((s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]));
                const double nq = sqrt((s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]));
                const double err = nd / nq;
                ++k;
                const bool more = (err > a.tol) && (k < a.max_it) && !aborted && info_out == 0;
                if (!(err - err == 0.0)) flags |= BG_FLAG_NONFINITE;
                if (k >= a.max_it) flags |= BG_FLAG_HIT_CAP;
                if (tid < BMAX_R) s_q[tid] = qn;
                __syncthreads();
                if (!more) break;
            }
            if (aborted) break;
            // ---- the reduced coordinates of U[:, n+1] = Phi q (:779) ---------------------------------------------------------
            if (tid < r) qhist[(size_t)(step + 1) * r + tid] = s_q[tid];
            if (tid == 0) a.iters[(size_t)smp * a.nsteps + step] = k;
        }
        if (tid == 0) {
            a.flags[smp] = flags;
            a.info[smp] = aborted ? BG_INFO_NEEDS_PIVOTING : info_out;
        }
    }
}

}  // namespace

extern "C" {

int bg_hyper_rom_blocked_limits(int* max_r, int* max_m)
{
    if (!max_r || !max_m) return BG_ERR_BAD_ARG;
    *max_r = BMAX_R;
    *max_m = HBMMAX;
    return BG_OK;
}

// doubles of the packed stencil table bg_hyper_rom_run_blocked reads: three rows of RP per sampled row, m rounded up to 8
long long bg_hyper_rom_blocked_table_elems(int m, int r)
{
    if (m < 1 || m > HBMMAX || r < 1 || r > BMAX_R) return 0;
    return (long long)3 * (((m + BSR - 1) / BSR) * BSR) * blocked_rp(r);
}

// doubles of one workspace slot: the padded system [RP][RP + 16] (Ar, then -br and 15 zero columns)
long long bg_hyper_rom_blocked_work_elems(int r)
{
    if (r < 1 || r > BMAX_R) return 0;
    const long long RP = blocked_rp(r);
    return RP * (RP + 16);
}

int bg_hyper_rom_run_blocked(int N, int B, int r, int m, int nsteps, int projection, const int32_t* rows, const double* xi,
                             const double* xs, const double* PhiS, const double* q0, const double* u0s, const double* mu1,
                             const double* mu2, double dt, double E, double tol, int max_it, int options, double* work, int slots,
                             double* qhist, int32_t* iters, int32_t* flags, int32_t* info, const int32_t* order, void* stream)
{
    if (options & BG_OPT_PIVOT_ON_DEVICE) return BG_ERR_BAD_ARG;      // this loop has no repair kernel
    HyperBlockedRunArgs a;
    const int rc = hyper_run_args(a, BMAX_R, HBMMAX, N, B, r, m, nsteps, projection, rows, xi, xs, PhiS, q0, u0s, mu1, mu2, dt, E, tol,
                                  max_it, options, qhist, iters, flags, info, order);
    if (rc != BG_OK || B == 0) return rc;
    if (!work || slots < 1) return BG_ERR_WORKSPACE;
    a.work = work; a.work_elems = bg_hyper_rom_blocked_work_elems(r);
    a.RP = blocked_rp(r); a.MPAD = ((m + BSR - 1) / BSR) * BSR;
    const int grid = B < slots ? B : slots;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_projection(projection, [&](auto p) {
        hipLaunchKernelGGL((rom_hyper_blocked_kernel<decltype(p)::galerkin>), dim3(grid), dim3(256), 0, st, a);
        return check_launch();
    });
}

}  // extern "C"
