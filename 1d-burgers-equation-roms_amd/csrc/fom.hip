// fom.hip -- fused batched FOM time-stepper for gfx950 and its C-ABI entry points.
//
// Replaces the body of FEMBurgers.fom_burgers (reference FEM/fem_burgers.py:646-707):
// one wavefront (N <= 1536) or one 256-thread workgroup (N <= 8192) integrates one (mu1, mu2)
// sample through all time steps and all Picard iterations; the state never leaves registers
// between iterations, HBM sees one coalesced row write per time step.
//
// The time loop, the diagnostic assembly and the diagnostic solve are each written once, over a
// topology (fom_sample, assemble_sample, solve_sample; WaveTopo / WgTopo of fom_wide.hpp).  The six
// kernels only find their sample, build the topology and call the body.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "fom_device.hpp"
#include "fom_wide.hpp"

namespace bg {
thread_local int tls_last_hip_error = 0;
}

namespace {

using namespace bg;

struct FomArgs {
    const double* x;
    const double* u0;
    const double* mu1;
    const double* mu2;
    double* hist;
    int32_t* iters;
    int32_t* flags;
    double dt, E, tol2;
    int N, B, nsteps, max_it, supg;
    double* errs;        // [B][nsteps][max_it], TRACE instantiations only: the error of every Picard iteration
};

constexpr int WAVES_PER_WG = 4;

// rows >= N read as `pad` (unless `full`: every row exists) and are not written
template <int R>
__device__ __forceinline__ void load_rows(const double* __restrict__ src, int N, int row0, bool full,
                                          double (&u)[R], double pad = 0.0)
{
#pragma unroll
    for (int j = 0; j < R; ++j) u[j] = (full || row0 + j < N) ? src[row0 + j] : pad;
}

template <int R>
__device__ __forceinline__ void store_rows(double* __restrict__ dst, int N, int row0, bool full,
                                           const double (&u)[R])
{
#pragma unroll
    for (int j = 0; j < R; ++j)
        if (full || row0 + j < N) dst[row0 + j] = u[j];
}

// ---- one sample over a topology (WaveTopo / WgTopo, fom_wide.hpp); the kernels below only choose s and the topology ----
// The whole time loop of sample s; every branch is uniform over the sample's threads (a wave or a workgroup), which
// all see the same sums.
// TRACE: also store error_U = ||dU|| / ||U1|| of every iteration (what the reference prints at :664); a separate
// instantiation, so that the hot kernel carries no trace of it.
// PARK (workgroup form, uniform mesh, 32 rows per thread): g and hfs live in LDS (*park) instead of 128 VGPRs per thread.
template <int R, bool FULL, bool UNI, bool TRACE, bool PARK, class Topo>
__device__ __forceinline__ void fom_sample(const FomArgs& a, Topo& tp, int s, WidePark<PARK ? R : 1>* park)
{
    static_assert(UNI || !PARK, "only the uniform assembly reads g and hfs through accessors");
    const int N = a.N, t = tp.g, row0 = t * R;
    const double h = (a.x[N - 1] - a.x[0]) / (double)(N - 1);
    const MeshConst c = make_mesh_const(h, a.dt, a.E, a.supg);
    const double mu1 = a.mu1[s], mu2 = a.mu2[s];

    double hfs[PARK ? 1 : R], fdt[R], u[R], g[PARK ? 1 : R];
    ElemGeom<UNI ? 0 : R> gm;
    if constexpr (PARK) {
        double hf[R];
        forcing_setup<R>(a.x, N, row0, mu2, c.h, a.dt, hf, fdt);
#pragma unroll
        for (int j = 0; j < R; ++j) park->hfs[j][t] = hf[j];
    } else if constexpr (UNI) {
        forcing_setup<R>(a.x, N, row0, mu2, c.h, a.dt, hfs, fdt);
    } else {
        geom_setup<R>(a.x, N, row0, a.dt, a.E, gm);
        forcing_setup_general<R>(a.x, N, row0, mu2, a.dt, hfs, fdt);
    }
    // g and hfs of local row j, where they live
    auto g_put = [&](int j, double v) { if constexpr (PARK) park->g[j][t] = v; else g[j] = v; };
    auto g_at = [&](int j) { if constexpr (PARK) return park->g[j][t]; else return g[j]; };
    auto hf_at = [&](int j) { if constexpr (PARK) return park->hfs[j][t]; else return hfs[j]; };

    double* hist = a.hist + (size_t)s * (size_t)(a.nsteps + 1) * (size_t)N;
    load_rows<R>(a.u0 + (size_t)s * N, N, row0, FULL, u);
    store_rows<R>(hist, N, row0, FULL, u);

    // ROT (BG_PICARD_ROTATE, topologies with rotates_picard): the loop is rotated by half an assembly.  assemble_head of an
    // iterate (halo, off-diagonals, SUPG terms) reads u, hfs and the mesh constants only, so it is formed right after the
    // update that makes the iterate, in the block of sum2 and the stopping test: with one wave per SIMD nothing else can
    // issue between the reduction's dependent rounds (on a uniform mesh the two are woven by hand, below; a graded mesh
    // has the head, then sum2).  Whichever way the test goes the head is the one needed next, by the next iteration or,
    // with the new g, by the first iteration of the next time step, which starts from the same u; only the head after a
    // sample's last step is dropped.  Every value is formed by the same operations in the same order as without the
    // rotation: histories, counts and flags are bit for bit those of -DBG_PICARD_ROTATE=0.  The TRACE instantiations
    // take the same form.
    constexpr bool ROT = BG_PICARD_ROTATE && Topo::rotates_picard;
    static_assert(!ROT || !PARK, "the parked form belongs to the workgroup topology");
    double huL, huR, hse[ROT ? R : 1], hlo[ROT ? R : 1], hup[ROT ? R : 1];   // ROT: the head of the coming iteration
    auto head = [&]() {
        if constexpr (ROT) {
            if constexpr (UNI) assemble_head<R>(tp, c, u, hf_at, huL, huR, hse, hlo, hup);
            else assemble_general_head<R>(tp, gm, a.dt, u, hfs, huL, huR, hse, hlo, hup);
        }
    };
    head();

    // Lean iterations (BG_PICARD_LEAN).  Far from convergence an iteration solves A v = b for the new iterate itself: the
    // three FMAs per row of A u in the right-hand side are not issued (assemble_p2, ITER), and du = v - u serves the stopping
    // norm only.  Such a solve is as accurate as the pivot-free solver, 1e-15 |u| to 1e-14 |u|, and unlike the solve for the
    // increment not corrected below that by the iteration after it, so a time step should not END on one.  A step
    // therefore runs in two loops, each a straight body: lean iterations while the stopping test is missed by more than
    // BG_PICARD_LEAN_FACTOR in the error (its square in the norms), then iterations for the increment until the test is met
    // or the cap reached; the history keeps the accuracy of the increment form.  Every step starts lean, whatever the step
    // before it did: a step is a function of its initial state alone, so a run restarted from a stored time level repeats
    // the original bit for bit.  A lean iteration ends a step only where the error falls by more than the factor in one
    // iteration (a step's first included: a step that converges at once), or at the cap; the step's result is then the
    // solver's, off by 1e-15 relative, and counted and flagged like any other.  Every branch derives from the sums all
    // threads of the sample hold, so it is uniform.
    // The second loop body costs registers.  It is left out where the kernel has none to give: the parked form, and a
    // graded mesh at 24 or more rows per thread, which spills as it is (profiles/iterate_form_resources.tsv).
    constexpr bool LEANS = BG_PICARD_LEAN && !PARK && (UNI || R < 24);
    constexpr double lean2 = BG_PICARD_LEAN_FACTOR * BG_PICARD_LEAN_FACTOR;
    int flags = 0;
    for (int step = 0; step < a.nsteps; ++step) {
        if constexpr (UNI) mass_rhs<R, FULL>(tp, c, N, u, fdt, g_put);
        else mass_rhs_general<R>(tp, gm, N, u, fdt, g);
        int k = 0;
        bool more = true, far = LEANS;
        auto iteration = [&](auto lean_c) __attribute__((always_inline)) {
            constexpr bool LEAN = decltype(lean_c)::value;
            double lo[R], di[R], up[R], rhs[R];
            if constexpr (ROT) {
#pragma unroll
                for (int j = 0; j < R; ++j) { lo[j] = hlo[j]; up[j] = hup[j]; }
                if constexpr (UNI) assemble_tail<R, FULL, LEAN>(tp, c, N, mu1, u, g_at, huL, huR, hse, lo, di, up, rhs);
                else assemble_general_tail<R, LEAN>(tp, gm, a.dt, c.kap, N, mu1, u, g, huL, huR, hse, lo, di, up, rhs);
            } else {
                if constexpr (UNI) assemble<R, FULL, LEAN>(tp, c, N, mu1, u, g_at, hf_at, lo, di, up, rhs);
                else assemble_general<R, LEAN>(tp, gm, a.dt, c.kap, N, mu1, u, g, hfs, lo, di, up, rhs);
            }
            // The solve leaves the last multiply of its rows j < R-1 open, x_j = rhs[j] * di[j] (wang_finish).  LEAN: x is the
            // new iterate, du_j = x_j - u_j is one FMA of the two factors, formed while u_j is still the old iterate, and
            // x_j then takes u_j's registers with no move.  Otherwise x is the increment.
            // Contraction is off here: the next assembly adds to the product x_j (LEAN) or to the sum u_j + x_j, and left to
            // itself the compiler fuses those, so that the assembly reads an unrounded iterate where the history holds the
            // rounded one; which sums it fuses differs between the instantiations, and traced and untraced runs, which
            // must agree bit for bit, then differ in the last place.
            // A kernel without the lean loop keeps the whole solve and the update as they were: its listing is unchanged.
            tp.template solve<R, !LEANS>(lo, di, up, rhs);
            double nd = 0.0, nu = 0.0;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if constexpr (!LEANS) {
                    u[j] += rhs[j];
                    nd = __builtin_fma(rhs[j], rhs[j], nd);
                    nu = __builtin_fma(u[j], u[j], nu);
                } else {
#pragma clang fp contract(off)
                    double d;
                    if constexpr (LEAN) {
                        d = (j < R - 1) ? __builtin_fma(rhs[j], di[j], -u[j]) : rhs[j] - u[j];
                        u[j] = (j < R - 1) ? rhs[j] * di[j] : rhs[j];
                    } else {
                        d = (j < R - 1) ? rhs[j] * di[j] : rhs[j];
                        u[j] += d;
                    }
                    nd = __builtin_fma(d, d, nd);
                    nu = __builtin_fma(u[j], u[j], nu);
                }
            }
            if constexpr (ROT && UNI) {
                // the head in chunks of four elements, a round of the norm reduction in front of each: left to itself the
                // scheduler emits the whole head and then the reduction in one dependent piece
                WaveSum2 ws;
                tp.halo(u[0], u[R - 1], huL, huR);
                ws.start(nd, nu);
                auto weave = [&](auto kc) {
                    constexpr int K = decltype(kc)::value, J0 = 4 * K, J1 = J0 + 4 < R ? J0 + 4 : R;
                    if constexpr (K < 5) ws.template round<K>();
                    if constexpr (J0 < R) assemble_p1_rows<R, J0, J1>(c, u, huR, hf_at, hlo, hup, hse);
                };
                static_assert(R <= 24, "six chunks");
                weave(std::integral_constant<int, 0>{}); weave(std::integral_constant<int, 1>{});
                weave(std::integral_constant<int, 2>{}); weave(std::integral_constant<int, 3>{});
                weave(std::integral_constant<int, 4>{}); weave(std::integral_constant<int, 5>{});
                hlo[0] = __builtin_fma(-c.dt6, __builtin_fma(2.0, u[0], huL), c.aoff);
                ws.finish(nd, nu);
            } else {
                head();
                tp.sum2(nd, nu, nd, nu);
            }
            if constexpr (TRACE) {
                if (tp.first()) a.errs[((size_t)s * a.nsteps + step) * a.max_it + k] = sqrt(nd) / sqrt(nu);
            }
            ++k;
            // reference: error = ||dU|| / ||U1||; continue while error > tol and k < cap.
            // NaN compares false and ends the loop, as in the reference.
            more = (nd > a.tol2 * nu) && (k < a.max_it);
            far = LEANS && nd > lean2 * (a.tol2 * nu);                    // a NaN norm compares false: not far
            flags |= uniform_nonfinite(nd, nu) ? BG_FLAG_NONFINITE : 0;   // scalar: nd, nu are readlane results
        };
        if constexpr (LEANS) {
            while (far && more) iteration(std::true_type{});
            while (more) iteration(std::false_type{});
        } else {
            do iteration(std::false_type{}); while (more);      // the one loop, as it was
        }
        if (k >= a.max_it) flags |= BG_FLAG_HIT_CAP;
        store_rows<R>(hist + (size_t)(step + 1) * N, N, row0, FULL, u);
        if (tp.first()) a.iters[(size_t)s * a.nsteps + step] = k;
    }
    if (tp.first()) a.flags[s] = flags;
}

// ---- diagnostics: one assembly / one solve, the loop's own functions on given states ------------
struct AsmArgs {
    const double *x, *uk, *un, *mu1, *mu2;
    double *lo, *di, *up, *rhs;
    double dt, E;
    int N, B, supg;
};

template <int R, bool FULL, bool UNI, class Topo>
__device__ __forceinline__ void assemble_sample(const AsmArgs& a, Topo& tp, int s)
{
    const int N = a.N, row0 = tp.g * R;
    const double h = (a.x[N - 1] - a.x[0]) / (double)(N - 1);
    const MeshConst c = make_mesh_const(h, a.dt, a.E, a.supg);
    double hfs[R], fdt[R], u[R], un[R], g[R], lo[R], di[R], up[R], rhs[R];
    load_rows<R>(a.un + (size_t)s * N, N, row0, FULL, un);
    load_rows<R>(a.uk + (size_t)s * N, N, row0, FULL, u);
    if constexpr (UNI) {
        forcing_setup<R>(a.x, N, row0, a.mu2[s], c.h, a.dt, hfs, fdt);
        auto g_put = [&](int j, double v) { g[j] = v; };
        auto g_at = [&](int j) { return g[j]; };
        auto hf_at = [&](int j) { return hfs[j]; };
        mass_rhs<R, FULL>(tp, c, N, un, fdt, g_put);
        assemble<R, FULL, false>(tp, c, N, a.mu1[s], u, g_at, hf_at, lo, di, up, rhs);
    } else {
        ElemGeom<R> gm;
        geom_setup<R>(a.x, N, row0, a.dt, a.E, gm);
        forcing_setup_general<R>(a.x, N, row0, a.mu2[s], a.dt, hfs, fdt);
        mass_rhs_general<R>(tp, gm, N, un, fdt, g);
        assemble_general<R, false>(tp, gm, a.dt, c.kap, N, a.mu1[s], u, g, hfs, lo, di, up, rhs);
    }
    store_rows<R>(a.lo + (size_t)s * N, N, row0, FULL, lo);
    store_rows<R>(a.di + (size_t)s * N, N, row0, FULL, di);
    store_rows<R>(a.up + (size_t)s * N, N, row0, FULL, up);
    store_rows<R>(a.rhs + (size_t)s * N, N, row0, FULL, rhs);
}

struct SolveArgs {
    const double *lo, *di, *up, *rhs;
    double* sol;
    int N, B;
};

template <int R, class Topo>
__device__ __forceinline__ void solve_sample(const SolveArgs& a, Topo& tp, int s)
{
    const int N = a.N, row0 = tp.g * R;
    double lo[R], di[R], up[R], rhs[R];
    const size_t off = (size_t)s * N;
    load_rows<R>(a.lo + off, N, row0, false, lo);
    load_rows<R>(a.di + off, N, row0, false, di, 1.0);      // rows >= N are identity rows
    load_rows<R>(a.up + off, N, row0, false, up);
    load_rows<R>(a.rhs + off, N, row0, false, rhs);
    tp.template solve<R>(lo, di, up, rhs);
    store_rows<R>(a.sol + off, N, row0, false, rhs);
}

// ---- one wavefront per sample (N <= 1536), four samples per workgroup ----------------------------
template <int R, bool FULL, bool UNI = true, bool TRACE = false>
__global__ __launch_bounds__(64 * WAVES_PER_WG, 1) void fom_fused_kernel(FomArgs a)
{
    const int s = blockIdx.x * WAVES_PER_WG + (int)(threadIdx.x >> 6);
    if (s >= a.B) return;                                   // wave-uniform
    WaveTopoT<UNI> tp{lane_id()};                           // uniform mesh: the one-sided closing of pcr64
    fom_sample<R, FULL, UNI, TRACE, false>(a, tp, s, nullptr);
}

template <int R, bool FULL, bool UNI = true>
__global__ __launch_bounds__(64 * WAVES_PER_WG, 1) void fom_assemble_kernel(AsmArgs a)
{
    const int s = blockIdx.x * WAVES_PER_WG + (int)(threadIdx.x >> 6);
    if (s >= a.B) return;
    WaveTopo tp{lane_id()};
    assemble_sample<R, FULL, UNI>(a, tp, s);
}

template <int R>
__global__ __launch_bounds__(64 * WAVES_PER_WG, 1) void tridiag_solve_kernel(SolveArgs a)
{
    const int s = blockIdx.x * WAVES_PER_WG + (int)(threadIdx.x >> 6);
    if (s >= a.B) return;
    WaveTopoT<true> tp{lane_id()};
    solve_sample<R>(a, tp, s);
}

// ---- one workgroup per sample (N <= 8192), see fom_wide.hpp ---------------------------------------
template <int R, bool UNI>
__global__ __launch_bounds__(WIDE_THREADS, 1) void fom_wide_kernel(FomArgs a)
{
    constexpr bool PARK = UNI && R >= 32;
    __shared__ WideLds lds;
    __shared__ WidePark<PARK ? R : 1> park;
    wide_init(lds, threadIdx.x);
    WgTopo tp{lds, (int)threadIdx.x, 0};
    fom_sample<R, false, UNI, false, PARK>(a, tp, blockIdx.x, &park);
}

template <int R, bool UNI>
__global__ __launch_bounds__(WIDE_THREADS, 1) void fom_assemble_wide_kernel(AsmArgs a)
{
    __shared__ WideLds lds;
    wide_init(lds, threadIdx.x);
    WgTopo tp{lds, (int)threadIdx.x, 0};
    assemble_sample<R, false, UNI>(a, tp, blockIdx.x);
}

template <int R>
__global__ __launch_bounds__(WIDE_THREADS, 1) void tridiag_solve_wide_kernel(SolveArgs a)
{
    __shared__ WideLds lds;
    wide_init(lds, threadIdx.x);
    WgTopo tp{lds, (int)threadIdx.x, 0};
    solve_sample<R>(a, tp, blockIdx.x);
}

// ---- batched transpose out[b][c][r] = in[b][r][c] ----------------------------------
__global__ __launch_bounds__(256) void transpose_kernel(const double* __restrict__ in,
                                                        double* __restrict__ out, int nb, int rows, int cols)
{
    __shared__ double tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int b = blockIdx.z; b < nb; b += gridDim.z) {        // grid.z is capped at 65535
        const size_t base = (size_t)b * rows * cols;
#pragma unroll
        for (int k = 0; k < 32; k += 8) {
            int r = r0 + ty + k, cc = c0 + tx;
            if (r < rows && cc < cols) tile[ty + k][tx] = in[base + (size_t)r * cols + cc];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 32; k += 8) {
            int cc = c0 + ty + k, r = r0 + tx;
            if (r < rows && cc < cols) out[base + (size_t)cc * rows + r] = tile[tx][ty + k];
        }
        __syncthreads();
    }
}

// ---- dispatch ------------------------------------------------------------------------
// workgroup-per-sample kernels: 8, 12, 16, 24 or 32 rows per THREAD of a 256-thread workgroup
// Measured (tools/time_wide.py, B = 1024): at 32 rows per lane the wave-per-sample kernel spills (N = 2048:
// 1.1e8 steps/s, N = 1800: 3.4e7) and the workgroup kernel at 8 rows per thread wins (1.29e8 / 1.24e8); at 24
// rows per lane the wave kernel still wins (N = 1536: 2.7e8 against 1.4e8).
constexpr int kWaveMaxN = 64 * 24, kWideMaxN = WIDE_THREADS * 32;

// Instantiations at 2 or 4 rows per thread (round 3) put a sample of N <= 512, 1024 nodes on all four SIMDs of a CU instead
// of on one wavefront: built as the low-latency form for small batches (the strong-scaling share of a sweep, the
// reference's one-mu-per-call pattern, FEM/paper_training_stage.py:28-49), measured slower than the wavefront form
// (see bg_fom_run) and therefore opt-in (BG_OPT_FOM_WIDE).
template <typename F>
int dispatch_wide(int N, F&& f)                                  // (N <= 256: identity rows beyond N)
{
    return dispatch_rows<WIDE_THREADS, 2, 4, 8, 12, 16, 24, 32>(N, f);
}

// rows per lane of the wave-per-sample kernels
template <typename F>
int dispatch_r(int N, F&& f)
{
    return dispatch_rows<64, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 16, 24>(N, f);
}

// The checks of bg_fom_run and bg_fom_run_traced (`traced`: wave-per-sample sizes only, and errs is required) and the
// kernels' argument block.  BG_OK with B == 0 means there is nothing to launch.
int fom_args(FomArgs& a, bool traced, int N, int B, int nsteps, const double* x, const double* u0, const double* mu1,
             const double* mu2, double dt, double E, double tol, int max_it, int supg, double* hist, int32_t* iters,
             int32_t* flags, double* errs)
{
    if (N < 2 || B < 0 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (traced && N > kWaveMaxN) return BG_ERR_UNSUPPORTED_N;
    if (B == 0) return BG_OK;
    if (!x || !u0 || !mu1 || !mu2 || !hist || !flags || (traced && !errs) || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    a.x = x; a.u0 = u0; a.mu1 = mu1; a.mu2 = mu2; a.hist = hist; a.iters = iters; a.flags = flags; a.errs = errs;
    // the kernels test nd > tol2 nu for the reference's error > tol; a negative tol never stops a step, which its square would
    a.dt = dt; a.E = E; a.tol2 = tol < 0.0 ? -1.0 : tol * tol;
    a.N = N; a.B = B; a.nsteps = nsteps; a.max_it = max_it; a.supg = supg & BG_OPT_SUPG;
    return BG_OK;
}

}  // namespace

extern "C" {

int bg_abi_version(void) { return BG_ABI_VERSION; }

int bg_last_hip_error(void) { return bg::tls_last_hip_error; }

int bg_fom_max_n(void) { return kWideMaxN; }

const char* bg_strerror(int code)
{
    switch (code) {
        case BG_OK: return "ok";
        case BG_ERR_BAD_ARG: return "bad argument";
        case BG_ERR_UNSUPPORTED_N: return "N not supported by the fused kernels (2 <= N <= 8192)";
        case BG_ERR_NONUNIFORM: return "mesh is not uniform";
        case BG_ERR_LAUNCH: return "kernel launch failed (see bg_last_hip_error)";
        case BG_ERR_UNSUPPORTED_R: return "reduced dimension not supported";
        case BG_ERR_PROJECTION: return "unknown projection";
        case BG_ERR_WORKSPACE: return "workspace too small";
        default: return "unknown error";
    }
}

int bg_fom_run(int N, int B, int nsteps, const double* x, const double* u0, const double* mu1,
               const double* mu2, double dt, double E, double tol, int max_it, int supg, double* hist,
               int32_t* iters, int32_t* flags, void* stream)
{
    FomArgs a;
    const int err = fom_args(a, false, N, B, nsteps, x, u0, mu1, mu2, dt, E, tol, max_it, supg, hist, iters, flags, nullptr);
    if (err != BG_OK || B == 0) return err;
    const bool nonuniform = (supg & BG_OPT_NONUNIFORM) != 0;
    const dim3 grid((B + WAVES_PER_WG - 1) / WAVES_PER_WG), block(64 * WAVES_PER_WG);
    hipStream_t st = (hipStream_t)stream;
    // one workgroup per sample: beyond one wavefront's registers -- and, on request (BG_OPT_FOM_WIDE, uniform mesh, N > 64),
    // below that too.  It is NOT the default there: measured at N = 1024 (round 3, B = 128 = one sample per second CU)
    // 2.18 us per Picard iteration against 1.86 us for one wavefront per sample -- 4 rows per thread instead of 16 shorten
    // the per-thread work threefold, but the seven workgroup barriers and LDS exchanges of an iteration cost more than that.
    const bool both = N <= kWaveMaxN && N > 64 && !nonuniform;
    const bool wide = N > kWaveMaxN || (both && (supg & BG_OPT_FOM_WIDE) && !(supg & BG_OPT_FOM_WAVE));
    if (wide)
        return dispatch_wide(N, [&](auto rc) {
            constexpr int R = decltype(rc)::value;
            if constexpr (R >= 8) {
                if (nonuniform) {
                    hipLaunchKernelGGL((fom_wide_kernel<R, false>), dim3(B), dim3(WIDE_THREADS), 0, st, a);
                    return check_launch();
                }
            }
            hipLaunchKernelGGL((fom_wide_kernel<R, true>), dim3(B), dim3(WIDE_THREADS), 0, st, a);
            return check_launch();
        });
    return dispatch_r(N, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        if (nonuniform)
            hipLaunchKernelGGL((fom_fused_kernel<R, false, false>), grid, block, 0, st, a);
        else if (N == 64 * R)
            hipLaunchKernelGGL((fom_fused_kernel<R, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((fom_fused_kernel<R, false>), grid, block, 0, st, a);
        return check_launch();
    });
}

int bg_fom_run_traced(int N, int B, int nsteps, const double* x, const double* u0, const double* mu1, const double* mu2,
                      double dt, double E, double tol, int max_it, int supg, double* hist, int32_t* iters, int32_t* flags,
                      double* errs, void* stream)
{
    FomArgs a;
    const int err = fom_args(a, true, N, B, nsteps, x, u0, mu1, mu2, dt, E, tol, max_it, supg, hist, iters, flags, errs);
    if (err != BG_OK || B == 0) return err;
    const bool nonuniform = (supg & BG_OPT_NONUNIFORM) != 0;
    const dim3 grid((B + WAVES_PER_WG - 1) / WAVES_PER_WG), block(64 * WAVES_PER_WG);
    hipStream_t st = (hipStream_t)stream;
    return dispatch_r(N, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        if (nonuniform)
            hipLaunchKernelGGL((fom_fused_kernel<R, false, false, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((fom_fused_kernel<R, false, true, true>), grid, block, 0, st, a);
        return check_launch();
    });
}

int bg_fom_assemble(int N, int B, const double* x, const double* uk, const double* un, const double* mu1,
                    const double* mu2, double dt, double E, int supg, double* lo, double* di, double* up,
                    double* rhs, void* stream)
{
    if (N < 2 || B < 0 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (B == 0) return BG_OK;
    if (!x || !uk || !un || !mu1 || !mu2 || !lo || !di || !up || !rhs) return BG_ERR_BAD_ARG;
    AsmArgs a;
    a.x = x; a.uk = uk; a.un = un; a.mu1 = mu1; a.mu2 = mu2; a.lo = lo; a.di = di; a.up = up; a.rhs = rhs;
    a.dt = dt; a.E = E; a.N = N; a.B = B; a.supg = supg & BG_OPT_SUPG;
    const bool nonuniform = (supg & BG_OPT_NONUNIFORM) != 0;
    const dim3 grid((B + WAVES_PER_WG - 1) / WAVES_PER_WG), block(64 * WAVES_PER_WG);
    hipStream_t st = (hipStream_t)stream;
    if (N > kWaveMaxN)
        return dispatch_wide(N, [&](auto rc) {
            constexpr int R = decltype(rc)::value;
            if (nonuniform)
                hipLaunchKernelGGL((fom_assemble_wide_kernel<R, false>), dim3(B), dim3(WIDE_THREADS), 0, st, a);
            else
                hipLaunchKernelGGL((fom_assemble_wide_kernel<R, true>), dim3(B), dim3(WIDE_THREADS), 0, st, a);
            return check_launch();
        });
    return dispatch_r(N, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        if (nonuniform)
            hipLaunchKernelGGL((fom_assemble_kernel<R, false, false>), grid, block, 0, st, a);
        else if (N == 64 * R)
            hipLaunchKernelGGL((fom_assemble_kernel<R, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((fom_assemble_kernel<R, false>), grid, block, 0, st, a);
        return check_launch();
    });
}

int bg_tridiag_solve(int N, int B, const double* lo, const double* di, const double* up, const double* rhs,
                     double* sol, void* stream)
{
    if (N < 1 || B < 0) return BG_ERR_BAD_ARG;
    if (B == 0) return BG_OK;
    if (!lo || !di || !up || !rhs || !sol) return BG_ERR_BAD_ARG;
    SolveArgs a{lo, di, up, rhs, sol, N, B};
    const dim3 grid((B + WAVES_PER_WG - 1) / WAVES_PER_WG), block(64 * WAVES_PER_WG);
    hipStream_t st = (hipStream_t)stream;
    if (N > kWaveMaxN)
        return dispatch_wide(N, [&](auto rc) {
            constexpr int R = decltype(rc)::value;
            hipLaunchKernelGGL((tridiag_solve_wide_kernel<R>), dim3(B), dim3(WIDE_THREADS), 0, st, a);
            return check_launch();
        });
    return dispatch_r(N, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        hipLaunchKernelGGL((tridiag_solve_kernel<R>), grid, block, 0, st, a);
        return check_launch();
    });
}

int bg_transpose_batched(int B, int rows, int cols, const double* in, double* out, void* stream)
{
    if (B < 0 || rows < 0 || cols < 0) return BG_ERR_BAD_ARG;
    if (B == 0 || rows == 0 || cols == 0) return BG_OK;
    if (!in || !out) return BG_ERR_BAD_ARG;
    const dim3 grid((cols + 31) / 32, (rows + 31) / 32, B < 65535 ? B : 65535), block(256);
    hipLaunchKernelGGL(transpose_kernel, grid, block, 0, (hipStream_t)stream, in, out, B, rows, cols);
    return check_launch();
}

}  // extern "C"
