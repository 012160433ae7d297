// fd.hip -- fused batched finite-difference true-Newton stepper (widening row f.4 of SURVEY 8).
//
// Replaces FDBurgers.fom_burgers_newton with the analytical Jacobian (reference
// FD/fd_burgers.py:59-107; residual :28-35, Jacobian :37-44, boundary values :19-22).
// Same skeleton as the FEM kernels: one body (fd_sample) over the topologies of fom_wide.hpp, one
// wavefront (N <= 2048) or one workgroup (N <= 8192) per (mu1, mu2) sample for the whole time loop,
// rows in registers, the tridiagonal Newton system solved by the Wang + PCR solver of
// fom_device.hpp.  The Jacobian is diagonally dominant here (1/dt + 2 nu/dx^2 on the diagonal),
// so pivot-free elimination is safe.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "fom_device.hpp"
#include "fom_wide.hpp"

namespace {

using namespace bg;

struct FdArgs {
    const double* x;
    const double* u0;
    const double* mu1;
    const double* mu2;
    double* hist;
    int32_t* iters;
    int32_t* flags;
    double dt, tol;
    int N, B, nsteps, max_it;
};

// boundary values of the reference's apply_dirichlet_bc: U[0] = mu1, U[-1] = U[-2]
template <int R, class Topo>
__device__ __forceinline__ void apply_bc(Topo& tp, double (&u)[R], int N, int row0, double mu1)
{
    const double uL = tp.below(u[R - 1]);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int i = row0 + j;
        const double um = (j == 0) ? uL : u[j - 1];
        u[j] = (i == 0) ? mu1 : ((i == N - 1) ? um : u[j]);
    }
}

// the whole time loop of sample s; every branch below is uniform over the sample's threads
template <int R, class Topo>
__device__ __forceinline__ void fd_sample(const FdArgs& a, Topo& tp, int s)
{
    const int N = a.N, row0 = tp.g * R;
    const double dx = (a.x[N - 1] - a.x[0]) / (double)(N - 1);
    const double idt = 1.0 / a.dt, i2dx = 1.0 / (2.0 * dx), idx2 = 1.0 / (dx * dx);
    const double mu1 = a.mu1[s], mu2 = a.mu2[s];
    double u[R], src[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int i = row0 + j;
        u[j] = (i < N) ? a.u0[(size_t)s * N + i] : 0.0;
        src[j] = (i < N) ? 0.02 * exp(mu2 * a.x[i]) : 0.0;
    }
    apply_bc<R>(tp, u, N, row0, mu1);
    double* hist = a.hist + (size_t)s * (size_t)(a.nsteps + 1) * (size_t)N;
#pragma unroll
    for (int j = 0; j < R; ++j)
        if (row0 + j < N) hist[row0 + j] = u[j];

    // The three maxima of an iteration are np.max's in the reference: NaN when an entry is, and both stopping tests then
    // fail.  fmax drops a NaN operand, so the NaN is carried beside the maxima, without a test per row and solve:
    //   unan   "an interior row of u is NaN", uniform over the sample.  From u0 here; afterwards u changes only by the
    //          solution of a solve, and a NaN never leaves u.
    //   a solve (wang_reduce, the PCR, wang_finish of fom_device.hpp) multiplies whatever NaN enters a thread's rows or
    //          coefficients into that thread's interface unknown, its last row, and from there into all its rows; only
    //          interior rows have coefficients that can be NaN.  So "the update has a NaN" is one test per thread.
    //   a NaN residual on a finite state (src, or inf - inf) fails the residual test where that test would pass.
    bool u0nan = false;
#pragma unroll
    for (int j = 0; j < R; ++j) u0nan |= (row0 + j >= 1) && (row0 + j <= N - 2) && (u[j] != u[j]);
    bool unan = tp.gmax(u0nan ? 1.0 : 0.0) > 0.0;
    const double nan = __builtin_nan("");

    int flags = 0;
    for (int step = 0; step < a.nsteps; ++step) {
        double uprev[R];
#pragma unroll
        for (int j = 0; j < R; ++j) uprev[j] = u[j];
        int k = 0;
        bool converged = false;
        for (int it = 0; it < a.max_it; ++it) {
            apply_bc<R>(tp, u, N, row0, mu1);
            const double uL = tp.below(u[R - 1]);
            const double uR = tp.above(u[0]);
            double mloc = 0.0;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const int i = row0 + j;
                mloc = (i >= 1 && i <= N - 2) ? fmax(mloc, fabs(u[j])) : mloc;
            }
            const double mglob = tp.gmax(mloc);
            const double umax_int = unan ? nan : mglob;             // max |U_guess[1:-1]|
            const double uall = (unan || mu1 != mu1) ? nan : fmax(umax_int, fabs(mu1));
            const double nu = 0.25 * dx * uall;                     // max over ALL entries (U[-1] = U[-2])
            const double nud = nu * idx2;
            double lo[R], di[R], up[R], rhs[R];
            double rloc = 0.0;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const int i = row0 + j;
                const double um = (j == 0) ? uL : u[j - 1];
                const double ur = (j == R - 1) ? uR : u[j + 1];
                const bool interior = (i >= 1) && (i <= N - 2);
                const double conv = (0.5 * ur * ur - 0.5 * um * um) * i2dx;
                const double diff = nu * ((ur - 2.0 * u[j]) + um) * idx2;
                const double Ri = (u[j] - uprev[j]) * idt + conv - src[j] - diff;
                rloc = interior ? fmax(rloc, fabs(Ri)) : rloc;
                lo[j] = (interior && i > 1) ? (-um * i2dx - nud) : 0.0;
                up[j] = (interior && i < N - 2) ? (ur * i2dx - nud) : 0.0;
                di[j] = interior ? (idt + 2.0 * nud) : 1.0;
                rhs[j] = interior ? -Ri : 0.0;
            }
            const double rglob = tp.gmax(rloc);
            const double res = unan ? nan : rglob;                  // a NaN state has a NaN nu, hence a NaN residual
            if (res < a.tol) {
                // about to leave: once per step at the most, look for a NaN the maximum has dropped (rhs = -Ri or 0)
                bool rnan = false;
#pragma unroll
                for (int j = 0; j < R; ++j) rnan |= (rhs[j] != rhs[j]);
                if (!(tp.gmax(rnan ? 1.0 : 0.0) > 0.0)) { converged = true; break; }
            }
            tp.template solve<R>(lo, di, up, rhs);
            double dloc = 0.0;
#pragma unroll
            for (int j = 0; j < R; ++j) {
                dloc = fmax(dloc, fabs(rhs[j]));
                u[j] += rhs[j];
            }
            const double dmax = tp.gmax_nan(dloc, rhs[R - 1] != rhs[R - 1]);
            unan |= (dmax != dmax);
            // a NaN umax_int stays NaN: Python's max(nan, 1e-15) is nan
            const double rel = dmax / (unan ? nan : fmax(umax_int, 1e-15));
            ++k;
            if (uniform_nonfinite(rel)) flags |= BG_FLAG_NONFINITE;
            if (rel < a.tol) { converged = true; break; }
        }
        if (!converged) flags |= BG_FLAG_HIT_CAP;
        apply_bc<R>(tp, u, N, row0, mu1);
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (row0 + j < N) hist[(size_t)(step + 1) * N + row0 + j] = u[j];
        if (tp.g == 0) a.iters[(size_t)s * a.nsteps + step] = k;
    }
    if (tp.g == 0) a.flags[s] = flags;
}

template <int R>
__global__ __launch_bounds__(256, 1) void fd_fused_kernel(FdArgs a)
{
    const int s = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (s >= a.B) return;                                           // wave-uniform
    WaveTopo tp{lane_id()};
    fd_sample<R>(a, tp, s);
}

template <int R>
__global__ __launch_bounds__(WIDE_THREADS, 1) void fd_wide_kernel(FdArgs a)
{
    __shared__ WideLds lds;
    wide_init(lds, threadIdx.x);
    WgTopo tp{lds, (int)threadIdx.x, 0};
    fd_sample<R>(a, tp, blockIdx.x);
}

}  // namespace

extern "C" int bg_fd_run(int N, int B, int nsteps, const double* x, const double* u0, const double* mu1,
                         const double* mu2, double dt, double tol, int max_it, double* hist, int32_t* iters,
                         int32_t* flags, void* stream)
{
    if (N < 3 || B < 0 || nsteps < 0 || max_it < 1 || !(dt > 0.0)) return BG_ERR_BAD_ARG;
    if (B == 0) return BG_OK;
    if (!x || !u0 || !mu1 || !mu2 || !hist || !flags || (nsteps > 0 && !iters)) return BG_ERR_BAD_ARG;
    FdArgs a{x, u0, mu1, mu2, hist, iters, flags, dt, tol, N, B, nsteps, max_it};
    const dim3 grid((B + 3) / 4), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (N > 2048)                                    // one workgroup per sample; BG_ERR_UNSUPPORTED_N beyond 8192
        return bg::dispatch_rows<WIDE_THREADS, 12, 16, 24, 32>(N, [&](auto rc) {
            hipLaunchKernelGGL((fd_wide_kernel<decltype(rc)::value>), dim3(B), dim3(WIDE_THREADS), 0, st, a);
            return bg::check_launch();
        });
    return bg::dispatch_rows<64, 1, 2, 4, 8, 12, 16, 24, 32>(N, [&](auto rc) {
        hipLaunchKernelGGL((fd_fused_kernel<decltype(rc)::value>), grid, block, 0, st, a);
        return bg::check_launch();
    });
}
