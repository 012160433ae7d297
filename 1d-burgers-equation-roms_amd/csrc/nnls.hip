// nnls.hip -- the device side of the active-set NNLS behind the hyper-reduction row samplings (burgers_hip/pod.py
// nnls_rows_device): the Lawson-Hanson iteration of pod.nnls_rows on a thin QR of the active columns that is kept on the
// device, appended to by two passes of classical Gram-Schmidt and rebuilt from the first dropped position when columns leave.
// The host drives the iteration and reads one 64-byte bg_nnls_status per least-squares solve; the matrices stay here.
//
// pick      bg_nnls_pick: nnls_dot_kernel, one wave per candidate column (16-byte loads, four pairs of them in flight per
//           lane, four accumulators folded in a fixed order, then the wave's shuffle tree), skips the masked columns;
//           nnls_pick_kernel, one workgroup: the largest entry (the lowest index on ties), |res|, and the decision of
//           nnls_rows' loop head (done / no column left / full / go on) that gates the append and the solve queued behind it.
// append    bg_nnls_append: h1 = Q^T v (nnls_dot_kernel over the rows of Q), v -= Q h1 (nnls_combine_kernel, one thread per
//           row, the columns in their order), the same once more, and nnls_finish_kernel (one workgroup): the two norms, the
//           dependence test, Q[k] = v / |v|, column k of R, z[k] = Q[k] . b.
// solve     bg_nnls_solve: one workgroup, thread i owns row i: back-substitution column by column (the multipliers of eight
//           columns are loaded ahead of the barriers), then nnls_rows' step rule and the compaction of order and x.
// residual  bg_nnls_residual: nnls_combine_kernel with the active columns of At themselves, in insertion order.
// No floating-point atomics; every sum runs in an order fixed by the shapes alone, so two calls give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"

namespace {

constexpr int NN_MAX_ACTIVE = 512;            // threads of the solve kernel: one per active column
constexpr int NN_MAX_COLS = 65536;
constexpr int NN_WG = 1024;                   // threads of the one-workgroup reductions
constexpr double NN_EPS = 2.220446049250313e-16;

typedef double double2v __attribute__((ext_vector_type(2)));

// Sum over the workgroup in a fixed tree; every thread gets it.  ``sh`` holds blockDim.x doubles.
__device__ inline double block_sum(double v, double* sh)
{
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    return sh[0];
}

// a . v over ``rows`` entries by one wave (a and v 16-byte aligned); the sum is in lane 0.  STREAM: a is read once and
// not again soon (the pass over G), so its loads are non-temporal; the rows of Q, read four times per append, stay cached.
template <bool STREAM>
__device__ inline double wave_dot(const double* __restrict__ a, const double* __restrict__ v, int rows, int lane)
{
    const int pairs = rows >> 1;
    const double2v* a2 = (const double2v*)a;
    const double2v* v2 = (const double2v*)v;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int p = lane;
    for (; p + 192 < pairs; p += 256) {
        double2v x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = STREAM ? __builtin_nontemporal_load(a2 + p + 64 * u) : a2[p + 64 * u];
#pragma unroll
        for (int u = 0; u < 4; ++u) y[u] = v2[p + 64 * u];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = __builtin_fma(x[u].y, y[u].y, __builtin_fma(x[u].x, y[u].x, acc[u]));
    }
    for (; p < pairs; p += 64) {
        const double2v x = a2[p], y = v2[p];
        acc[0] = __builtin_fma(x.y, y.y, __builtin_fma(x.x, y.x, acc[0]));
    }
    if (lane == 0 && (rows & 1)) acc[1] = __builtin_fma(a[rows - 1], v[rows - 1], acc[1]);
    double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    return s;
}

// What an append works on: the pick of the last bg_nnls_pick, or order[k] when a drop is being repaired.
__device__ inline int append_column(const bg_nnls_status* st, const int32_t* order, int k, int rebuild)
{
    return rebuild ? order[k] : st->pick;
}

__device__ inline bool append_gated(const bg_nnls_status* st, int rebuild)
{
    return rebuild ? st->stop == BG_NNLS_FAULT : st->stop != BG_NNLS_GO;
}

// out[i] = M[i] . v for the rows i < n of M that no mask names.  MODE 0: v is ``v`` (the gradient); 1: v is the append's
// column of At; 2: v is ``v``, gated like an append.
template <int MODE>
__global__ __launch_bounds__(256) void nnls_dot_kernel(int n, int rows, size_t ld, const double* __restrict__ M,
                                                       const double* __restrict__ v, const int32_t* __restrict__ m1,
                                                       const int32_t* __restrict__ m2, double* __restrict__ out,
                                                       const bg_nnls_status* __restrict__ st,
                                                       const int32_t* __restrict__ order, int k, int rebuild)
{
    const int i = 4 * (int)blockIdx.x + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    if (MODE != 0) {
        if (append_gated(st, rebuild)) return;
        if (MODE == 1) v += (size_t)append_column(st, order, k, rebuild) * ld;
    } else if (m1[i] != 0 || m2[i] != 0) {
        if (lane == 0) out[i] = 0.0;
        return;
    }
    const double s = wave_dot<MODE == 0>(M + (size_t)i * ld, v, rows, lane);
    if (lane == 0) out[i] = s;
}

// out[row] = base[row] - sum_{c < k} coef[c] M[idx ? idx[c] : c][row], the sum in the order of c.  MODE 0: the residual
// (base is ``base``); 1: base is the append's column of At; 2: base is ``base``, gated like an append.
template <int MODE>
__global__ __launch_bounds__(256) void nnls_combine_kernel(int rows, size_t ld, int k, const double* __restrict__ M,
                                                           const int32_t* __restrict__ idx, const double* __restrict__ coef,
                                                           const double* base, double* out, const bg_nnls_status* __restrict__ st,
                                                           const int32_t* __restrict__ order, int ka, int rebuild)
{
    const int row = 256 * (int)blockIdx.x + (int)threadIdx.x;
    if (MODE != 0) {
        if (append_gated(st, rebuild)) return;
        if (MODE == 1) base += (size_t)append_column(st, order, ka, rebuild) * ld;
    }
    if (row >= rows) return;
    double acc = 0.0;
#pragma unroll 8
    for (int c = 0; c < k; ++c) {
        const size_t r = idx ? (size_t)idx[c] : (size_t)c;
        acc = __builtin_fma(coef[c], M[r * ld + row], acc);
    }
    out[row] = base[row] - acc;
}

// The largest unmasked entry of w (lowest index on ties), |res|, and the head of nnls_rows' loop.  G is finite (the builders
// refuse anything else), so w is: a NaN entry would not be singled out as np.argmax singles it out.
__global__ __launch_bounds__(NN_WG) void nnls_pick_kernel(int n, int rows, const double* __restrict__ w,
                                                          const int32_t* __restrict__ active, const int32_t* __restrict__ tabu,
                                                          const double* __restrict__ res, double dnorm, double tau,
                                                          int min_cols, int max_cols, bg_nnls_status* st)
{
    __shared__ double sv[NN_WG];
    __shared__ int si[NN_WG];
    const int t = threadIdx.x;
    double best = -INFINITY;
    int arg = -1;
    for (int j = t; j < n; j += NN_WG)
        if (active[j] == 0 && tabu[j] == 0 && (arg < 0 || w[j] > best)) { best = w[j]; arg = j; }
    sv[t] = best;
    si[t] = arg;
    __syncthreads();
    for (int o = NN_WG >> 1; o > 0; o >>= 1) {
        if (t < o) {
            const double vb = sv[t + o];
            const int ib = si[t + o];
            if (ib >= 0 && (si[t] < 0 || vb > sv[t] || (vb == sv[t] && ib < si[t]))) { sv[t] = vb; si[t] = ib; }
        }
        __syncthreads();
    }
    best = sv[0];
    arg = si[0];
    double q = 0.0;
    for (int i = t; i < rows; i += NN_WG) q = __builtin_fma(res[i], res[i], q);
    const double nrm = sqrt(block_sum(q, sv));
    if (t != 0) return;
    const double rel = dnorm > 0.0 ? nrm / dnorm : 0.0;
    const int fit_done = rel <= tau ? 1 : 0;
    const int count = st->count;
    int stop = BG_NNLS_GO;
    if (st->stop == BG_NNLS_FAULT) stop = BG_NNLS_FAULT;
    else if (fit_done && count >= min_cols) stop = BG_NNLS_DONE;
    else if (arg < 0 || !isfinite(best) || (!fit_done && best <= 0.0)) stop = BG_NNLS_NO_COLUMN;
    else if (count + 1 > max_cols) stop = BG_NNLS_FULL;
    st->stop = stop;
    st->pick = arg;
    st->fit_done = fit_done;
    st->dependent = 0;
    st->accepted = 0;
    st->p0 = count;
    st->pick_active = 0;
    st->w = arg >= 0 ? best : -INFINITY;
    st->resnorm = nrm;
    st->rel = rel;
}

// The end of an append: work holds v after the two Gram-Schmidt passes, h1 and h2 their coefficients.
__global__ __launch_bounds__(NN_WG) void nnls_finish_kernel(int rows, size_t ld, int k, const double* __restrict__ At,
                                                            const double* __restrict__ b, double* __restrict__ Q,
                                                            double* __restrict__ Rc, size_t ldr, double* __restrict__ z,
                                                            double* __restrict__ x, int32_t* __restrict__ order,
                                                            int32_t* __restrict__ active, int32_t* __restrict__ tabu,
                                                            const double* __restrict__ work, const double* __restrict__ h1,
                                                            const double* __restrict__ h2, bg_nnls_status* st, int rebuild)
{
    __shared__ double sh[NN_WG];
    if (append_gated(st, rebuild)) return;
    const int t = threadIdx.x;
    const int col = append_column(st, order, k, rebuild);
    const double* a = At + (size_t)col * ld;
    double qv = 0.0, qa = 0.0;
    for (int i = t; i < rows; i += NN_WG) {
        qv = __builtin_fma(work[i], work[i], qv);
        qa = __builtin_fma(a[i], a[i], qa);
    }
    const double nv = sqrt(block_sum(qv, sh)), na = sqrt(block_sum(qa, sh));
    const double ratio = na > 0.0 ? nv / na : 0.0;
    const bool dependent = !(nv > BG_NNLS_DEPENDENT_MULTIPLE * NN_EPS * na);
    if (dependent) {
        if (t == 0) {
            st->ratio = ratio;
            if (rebuild) {
                st->stop = BG_NNLS_FAULT;                  // a subset of independent columns cannot be dependent
            } else {
                st->dependent = 1;
                tabu[col] = 1;
            }
        }
        return;
    }
    double* q = Q + (size_t)k * ld;
    double qz = 0.0;
    for (int i = t; i < rows; i += NN_WG) {
        const double e = work[i] / nv;
        q[i] = e;
        qz = __builtin_fma(e, b[i], qz);
    }
    const double zk = block_sum(qz, sh);
    double* rk = Rc + (size_t)k * ldr;
    for (int i = t; i < k; i += NN_WG) rk[i] = h1[i] + h2[i];
    if (t == 0) {
        rk[k] = nv;
        z[k] = zk;
        active[col] = 1;
        if (!rebuild) {
            order[k] = col;
            x[k] = 0.0;
            st->dependent = 0;
        }
        st->count = k + 1;
        st->ratio = ratio;
    }
}

// R s = z, then nnls_rows' acceptance or step.  Rc[c][i] = R[i][c]: column c of R is contiguous.
__global__ __launch_bounds__(NN_MAX_ACTIVE) void nnls_solve_kernel(int k, const double* __restrict__ Rc, size_t ldr,
                                                                   const double* __restrict__ z, double* __restrict__ x,
                                                                   int32_t* __restrict__ order, int32_t* __restrict__ active,
                                                                   bg_nnls_status* st)
{
    __shared__ double sh[2];
    __shared__ double smin[NN_MAX_ACTIVE];
    __shared__ int sdrop[NN_MAX_ACTIVE], spos[NN_MAX_ACTIVE];
    __shared__ int s_p0, s_cnt;
    const int i = threadIdx.x;
    if (st->stop != BG_NNLS_GO || st->dependent != 0) return;
    if (st->count != k) {
        if (i == 0) st->stop = BG_NNLS_FAULT;
        return;
    }
    double zz = i < k ? z[i] : 0.0, s = 1.0;
    for (int c0 = k - 1; c0 >= 0; c0 -= 8) {
        double r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = c0 - u;
            r[u] = c >= 0 && i <= c ? Rc[(size_t)c * ldr + i] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = c0 - u;                     // the same for every thread
            if (c >= 0) {
                if (i == c) {
                    s = zz / r[u];
                    sh[c & 1] = s;
                }
                __syncthreads();
                if (i < c) zz = __builtin_fma(-r[u], sh[c & 1], zz);
            }
        }
    }
    const bool in = i < k;
    const int pick = st->pick;
    const int oi = in ? order[i] : -1;
    const double xi = in ? x[i] : 0.0;
    const bool neg = in && s <= 0.0;
    if (__syncthreads_count(neg) == 0) {
        if (in) x[i] = s;
        const int pa = __syncthreads_or(in && oi == pick);
        if (i == 0) {
            st->accepted = 1;
            st->p0 = k;
            st->pick_active = pa ? 1 : 0;
        }
        return;
    }
    // step towards s as far as x stays non-negative, drop what reaches 0 (no fused multiply-add: the host's roundings)
    // an entry at 0 (the column just appended) leaves at once; the host's quotient is 0 there too, or 0 / 0 for s = 0 exactly
    const double ratio = neg ? (xi > 0.0 ? xi / (xi - s) : 0.0) : INFINITY;
    smin[i] = ratio;
    __syncthreads();
    for (int o = NN_MAX_ACTIVE >> 1; o > 0; o >>= 1) {
        if (i < o) smin[i] = fmin(smin[i], smin[i + o]);
        __syncthreads();
    }
    const double alpha = smin[0];
    double xa = __dadd_rn(xi, __dmul_rn(alpha, __dsub_rn(s, xi)));
    if (ratio <= alpha) xa = 0.0;
    const double xn = fmax(xa, 0.0);
    const bool drop = in && xn <= 0.0;
    sdrop[i] = drop ? 1 : 0;
    __syncthreads();
    if (i == 0) {
        int cnt = 0, p0 = k;
        for (int c = 0; c < k; ++c) {
            spos[c] = cnt;
            if (sdrop[c]) {
                if (p0 == k) p0 = c;
            } else {
                ++cnt;
            }
        }
        s_p0 = p0;
        s_cnt = cnt;
    }
    __syncthreads();                                  // every order[i] and x[i] was read before this barrier
    if (in) {
        if (drop) {
            active[oi] = 0;
        } else {
            order[spos[i]] = oi;
            x[spos[i]] = xn;
        }
    }
    const int pa = __syncthreads_or(in && !drop && oi == pick);
    if (i == 0) {
        st->accepted = 0;
        st->p0 = s_p0;
        st->count = s_cnt;
        st->pick_active = pa ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void nnls_mark_kernel(int n, int32_t* __restrict__ tabu, int j, int value)
{
    const int i = 256 * (int)blockIdx.x + (int)threadIdx.x;
    if (j >= 0) {
        if (i == 0) tabu[j] = value;
    } else if (i < n) {
        tabu[i] = value;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int bg_nnls_limits(int* max_active, int* max_cols)
{
    if (!max_active || !max_cols) return BG_ERR_BAD_ARG;
    *max_active = NN_MAX_ACTIVE;
    *max_cols = NN_MAX_COLS;
    return BG_OK;
}

extern "C" long long bg_nnls_work_elems(int ld) { return ld < 0 ? 0 : (long long)ld + 2 * NN_MAX_ACTIVE; }

extern "C" int bg_nnls_residual(int rows, int ld, int k, const double* At, const double* b, const double* x,
                                const int32_t* order, double* res, void* stream)
{
    if (rows < 0 || k < 0 || ld < rows) return BG_ERR_BAD_ARG;
    if (rows == 0) return BG_OK;
    if (k > NN_MAX_ACTIVE) return BG_ERR_UNSUPPORTED_R;
    if (!b || !res || (k > 0 && (!At || !x || !order))) return BG_ERR_BAD_ARG;
    hipLaunchKernelGGL(nnls_combine_kernel<0>, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, rows, (size_t)ld, k,
                       At, order, x, b, res, (const bg_nnls_status*)nullptr, (const int32_t*)nullptr, 0, 0);
    return bg::check_launch();
}

extern "C" int bg_nnls_pick(int rows, int n, int ld, const double* At, const double* res, const int32_t* active,
                            const int32_t* tabu, double dnorm, double tau, int min_cols, int max_cols, double* w,
                            bg_nnls_status* status, void* stream)
{
    if (rows < 0 || n < 0 || ld < rows || min_cols < 0 || max_cols < 0 || !(dnorm >= 0.0) || !(tau >= 0.0)) return BG_ERR_BAD_ARG;
    if (n == 0) return BG_OK;
    if (n > NN_MAX_COLS || max_cols > NN_MAX_ACTIVE) return BG_ERR_UNSUPPORTED_R;
    if (!At || !res || !active || !tabu || !w || !status) return BG_ERR_BAD_ARG;
    if ((ld & 1) || !aligned16(At) || !aligned16(res)) return BG_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nnls_dot_kernel<0>, dim3((n + 3) / 4), dim3(256), 0, st, n, rows, (size_t)ld, At, res, active, tabu, w,
                       (const bg_nnls_status*)nullptr, (const int32_t*)nullptr, 0, 0);
    hipLaunchKernelGGL(nnls_pick_kernel, dim3(1), dim3(NN_WG), 0, st, n, rows, w, active, tabu, res, dnorm, tau, min_cols,
                       max_cols, status);
    return bg::check_launch();
}

extern "C" int bg_nnls_append(int rows, int ld, int k, int rebuild, const double* At, const double* b, double* Q, double* R,
                              int ldr, double* z, double* x, int32_t* order, int32_t* active, int32_t* tabu, double* work,
                              bg_nnls_status* status, void* stream)
{
    if (rows < 0 || k < 0 || ld < rows || ldr < 0) return BG_ERR_BAD_ARG;
    if (rows == 0) return BG_OK;
    if (k >= NN_MAX_ACTIVE) return BG_ERR_UNSUPPORTED_R;
    if (ldr <= k) return BG_ERR_BAD_ARG;
    if (!At || !b || !Q || !R || !z || !x || !order || !active || !tabu || !work || !status) return BG_ERR_BAD_ARG;
    if ((ld & 1) || !aligned16(At) || !aligned16(Q) || !aligned16(work)) return BG_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    double* h1 = work + ld;
    double* h2 = h1 + NN_MAX_ACTIVE;
    const dim3 wg(256), per_row((rows + 255) / 256), per_col((k + 3) / 4);
    const int rb = rebuild ? 1 : 0;
    if (k > 0)
        hipLaunchKernelGGL(nnls_dot_kernel<1>, per_col, wg, 0, st, k, rows, (size_t)ld, Q, At, (const int32_t*)nullptr,
                           (const int32_t*)nullptr, h1, status, order, k, rb);
    hipLaunchKernelGGL(nnls_combine_kernel<1>, per_row, wg, 0, st, rows, (size_t)ld, k, Q, (const int32_t*)nullptr, h1, At, work,
                       status, order, k, rb);
    if (k > 0) {
        hipLaunchKernelGGL(nnls_dot_kernel<2>, per_col, wg, 0, st, k, rows, (size_t)ld, Q, work, (const int32_t*)nullptr,
                           (const int32_t*)nullptr, h2, status, order, k, rb);
        hipLaunchKernelGGL(nnls_combine_kernel<2>, per_row, wg, 0, st, rows, (size_t)ld, k, Q, (const int32_t*)nullptr, h2, work,
                           work, status, order, k, rb);
    }
    hipLaunchKernelGGL(nnls_finish_kernel, dim3(1), dim3(NN_WG), 0, st, rows, (size_t)ld, k, At, b, Q, R, (size_t)ldr, z, x, order,
                       active, tabu, work, h1, h2, status, rb);
    return bg::check_launch();
}

extern "C" int bg_nnls_solve(int k, const double* R, int ldr, const double* z, double* x, int32_t* order, int32_t* active,
                             bg_nnls_status* status, void* stream)
{
    if (k < 0 || ldr < k) return BG_ERR_BAD_ARG;
    if (k == 0) return BG_OK;
    if (k > NN_MAX_ACTIVE) return BG_ERR_UNSUPPORTED_R;
    if (!R || !z || !x || !order || !active || !status) return BG_ERR_BAD_ARG;
    hipLaunchKernelGGL(nnls_solve_kernel, dim3(1), dim3(NN_MAX_ACTIVE), 0, (hipStream_t)stream, k, R, (size_t)ldr, z, x, order,
                       active, status);
    return bg::check_launch();
}

extern "C" int bg_nnls_mark(int n, int32_t* tabu, int j, int value, void* stream)
{
    if (n < 0 || j >= n) return BG_ERR_BAD_ARG;
    if (n == 0) return BG_OK;
    if (n > NN_MAX_COLS) return BG_ERR_UNSUPPORTED_R;
    if (!tabu) return BG_ERR_BAD_ARG;
    hipLaunchKernelGGL(nnls_mark_kernel, dim3(j >= 0 ? 1 : (n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, tabu, j,
                       value ? 1 : 0);
    return bg::check_launch();
}
