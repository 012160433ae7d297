// kmeans.hip -- the two kernels of the Lloyd iteration behind the local POD builder (burgers_hip/pod.py kmeans,
// build_local_bases): bg_kmeans_assign labels every snapshot with its nearest centre, bg_kmeans_update moves every centre to
// the mean of its snapshots.  The points are the snapshots in global POD coordinates, q [Ns][m] row-major, m <= 64; the
// centres [C][m], C <= 64: the limits of the device loops that consume the result (bg_local_rom_limits).
//
// assign: one WAVE per point, four waves per workgroup, grid-stride over the points.  The wave puts its point into LDS and
// calls local_nearest_centre (rom_stream_device.hpp), the function of the time loops -- lane c sums |q - centre_c|^2 in j
// order by FMA, the wave takes the first index of the minimum -- so a training snapshot gets the label the online loop
// picks for the same q_g, bit for bit, ties and all.  The lane distances are still at hand afterwards: one ballot gives the overlap
// membership word (bit c: c is the label, or d_c < overlap d_min) without an Ns x C distance matrix.  Changed labels are
// counted per wave and added with one integer atomic.
//
// update: one 1024-thread workgroup per cluster, no workspace and no floating-point atomics.  The workgroup walks the labels
// 1024 at a time and compacts the indices of its own points, in order, into LDS.  The sum is defined on the RANK of a point
// within its cluster alone: ranks are cut into chunks of 1024, wave w of a chunk adds its 64 ranks one after the other (lane
// j holds coordinate j), the waves' partial sums are added in wave order, the chunks in chunk order.  Nothing depends on
// the grid, on timing or on where the other clusters' points sit in the input, so the centres are bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/burgers_hip.h"
#include "abi_common.hpp"
#include "rom_stream_device.hpp"

namespace {

using namespace bg;

constexpr int KM_MAX_M = 64, KM_MAX_C = 64;
constexpr int KM_ASSIGN_WAVES = 4;             // waves (= points in flight) per workgroup of the assign kernel
constexpr int KM_ASSIGN_GRID = 2048;           // its largest grid: beyond 8192 points a wave takes more than one
constexpr int KM_CHUNK = 1024;                 // threads of an update workgroup = labels per tile = ranks per chunk

__global__ __launch_bounds__(64 * KM_ASSIGN_WAVES) void kmeans_assign_kernel(
    int Ns, int m, int C, const double* __restrict__ q, const double* __restrict__ centres, double overlap,
    int32_t* __restrict__ labels, double* __restrict__ d2min, uint64_t* __restrict__ member, int32_t* __restrict__ changed)
{
    __shared__ double s_q[KM_ASSIGN_WAVES][KM_MAX_M];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int n_changed = 0;
    for (long long i = (long long)blockIdx.x * KM_ASSIGN_WAVES + w; i < Ns; i += (long long)gridDim.x * KM_ASSIGN_WAVES) {
        if (lane < m) s_q[w][lane] = q[(size_t)i * m + lane];
        __builtin_amdgcn_wave_barrier();       // the wave's own row: written and read by this wave only
        double dc, d;                          // this lane's distance, the smallest of the wave
        const int label = local_nearest_centre<true>(s_q[w], centres, C, m, lane, &dc, &d);
        if (member) {
            const uint64_t bits = __ballot(lane < C && (lane == label || dc < overlap * d));
            if (lane == 0) member[i] = bits;
        }
        if (lane == 0) {
            n_changed += labels[i] != label;
            labels[i] = label;
            d2min[i] = d;
        }
        __builtin_amdgcn_wave_barrier();       // every lane has read s_q before the next point overwrites it
    }
    if (lane == 0 && n_changed) atomicAdd(changed, n_changed);
}

__global__ __launch_bounds__(KM_CHUNK) void kmeans_update_kernel(int Ns, int m, const double* __restrict__ q,
                                                                 const int32_t* __restrict__ labels,
                                                                 double* __restrict__ centres, int32_t* __restrict__ counts)
{
    constexpr int WAVES = KM_CHUNK / 64;
    __shared__ int s_idx[2 * KM_CHUNK];        // indices of this cluster's points, in order, not yet summed
    __shared__ int s_wcount[WAVES];
    __shared__ double s_part[WAVES][KM_MAX_M];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double total = 0.0;                        // wave 0, lane j: coordinate j of the cluster's sum
    int fill = 0, count = 0;                   // workgroup-uniform

    // the sum of the ranks [0, n) held in s_idx, n <= KM_CHUNK, added to total; a workgroup barrier on either side
    auto add_chunk = [&](int n) {
        const int k0 = w * 64, k1 = min(k0 + 64, n);
        double p = 0.0;
        if (lane < m) {
#pragma unroll 8
            for (int k = k0; k < k1; ++k) p += q[(size_t)s_idx[k] * m + lane];
            s_part[w][lane] = p;
        }
        __syncthreads();
        if (w == 0 && lane < m) {
            const int nw = (n + 63) / 64;
            double t = s_part[0][lane];
            for (int v = 1; v < nw; ++v) t += s_part[v][lane];
            total += t;
        }
        __syncthreads();
    };

    for (int base = 0; base < Ns; base += KM_CHUNK) {
        const int i = base + tid;              // base < Ns <= INT_MAX and base + tid < base + 1024: checked by the entry point
        const bool mine = i < Ns && labels[i] == c;
        const uint64_t vote = __ballot(mine);
        if (lane == 0) s_wcount[w] = __popcll(vote);
        __syncthreads();
        int before = 0, tile = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) {
            const int n = s_wcount[v];
            before += v < w ? n : 0;
            tile += n;
        }
        if (mine) s_idx[fill + before + __popcll(vote & ((1ull << lane) - 1ull))] = i;
        __syncthreads();
        fill += tile;
        count += tile;
        if (fill >= KM_CHUNK) {                // fill < KM_CHUNK before the tile, so fill < 2 KM_CHUNK here
            add_chunk(KM_CHUNK);
            fill -= KM_CHUNK;
            const int keep = tid < fill ? s_idx[KM_CHUNK + tid] : 0;
            __syncthreads();
            if (tid < fill) s_idx[tid] = keep;
            __syncthreads();
        }
    }
    if (fill > 0) add_chunk(fill);
    if (w == 0) {
        if (lane < m && count > 0) centres[(size_t)c * m + lane] = total / (double)count;   // an empty cluster keeps its centre
        if (lane == 0) counts[c] = count;
    }
}

}  // namespace

extern "C" int bg_kmeans_limits(int* max_m, int* max_clusters)
{
    if (max_m) *max_m = KM_MAX_M;
    if (max_clusters) *max_clusters = KM_MAX_C;
    return BG_OK;
}

extern "C" int bg_kmeans_assign(int Ns, int m, int C, const double* q, const double* centres, double overlap, int32_t* labels,
                                double* d2min, uint64_t* member, int32_t* changed, void* stream)
{
    if (Ns < 0 || m < 1 || C < 1 || !(overlap >= 0.0)) return BG_ERR_BAD_ARG;
    if (m > KM_MAX_M || C > KM_MAX_C) return BG_ERR_UNSUPPORTED_R;
    if (Ns == 0) return BG_OK;
    if (!q || !centres || !labels || !d2min || !changed) return BG_ERR_BAD_ARG;
    const int grid = (int)min((long long)KM_ASSIGN_GRID, ((long long)Ns + KM_ASSIGN_WAVES - 1) / KM_ASSIGN_WAVES);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(grid), dim3(64 * KM_ASSIGN_WAVES), 0, (hipStream_t)stream, Ns, m, C, q,
                       centres, overlap, labels, d2min, member, changed);
    return bg::check_launch();
}

extern "C" int bg_kmeans_update(int Ns, int m, int C, const double* q, const int32_t* labels, double* centres, int32_t* counts,
                                void* stream)
{
    if (Ns < 0 || m < 1 || C < 1) return BG_ERR_BAD_ARG;
    if (m > KM_MAX_M || C > KM_MAX_C) return BG_ERR_UNSUPPORTED_R;
    if (Ns == 0) return BG_OK;
    if (Ns > INT32_MAX - KM_CHUNK) return BG_ERR_BAD_ARG;       // the tile loop's index stays an int
    if (!q || !labels || !centres || !counts) return BG_ERR_BAD_ARG;
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(C), dim3(KM_CHUNK), 0, (hipStream_t)stream, Ns, m, q, labels, centres, counts);
    return bg::check_launch();
}
