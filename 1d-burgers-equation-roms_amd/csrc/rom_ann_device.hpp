// rom_ann_device.hpp -- the closure MLP of the POD-ANN time loops: its limits, its part of the kernel arguments, the host-side
// check that fills it, and the float32 forward-mode layer loop.
// Used by rom_ann_fused.hip (bg_ann_rom_run, 8 outputs per thread) and rom_ann_wide_loop_device.hpp (bg_ann_rom_run_wide and
// bg_hyper_ann_rom_run_wide, 4 outputs per thread).  The kernels keep the input set-up, the tables they build from the outputs, the LDS overlays, the opaque
// re-derivation of the thread indices, the issue priorities and the loops.
#pragma once
#include <stdint.h>

#include "rom_fused_device.hpp"

namespace bg {
namespace fused {

constexpr int ANN_MAX_LAYERS = 8;
constexpr int ANN_MAX_WIDTH = 256;      // one thread per neuron
constexpr int ANN_MAX_NBAR = 128;

struct AnnModel {
    const float* wt[ANN_MAX_LAYERS];     // layer l: W^T, [in4][ld] row-major: width[l] rounded up to 4 rows, width[l+1] to 8 columns, zero fill
    const float* bias[ANN_MAX_LAYERS];   // [width[l+1]] or null
    int width[ANN_MAX_LAYERS + 1];
    int act[ANN_MAX_LAYERS];
    float alpha[ANN_MAX_LAYERS];
    int nl;
};

// Kernel arguments of both loops.  UT: rows 0 .. n-1 = U_p^T, rows n .. n+nbar-1 = U_s^T;
//   bg_ann_rom_run:       [m8][N], zero rows up to m8 = (n + nbar) rounded up to 8
//   bg_ann_rom_run_wide:  [n + nbar][512], zero columns from N; does not read no_reuse
struct AnnRunArgs {
    const double* x;        // [N]
    const double* UT;
    const double* u0;       // [B][N]
    const double* mu1;      // [B]
    const double* mu2;      // [B]
    double* hist;           // [B][nsteps+1][N]
    int32_t* iters;         // [B][nsteps]
    int32_t* flags;         // [B]
    int32_t* info;          // [B]
    const int32_t* order;   // [B] or null: slot i of the persistent loop works on sample order[i]
    AnnModel m;
    double dt, E, tol;
    int N, B, n, nbar, nsteps, max_it, supg, nonuniform, no_reuse;
};

// The model part of an entry point's argument check, after its scalar, projection and mesh checks; fills m.
inline int ann_model_check(int max_n, int n, int nbar, int n_layers, const int* widths, const float* const* wt,
                           const float* const* bias, const int* acts, const float* alphas, AnnModel& m)
{
    if (n > max_n || nbar > ANN_MAX_NBAR || n_layers > ANN_MAX_LAYERS) return BG_ERR_UNSUPPORTED_R;
    if (!widths || !wt || !bias || !acts || !alphas) return BG_ERR_BAD_ARG;
    if (widths[0] != n || widths[n_layers] != nbar) return BG_ERR_BAD_ARG;
    for (int l = 0; l < n_layers; ++l) {
        if (widths[l + 1] < 1 || widths[l + 1] > ANN_MAX_WIDTH) return BG_ERR_UNSUPPORTED_R;
        if (!wt[l] || ((uintptr_t)wt[l] & 15)) return BG_ERR_BAD_ARG;
        if (acts[l] != BG_ACT_NONE && acts[l] != BG_ACT_ELU && acts[l] != BG_ACT_RELU && acts[l] != BG_ACT_TANH) return BG_ERR_BAD_ARG;
        m.wt[l] = wt[l]; m.bias[l] = bias[l]; m.act[l] = acts[l]; m.alpha[l] = alphas[l];
    }
    for (int l = 0; l <= n_layers; ++l) m.width[l] = widths[l];
    m.nl = n_layers;
    return BG_OK;
}

// ---- the layers of N(q_p) and dN/dq_p, float32 forward mode: rows 0 = value, 1 .. NRT-1 = tangent directions ----------
// The caller has put the inputs (zero-padded to a multiple of 4) into s_act[0] and passed a barrier; returns the buffer of
// the outputs.  Layer l on all 256 threads.  A thread owns NCH chunks of 4 outputs -- [4 og, 4 og + 4) and, for NCH = 2,
// the same in the second half of the row: NCH 16-byte weight loads per input k, no guards (the host pads W^T to
// [in4][ld]) -- and every KPw-th group of 4 inputs; lane = (input slice) * P + (output group), so that neighbouring lanes
// read neighbouring 16-byte chunks of a weight row.  The KPw slices are folded inside a row of 16 lanes with DPP shifts
// towards the higher lanes, so that the row total lands in its last P lanes, and across the four rows by
//   SWAP       v_permlane16_swap / v_permlane32_swap (VALU; ds_bpermute would make the LDS pipe the bottleneck).  One swap +
//              add folds two values, and the pairing is chosen so that row rho of the wave ends up with the totals of the
//              NCH outputs NCH rho + e of the thread's 4 NCH, for ALL rows: the value and its tangent rows meet in one
//              lane, which applies bias, activation and derivative scaling in registers -- one barrier per layer;
//   TWO_STAGE  ds_bpermute, the pre-activations through LDS and a second stage with one output per thread.
// With both compiled in, a layer whose slices fill the wave (span == 64) takes the swap fold.  The lanes beyond the span
// hold zeros: the swap-only form adds them unconditionally, the two-stage form keeps them out of the fold.
// Row 0 is computed by the same operations in the same order whatever NRT is.  The skip() bits are those of the timing
// builds of rom_ann_fused.hip; clk gets that file's laps (a PhaseClock<false, .> elsewhere).
template <int NRT, int NCH, bool SWAP, bool TWO_STAGE, int ROWS, class Clock>
__device__ __forceinline__ int ann_layers(const AnnModel& m, float (&s_act)[2][ROWS][ANN_MAX_WIDTH], int tid, int lane, int w,
                                          Clock& clk)
{
    static_assert(NCH == 1 || NCH == 2, "one or two 16-byte chunks of outputs per thread");
    static_assert(SWAP || TWO_STAGE, "a fold across the rows of 16 lanes");
    static_assert(NRT <= ROWS, "rows compiled in");
    constexpr int E = NCH;                                            // outputs a lane finishes in the swap fold
    constexpr int NC = 4 * NCH;                                       // outputs of a thread
    int cur = 0;
    for (int l = 0; l < (skip(128) ? 0 : m.nl); ++l) {               // (128: timing builds only)
        const int in4 = (m.width[l] + 3) & ~3, out = m.width[l + 1], ldw = (out + 7) & ~7, ogn = ldw >> (NCH + 1);
        int P = 1, pshift = 0;
        while (4 * P < ogn) { P <<= 1; ++pshift; }                    // output groups per wave (a power of two, <= 16 / NCH)
        int KPw = 64 >> pshift;                                       // input slices per wave ...
        while (4 * KPw > in4 && KPw > 1) KPw >>= 1;                   // ... at most one per group of 4 inputs (small layers)
        const int span = P * KPw;                                     // lanes of a wave that carry partial sums
        const int kp = lane >> pshift, ogr = w * P + (lane & (P - 1));    // neighbouring lanes: neighbouring 16-byte chunks
        const int og = ogr < ogn ? ogr : ogn - 1;                     // spare lanes redo the last group (no guarded loads)
        const float* __restrict__ wp = m.wt[l] + 4 * og;
        const int half = 4 * ogn;
        // this thread's bias for the second stage, fetched now so that its latency hides behind the layer
        const float bias_v = (TWO_STAGE && m.bias[l]) ? m.bias[l][tid < out ? tid : out - 1] : 0.0f;
        // ... and the E outputs this lane finishes when the layer takes the swap fold: E rho + e of the thread's 4 NCH
        const int rho = lane >> 4;
        const int o0 = ((E * rho) >> 2) * half + 4 * og + ((E * rho) & 3);
        float bias_o[E];
#pragma unroll
        for (int e = 0; e < E; ++e) bias_o[e] = m.bias[l] ? m.bias[l][o0 + e < out ? o0 + e : out - 1] : 0.0f;
        float acc[NRT][NC];
#pragma unroll
        for (int r = 0; r < NRT; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[r][c] = 0.0f;
        auto kload = [&](int kb, float4 (&wv)[4][NCH]) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const float4* src = reinterpret_cast<const float4*>(wp + (size_t)(kb + kk) * ldw);
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    if constexpr (skip(1024)) wv[kk][c] = make_float4(1.0f * kb, 2.0f, 3.0f, 4.0f);   // timing only: no weight traffic
                    else wv[kk][c] = src[c * ogn];
                }
            }
        };
        auto kfma = [&](int kb, const float4 (&wv)[4][NCH]) {
#pragma unroll
            for (int r = 0; r < (skip(512) ? 1 : NRT); ++r) {          // (512: timing only: weight traffic, one row of arithmetic)
                const float4 xv = *reinterpret_cast<const float4*>(&s_act[cur][r][kb]);
                const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        acc[r][4 * c + 0] = __builtin_fmaf(xs[kk], wv[kk][c].x, acc[r][4 * c + 0]);
                        acc[r][4 * c + 1] = __builtin_fmaf(xs[kk], wv[kk][c].y, acc[r][4 * c + 1]);
                        acc[r][4 * c + 2] = __builtin_fmaf(xs[kk], wv[kk][c].z, acc[r][4 * c + 2]);
                        acc[r][4 * c + 3] = __builtin_fmaf(xs[kk], wv[kk][c].w, acc[r][4 * c + 3]);
                    }
                }
            }
        };
        // Two slices per trip (8 NCH weight loads in flight) where the registers allow it: up to 6 rows of 8 outputs, 10 of 4;
        // beyond that the loop spills.  A rolling ring of fetches that also runs ahead into the next layer was tried in
        // rom_ann_fused.hip: with the 256-register budget of two workgroups per CU it spills, and was slower.
        const int kstride = 4 * KPw;
        int kb = kp < KPw ? 4 * kp : in4;                             // lanes beyond the span hold zeros
        if constexpr (NRT * NCH <= 12) {
            for (; kb + kstride < in4; kb += 2 * kstride) {
                float4 wa[4][NCH], wb[4][NCH];
                kload(kb, wa);
                kload(kb + kstride, wb);
                kfma(kb, wa);
                kfma(kb + kstride, wb);
            }
        }
        for (; kb < in4; kb += kstride) {
            float4 wa[4][NCH];
            kload(kb, wa);
            kfma(kb, wa);
        }
        if constexpr (skip(8192)) clk.lap(3);                          // (8192: timing only: sub-phases of a layer summed over the layers)
        auto fold = [&](auto get) {
            if constexpr (skip(2048)) return;                         // timing only
#pragma unroll
            for (int r = 0; r < NRT; ++r)
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[r][c] += get(acc[r][c]);
        };
        auto live = [&](int k) { return !TWO_STAGE || span > k; };    // does the fold over k lanes meet a partial sum?
        if (P <= 1 && live(1)) fold([](float v) { return dpp_f32<0x111>(v); });      // row_shr:1
        if (P <= 2 && live(2)) fold([](float v) { return dpp_f32<0x112>(v); });      // row_shr:2
        if (P <= 4 && live(4)) fold([](float v) { return dpp_f32<0x114>(v); });      // row_shr:4
        if (P <= 8 && live(8)) fold([](float v) { return dpp_f32<0x118>(v); });      // row_shr:8
        const int kind = m.act[l];
        const float alpha = m.alpha[l];
        if constexpr (skip(8192)) clk.lap(4);
        const bool swapfold = SWAP && (!TWO_STAGE || (span == 64 && !skip(2048)));      // workgroup-uniform
        if (swapfold) {
            float res[NRT][E];
#pragma unroll
            for (int r = 0; r < NRT; ++r) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float s01 = swap16_add(acc[r][e], acc[r][E + e]);
                    const float s23 = swap16_add(acc[r][2 * E + e], acc[r][3 * E + e]);
                    res[r][e] = swap32_add(s01, s23);
                }
            }
            if ((lane & 15) >= 16 - P && ogr < ogn) {
                float outv[NRT][E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const bool real = o0 + e < out;
                    float av, d;                                      // bias, activation, derivative scaling
                    mlp_activate(kind, alpha, res[0][e] + (real ? bias_o[e] : 0.0f), av, d);
                    outv[0][e] = real ? av : 0.0f;                    // the padding outputs feed the next layer's padded inputs
#pragma unroll
                    for (int r = 1; r < NRT; ++r) outv[r][e] = real ? ((kind != BG_ACT_NONE) ? res[r][e] * d : res[r][e]) : 0.0f;
                }
#pragma unroll
                for (int r = 0; r < NRT; ++r) {
                    if constexpr (E == 2) *reinterpret_cast<float2*>(&s_act[cur ^ 1][r][o0]) = make_float2(outv[r][0], outv[r][1]);
                    else s_act[cur ^ 1][r][o0] = outv[r][0];
                }
            }
        } else if constexpr (TWO_STAGE) {
            if (span > 16) fold([](float v) { return __shfl_xor(v, 16); });
            if (span > 32) fold([](float v) { return __shfl_xor(v, 32); });
            const int top = span < 16 ? span : 16;                    // the totals sit in the last P lanes below `top`
            if (lane >= top - P && lane < top && ogr < ogn) {         // pre-activations of the thread's outputs, all rows
#pragma unroll
                for (int r = 0; r < NRT; ++r)
#pragma unroll
                    for (int c = 0; c < NCH; ++c)
                        *reinterpret_cast<float4*>(&s_act[cur ^ 1][r][c * half + 4 * og]) =
                            make_float4(acc[r][4 * c], acc[r][4 * c + 1], acc[r][4 * c + 2], acc[r][4 * c + 3]);
            }
        }
        if constexpr (skip(8192)) clk.lap(5);
        __syncthreads();
        if constexpr (skip(8192)) clk.lap(6);
        cur ^= 1;
        if (TWO_STAGE && !swapfold) {                                 // second stage, one output per thread
            if (tid < ldw && !skip(4096)) {
                const bool real = tid < out;
                float av, d;
                mlp_activate(kind, alpha, s_act[cur][0][tid] + (real ? bias_v : 0.0f), av, d);
                if (!real) { av = 0.0f; d = 0.0f; }
                s_act[cur][0][tid] = av;
                if (kind != BG_ACT_NONE || !real) {
#pragma unroll
                    for (int r = 1; r < NRT; ++r) s_act[cur][r][tid] *= d;
                }
            }
            __syncthreads();
        }
        if constexpr (skip(8192)) clk.lap(7);
        else if constexpr (kTiming || kPhaseClock) {                  // per-layer laps of the diagnostic builds
#pragma unroll
            for (int i = 0; i < ANN_MAX_LAYERS; ++i)
                if (i == l) clk.lap(3 + i);
        }
    }
    return cur;
}

}  // namespace fused
}  // namespace bg
