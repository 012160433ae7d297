// wave_ops.hpp -- wave64 cross-lane and arithmetic helpers for gfx950 (CDNA4).
//
// One wavefront owns one Burgers sample; everything below is wave-private (no LDS
// storage, no barriers).  Cross-lane traffic uses DPP moves where the pattern allows
// (1 VALU op per dword) and ds_bpermute (LDS crossbar, no LDS memory) otherwise.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/burgers_hip.h"

namespace bg {

constexpr int WAVE = 64;

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

// ---- DPP moves on doubles ---------------------------------------------------------
// dpp_ctrl encodings (GFX9): wave_shl:1 = 0x130, wave_shr:1 = 0x138,
// row_shr:n = 0x110+n, row_bcast15 = 0x142, row_bcast31 = 0x143.
template <int CTRL, int ROW_MASK = 0xF, bool BOUND_ZERO = true>
__device__ __forceinline__ double dpp_mov(double v, double old = 0.0)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    int olo = __double2loint(old), ohi = __double2hiint(old);
    lo = __builtin_amdgcn_update_dpp(olo, lo, CTRL, ROW_MASK, 0xF, BOUND_ZERO);
    hi = __builtin_amdgcn_update_dpp(ohi, hi, CTRL, ROW_MASK, 0xF, BOUND_ZERO);
    return __hiloint2double(hi, lo);
}

// value held by lane-1 (lane 0 receives 0)
__device__ __forceinline__ double from_lane_below(double v) { return dpp_mov<0x138>(v); }
// value held by lane+1 (lane 63 receives 0)
__device__ __forceinline__ double from_lane_above(double v) { return dpp_mov<0x130>(v); }

// value held by lane (lane + delta) mod 64, any delta; ds_bpermute, 2 ops per double
__device__ __forceinline__ double from_lane_rot(double v, int src_lane_times4)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_ds_bpermute(src_lane_times4, lo);
    hi = __builtin_amdgcn_ds_bpermute(src_lane_times4, hi);
    return __hiloint2double(hi, lo);
}

// ---- wave-wide sum, result broadcast to every lane --------------------------------
// row_shr 1,2,4,8 inside each row of 16, then row_bcast15 / row_bcast31 across rows;
// lane 63 ends up with the total, which is then read back through an SGPR pair.
__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_mov<0x111>(v);            // row_shr:1
    v += dpp_mov<0x112>(v);            // row_shr:2
    v += dpp_mov<0x114>(v);            // row_shr:4
    v += dpp_mov<0x118>(v);            // row_shr:8
    v += dpp_mov<0x142, 0xA>(v);       // row_bcast15 -> rows 1,3
    v += dpp_mov<0x143, 0xC>(v);       // row_bcast31 -> rows 2,3
    int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    return __hiloint2double(hi, lo);
}

// ---- reciprocal: v_rcp_f64 seed (~2^-23 relative) + two Newton steps ---------------
__device__ __forceinline__ double rcp(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    return r;
}

// one Newton step only: 2.1e-15 max relative error measured on gfx950 (tools/microbench.hip);
// used where the consumer is itself an iteration that contracts such perturbations
__device__ __forceinline__ double rcp1(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    return __builtin_fma(r, e, r);
}

// DPP move applied REPS times (wave_shr:1 twice = shift by two lanes, zero filled)
template <int CTRL, int REPS>
__device__ __forceinline__ double dpp_shift(double v)
{
#pragma unroll
    for (int i = 0; i < REPS; ++i) v = dpp_mov<CTRL>(v);
    return v;
}

// two wave-wide sums for little more than the price of one: v_permlane32_swap puts the
// partial sums of `a` in lanes 0..31 and those of `b` in lanes 32..63, then one row scan.
__device__ __forceinline__ void wave_sum2(double a, double b, double& sa, double& sb)
{
    auto l = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    auto h = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    double v = __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
    v += dpp_mov<0x111>(v);            // row_shr:1
    v += dpp_mov<0x112>(v);            // row_shr:2
    v += dpp_mov<0x114>(v);            // row_shr:4
    v += dpp_mov<0x118>(v);            // row_shr:8
    v += dpp_mov<0x142, 0xA>(v);       // row_bcast15 -> rows 1,3
    sa = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 31),
                          __builtin_amdgcn_readlane(__double2loint(v), 31));
    sb = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63),
                          __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// wave_sum2 in its stages, for a caller that has independent work to place between them: each round waits for the one
// before (a DPP move of the running sum, then the add).  start, round<0> ... round<4>, finish are wave_sum2's operations
// in wave_sum2's order.
struct WaveSum2 {
    double v;
    __device__ __forceinline__ void start(double a, double b)
    {
        auto l = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
        auto h = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
        v = __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
    }
    template <int I>
    __device__ __forceinline__ void round()
    {
        if constexpr (I == 0) v += dpp_mov<0x111>(v);
        if constexpr (I == 1) v += dpp_mov<0x112>(v);
        if constexpr (I == 2) v += dpp_mov<0x114>(v);
        if constexpr (I == 3) v += dpp_mov<0x118>(v);
        if constexpr (I == 4) v += dpp_mov<0x142, 0xA>(v);
    }
    __device__ __forceinline__ void finish(double& sa, double& sb) const
    {
        sa = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 31),
                              __builtin_amdgcn_readlane(__double2loint(v), 31));
        sb = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63),
                              __builtin_amdgcn_readlane(__double2loint(v), 63));
    }
};

__device__ __forceinline__ double sel(bool c, double a, double b) { return c ? a : b; }

// inf or NaN in a WAVE-UNIFORM value (every lane holds the same v): exponent field all ones; zeros and denormals are
// finite.  The same predicate as !(v - v == 0.0), but an integer test of the high word on the scalar unit: where v
// already sits in an SGPR pair (the readlane results of wave_sum2) it is an s_and and an s_cmp instead of a v_add_f64
// and a v_cmp_eq_f64.  The empty asm with its SGPR constraint is what keeps it there: the compiler turns every bare
// spelling of the integer test back into a floating-point class compare on the vector unit.  It emits nothing, and
// the readfirstlane folds away on an SGPR operand.
constexpr unsigned F64_EXP_HI = 0x7ff00000u;
__device__ __forceinline__ unsigned uniform_exponent_bits(double v)
{
    unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane(__double2hiint(v));
    asm("" : "+s"(hi));
    return hi & F64_EXP_HI;
}
__device__ __forceinline__ bool uniform_nonfinite(double v) { return uniform_exponent_bits(v) == F64_EXP_HI; }
// either of two (the masked fields are <= F64_EXP_HI, so one s_max_u32 and one compare serve both)
__device__ __forceinline__ bool uniform_nonfinite(double a, double b)
{
    const unsigned ea = uniform_exponent_bits(a), eb = uniform_exponent_bits(b);
    return (ea > eb ? ea : eb) == F64_EXP_HI;
}

// ---- float32: DPP move, and folds across the rows of 16 lanes on the VALU (v_permlane16_swap / v_permlane32_swap) ----
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// a + (a of the neighbouring row) in the even rows of 16 lanes, b + (b of the neighbouring row) in the odd rows
__device__ __forceinline__ float swap16_add(float a, float b)
{
    const auto t = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
    return __builtin_bit_cast(float, (unsigned)t[0]) + __builtin_bit_cast(float, (unsigned)t[1]);
}
// a + (a of the other half) in lanes 0..31, b + (b of the other half) in lanes 32..63
__device__ __forceinline__ float swap32_add(float a, float b)
{
    const auto t = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
    return __builtin_bit_cast(float, (unsigned)t[0]) + __builtin_bit_cast(float, (unsigned)t[1]);
}

// ---- MLP activation of the pre-activation v (bias added): value av and derivative d, the arithmetic of bg_mlp_act_jvp
// (csrc/mlp.hip) but for the ELU value below 0: e - alpha here, alpha expm1(v) there, eps32 alpha / 2 apart at the most, which
// is 1e-8 of the closure where the loops are held to 5e-6 (tests/test_mlp_stage_gpu.py).  BG_ACT_NONE: av = v, d = 1
__device__ __forceinline__ void mlp_activate(int kind, float alpha, float v, float& av, float& d)
{
    av = v; d = 1.0f;
    if (kind == BG_ACT_ELU) {
        const float e = alpha * expf(v);
        av = v > 0.0f ? v : e - alpha;
        d = v > 0.0f ? 1.0f : e;
    } else if (kind == BG_ACT_RELU) {
        av = v > 0.0f ? v : 0.0f;
        d = v > 0.0f ? 1.0f : 0.0f;
    } else if (kind == BG_ACT_TANH) {
        av = tanhf(v);
        d = 1.0f - av * av;
    }
}

// ---- phase clock of the diagnostic builds (-DBG_PHASE_CLOCK; never defined in the product build) ---------------------
// A device-side time loop constructs one per sample: lap(i) adds the shader clocks since the previous lap (or the
// construction) to slot i, pass() counts a Picard / Gauss-Newton pass, store() overwrites the head of the sample's row
// of iteration counts with the one record tools/_timing.py (phase_report) reads:
//   [0, SLOTS) kilo-clocks per phase (>> 10) | [SLOTS] passes | [SLOTS + 1] shader kilo-clocks, [SLOTS + 2] 100 MHz
//   kilo-ticks since construction; nothing when the run has fewer than SLOTS + 3 time steps.  ON = false is empty.
#ifdef BG_PHASE_CLOCK
constexpr bool kPhaseClock = true;
#else
constexpr bool kPhaseClock = false;
#endif

template <bool ON, int SLOTS>
struct PhaseClock {
    long long cyc[SLOTS] = {};
    long long real0, tick;
    int passes = 0;
    __device__ __forceinline__ PhaseClock()
        : real0((long long)__builtin_amdgcn_s_memrealtime()), tick((long long)__builtin_amdgcn_s_memtime()) {}
    __device__ __forceinline__ void lap(int i)
    {
        const long long now = (long long)__builtin_amdgcn_s_memtime();
        cyc[i] += now - tick;
        tick = now;
    }
    __device__ __forceinline__ void pass() { ++passes; }
    __device__ __forceinline__ void store(int32_t* iters_row, int nsteps) const
    {
        if (nsteps < SLOTS + 3) return;
        long long total = (long long)__builtin_amdgcn_s_memtime() - tick;      // the laps partition the time before `tick`
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            iters_row[i] = (int)(cyc[i] >> 10);
            total += cyc[i];
        }
        iters_row[SLOTS] = passes;
        iters_row[SLOTS + 1] = (int)(total >> 10);
        iters_row[SLOTS + 2] = (int)(((long long)__builtin_amdgcn_s_memrealtime() - real0) >> 10);
    }
};
template <int SLOTS>
struct PhaseClock<false, SLOTS> {
    __device__ __forceinline__ void lap(int) const {}
    __device__ __forceinline__ void pass() const {}
    __device__ __forceinline__ void store(int32_t*, int) const {}
};

}  // namespace bg
