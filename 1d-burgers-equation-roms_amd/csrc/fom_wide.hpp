// fom_wide.hpp -- one WORKGROUP (4 wavefronts) per sample, for meshes beyond one wavefront's
// registers (1536 < N <= 8192), and the two topologies (WaveTopo, WgTopo, at the end) over which
// the FEM bodies of fom.hip and the FD body of fd.hip are written once.  Same arithmetic as
// fom_device.hpp; what changes is where the halo values come from and how the 256 interface
// equations of the Wang partition are solved.
//
// Row distribution: thread g = 64*wave + lane of the workgroup owns the R consecutive rows
// [g*R, g*R + R), N <= 256*R.  Neighbour values travel through LDS arrays indexed by g with two
// zero pads on either side (the zero fill the DPP shifts give inside one wave).
//
// Interface system (256 normalised equations, one per thread): parallel cyclic reduction.  The
// equations are re-dealt so that equation e sits in wave e & 3, lane e >> 2; the strides 1 and 2
// then cross waves (two LDS exchanges), after which the four interleaved stride-4 systems each
// live in one wave in lane order and finish with the in-wave pcr64 of fom_device.hpp.
#pragma once
#include "fom_device.hpp"

namespace bg {

constexpr int WIDE_WAVES = 4;
constexpr int WIDE_THREADS = 64 * WIDE_WAVES;
constexpr int WIDE_PAD = 2;
constexpr int WIDE_LEN = WIDE_THREADS + 2 * WIDE_PAD;

struct WideLds {
    double ufirst[WIDE_LEN], ulast[WIDE_LEN];   // u of every thread's first / last row
    double se[WIDE_LEN];                        // SUPG term of every thread's last element
    double fgr[3][WIDE_LEN];                    // normalised row 0 of every thread (F0, G0, R0)
    double pcr[2][3][WIDE_LEN];                 // interface equations (A, C, D), double-buffered
    double x[WIDE_LEN];                         // interface unknowns
    double nrm[2][WIDE_WAVES];                  // per-wave partial norms
};

// pads are written once; every later store goes to [WIDE_PAD, WIDE_PAD + 256)
__device__ __forceinline__ void wide_init(WideLds& s, int tid)
{
    double* p = reinterpret_cast<double*>(&s);
    for (int i = tid; i < (int)(sizeof(WideLds) / sizeof(double)); i += WIDE_THREADS) p[i] = 0.0;
    __syncthreads();
}

// Parked rows: at 32 rows per thread the per-row constants of a whole time step, g = M u^n + dt F and hfs, no longer fit
// the register file beside the solver's working set (404 bytes of scratch per thread).  The uniform-mesh N > 6144 kernel
// keeps them in LDS instead, row-major over threads (park[j][g]: consecutive threads, consecutive addresses) and reads
// each value where the assembly uses it.
template <int R>
struct WidePark {
    double g[R][WIDE_THREADS];
    double hfs[R][WIDE_THREADS];
};

// One PCR step of stride S on equation e, neighbours from the LDS copy `buf` of all equations.
template <int S>
__device__ __forceinline__ void wide_pcr_step(const double (&buf)[3][WIDE_LEN], int e, double& A, double& C, double& D)
{
    const int m = e + WIDE_PAD - S, p = e + WIDE_PAD + S;
    const double Am = buf[0][m], Cm = buf[1][m], Dm = buf[2][m];
    const double Ap = buf[0][p], Cp = buf[1][p], Dp = buf[2][p];
    double Bn = __builtin_fma(-Cm, A, 1.0);
    Bn = __builtin_fma(-Ap, C, Bn);
    double Dn = __builtin_fma(-Dm, A, D);
    Dn = __builtin_fma(-Dp, C, Dn);
    const double rb = BG_RCP(Bn);
    D = Dn * rb;
    A = -(Am * A) * rb;
    C = -(Cp * C) * rb;
}

// Pivot-free tridiagonal solve across the workgroup.  In: lo/di/up/rhs.  Out: solution in rhs (SCALE: see wang_finish).
template <int R, bool SCALE = true>
__device__ __forceinline__ void wide_tridiag_solve(WideLds& s, int g, double (&lo)[R], double (&di)[R],
                                                   const double (&up)[R], double (&rhs)[R])
{
    double gs[R];
    const double dp = wang_reduce<R>(lo, di, up, rhs, gs);
    s.fgr[0][g + WIDE_PAD] = lo[0] * di[0];
    s.fgr[1][g + WIDE_PAD] = gs[0] * di[0];
    s.fgr[2][g + WIDE_PAD] = rhs[0] * di[0];
    __syncthreads();
    double A, C, D;
    wang_interface<R>(lo, up, rhs, dp, s.fgr[0][g + WIDE_PAD + 1], s.fgr[1][g + WIDE_PAD + 1],
                      s.fgr[2][g + WIDE_PAD + 1], A, C, D);
    s.pcr[0][0][g + WIDE_PAD] = A;
    s.pcr[0][1][g + WIDE_PAD] = C;
    s.pcr[0][2][g + WIDE_PAD] = D;
    __syncthreads();
    const int e = (g & 63) * WIDE_WAVES + (g >> 6);          // the equation this thread carries through the PCR
    A = s.pcr[0][0][e + WIDE_PAD]; C = s.pcr[0][1][e + WIDE_PAD]; D = s.pcr[0][2][e + WIDE_PAD];
    wide_pcr_step<1>(s.pcr[0], e, A, C, D);
    s.pcr[1][0][e + WIDE_PAD] = A;
    s.pcr[1][1][e + WIDE_PAD] = C;
    s.pcr[1][2][e + WIDE_PAD] = D;
    __syncthreads();
    wide_pcr_step<2>(s.pcr[1], e, A, C, D);
    s.x[e + WIDE_PAD] = pcr64<R>(A, C, D);                   // stride-4 system e & 3 = this wave, in lane order
    __syncthreads();
    wang_finish<R, SCALE>(lo, di, rhs, gs, s.x[g + WIDE_PAD], s.x[g + WIDE_PAD - 1]);
}

// sums over the whole workgroup, the same value in every thread (fixed summation order)
__device__ __forceinline__ void wide_sum2(WideLds& s, int g, double a, double b, double& sa, double& sb)
{
    wave_sum2(a, b, a, b);
    if ((g & 63) == 0) { s.nrm[0][g >> 6] = a; s.nrm[1][g >> 6] = b; }
    __syncthreads();
    sa = (s.nrm[0][0] + s.nrm[0][1]) + (s.nrm[0][2] + s.nrm[0][3]);
    sb = (s.nrm[1][0] + s.nrm[1][1]) + (s.nrm[1][2] + s.nrm[1][3]);
}

__device__ __forceinline__ double wave_max(double v)
{
    v = fmax(v, dpp_mov<0x111>(v));
    v = fmax(v, dpp_mov<0x112>(v));
    v = fmax(v, dpp_mov<0x114>(v));
    v = fmax(v, dpp_mov<0x118>(v));
    v = fmax(v, dpp_mov<0x142, 0xA>(v));
    v = fmax(v, dpp_mov<0x143, 0xC>(v));
    int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    return __hiloint2double(hi, lo);
}

// wave_max of v >= 0 as np.max has it: NaN when `nan` holds in any lane (fmax alone drops a NaN operand).  `nan` is one
// bit per lane, so it rides on a ballot beside the reduction that is there anyway.
__device__ __forceinline__ double wave_max_nan(double v, bool nan)
{
    const double m = wave_max(v);
    return __builtin_amdgcn_ballot_w64(nan) ? __builtin_nan("") : m;
}

// ---- the topology of a sample: what the FEM bodies (fom.hip) and the FD body (fd.hip) are written over ----
// Thread g of the sample's threads owns the rows [g*R, g*R + R).  Where neighbour values, sums, maxima and the
// tridiagonal solve come from: one wavefront per sample (DPP inside the wave, no barrier anywhere) or one 256-thread
// workgroup per sample (LDS across its four waves).  Values from outside the sample's threads are 0.
//   halo        uL / uR = `last` of thread g-1 / `first` of thread g+1, one exchange.  The workgroup form needs
//               halo_done() before the next halo() (it refills ufirst / ulast); the wave form's is empty.
//   below_se    v of thread g-1 through WideLds::se: once per Picard iteration, the solve's barriers lie between two uses
//   below, above, gmax, gmax_nan   the FD stepper's exchanges: alternating buffers, so one barrier each in any sequence.
//               gmax_nan(v, nan): gmax of v >= 0, NaN when `nan` holds in any of the sample's threads (np.max, not fmax)
//   rotates_picard   whether fom_sample may form the next iterate's assemble_head ahead of sum2 (BG_PICARD_ROTATE): the wave
//               form's exchanges are DPP moves and order freely; the workgroup form's halo() and below_se() refill LDS
//               buffers between barriers, and a halo() in front of sum2's barrier has not been argued
//   ONESIDED    (one wavefront per sample) the solve closes its interface system by the one-sided route of pcr64 where a
//               lane owns enough rows; for kernels whose systems couple upwards only
template <bool ONESIDED>
struct WaveTopoT {
    static constexpr bool rotates_picard = true;
    int g;                                           // = lane
    __device__ __forceinline__ bool first() const { return g == 0; }        // owns global row 0
    __device__ __forceinline__ bool last() const { return g == 63; }        // owns the last row when N = 64 R (FULL)
    __device__ __forceinline__ void halo(double first, double last, double& uL, double& uR)
    {
        uL = from_lane_below(last);
        uR = from_lane_above(first);
    }
    __device__ __forceinline__ void halo_done() {}
    __device__ __forceinline__ double below_se(double v) { return from_lane_below(v); }
    __device__ __forceinline__ double below(double v) { return from_lane_below(v); }
    __device__ __forceinline__ double above(double v) { return from_lane_above(v); }
    __device__ __forceinline__ double gmax(double v) { return wave_max(v); }
    __device__ __forceinline__ double gmax_nan(double v, bool nan) { return wave_max_nan(v, nan); }
    __device__ __forceinline__ void sum2(double a, double b, double& sa, double& sb) { wave_sum2(a, b, sa, sb); }
    template <int R, bool SCALE = true>
    __device__ __forceinline__ void solve(double (&lo)[R], double (&di)[R], const double (&up)[R], double (&rhs)[R])
    {
        tridiag_solve<R, ONESIDED, SCALE>(lo, di, up, rhs);
    }
};
using WaveTopo = WaveTopoT<false>;

struct WgTopo {
    static constexpr bool rotates_picard = false;
    WideLds& s;
    int g;                                           // = threadIdx.x
    int par;                                         // alternating exchange buffers: one barrier per exchange
    __device__ __forceinline__ bool first() const { return g == 0; }
    __device__ __forceinline__ bool last() const { return g == WIDE_THREADS - 1; }
    __device__ __forceinline__ void halo(double first, double last, double& uL, double& uR)
    {
        s.ufirst[g + WIDE_PAD] = first;
        s.ulast[g + WIDE_PAD] = last;
        __syncthreads();
        uL = s.ulast[g + WIDE_PAD - 1];
        uR = s.ufirst[g + WIDE_PAD + 1];
    }
    __device__ __forceinline__ void halo_done() { __syncthreads(); }
    __device__ __forceinline__ double below_se(double v)
    {
        s.se[g + WIDE_PAD] = v;
        __syncthreads();
        return s.se[g + WIDE_PAD - 1];
    }
    __device__ __forceinline__ double shift(double v, int d)
    {
        double* buf = par ? s.ulast : s.ufirst;
        par ^= 1;
        buf[g + WIDE_PAD] = v;
        __syncthreads();
        return buf[g + WIDE_PAD + d];
    }
    __device__ __forceinline__ double below(double v) { return shift(v, -1); }
    __device__ __forceinline__ double above(double v) { return shift(v, +1); }
    __device__ __forceinline__ double gmax(double v)
    {
        v = wave_max(v);
        double* buf = s.nrm[par];
        par ^= 1;
        if ((g & 63) == 0) buf[g >> 6] = v;
        __syncthreads();
        return fmax(fmax(buf[0], buf[1]), fmax(buf[2], buf[3]));
    }
    __device__ __forceinline__ double gmax_nan(double v, bool nan)
    {
        v = wave_max_nan(v, nan);
        double* buf = s.nrm[par];
        par ^= 1;
        if ((g & 63) == 0) buf[g >> 6] = v;
        __syncthreads();
        const double b0 = buf[0], b1 = buf[1], b2 = buf[2], b3 = buf[3];
        const double m = fmax(fmax(b0, b1), fmax(b2, b3));
        return ((b0 != b0) | (b1 != b1) | (b2 != b2) | (b3 != b3)) ? __builtin_nan("") : m;
    }
    __device__ __forceinline__ void sum2(double a, double b, double& sa, double& sb) { wide_sum2(s, g, a, b, sa, sb); }
    template <int R, bool SCALE = true>
    __device__ __forceinline__ void solve(double (&lo)[R], double (&di)[R], const double (&up)[R], double (&rhs)[R])
    {
        wide_tridiag_solve<R, SCALE>(s, g, lo, di, up, rhs);
    }
};

}  // namespace bg
