// rom_wide_device.hpp -- what the two LDS-streaming POD loops for the thesis' LARGER bases (40 < r <= 96) share:
// bg_rom_run_wide (rom_wide.hip, N <= 512) and bg_rom_run_long_wide (rom_long_wide.hip, 513 <= N <= 1024).  The loop itself is
// rom_stream_device.hpp's; here are the layout constants, the 96 x 96 solve by all four waves (wide_solve) and the
// description WidePod, which the long kernel's description LongWidePod derives from; and wide_solve_pivoted, the same solve
// with partial pivoting, which the hyper-reduced wide loop's repair kernel (rom_hyper_wide.hip) and bg_wide_solve_pivoted
// (wide_solve.hip) call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rom_stream_device.hpp"

namespace bg {

constexpr int WR = 96;                 // padded reduced dimension: column 24 t + c  <->  (lane index t, block c)
constexpr int WNB = 24;                // 4-column blocks
constexpr int WPS = 98;                // doubles per row of the LDS slabs and of the parked system (16-byte aligned rows)
constexpr int WNMAX = 512;             // mesh rows

typedef __attribute__((address_space(3))) double lds_double_t;
typedef __attribute__((address_space(3))) int lds_int_t;

// The 96 x 96 solve of one iteration by all four waves: ONE out-of-line copy for every wave and both halves of the panel
// range (the wave number and the panel are run-time values here).  Inlined into the four per-wave bodies and unrolled over
// its 24 panels it was 160 KB of straight-line code per pass and CU -- four waves streaming four different copies through
// the instruction cache -- and took longer than the projection (111 k of 218 k clocks per pass).
// In: the parked system S (Ar | br, LSPG: upper blocks).  Out: s_diag, s_y (x_k = y_k / d_k), s_bad[w] = guard of this wave.
// wave w owns the column blocks b = w, w + 4, ... (six of 24); the right-hand side rides with wave 3.
// col[s][tile][tt] = entry (row 64 tile + lane, column 4 (w + 4 s) + tt).  Contains workgroup barriers: all waves call it.
template <bool GAL>
static __device__ __attribute__((noinline)) void wide_solve(const lds_double_t* S, lds_double_t* s_m, lds_double_t* s_diag, lds_double_t* s_y,
                                                     lds_int_t* s_bad, int w, int lane, int r)
{
    double col[6][2][4], rhs[2];
    auto entry = [&](int i, int j) -> double {   // (Ar | br)[i][j]; LSPG: the lower blocks by symmetry
        int rr = i, cc = j;
        if (!GAL && j < WR && (i % 24) > (j % 24)) { rr = j; cc = i; }
        return S[rr * WPS + cc];
    };
#pragma unroll
    for (int tile = 0; tile < 2; ++tile) {
        const int row = 64 * tile + lane;
        const bool rin = row < WR;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int j = 4 * (w + 4 * s) + tt;
                double v = 0.0;
                if (rin) v = (row >= r || j >= r) ? ((row == j) ? 1.0 : 0.0) : entry(row, j);
                col[s][tile][tt] = v;
            }
        }
        rhs[tile] = (w == 3 && rin && row < r) ? -entry(row, WR) : 0.0;
    }
    double gmax = 0.0;
    bool zero_piv = false;
    // factor the panel p held in slot OS (pivot rows in row tile TK); multipliers of all 96 rows -> s_m[p & 1][kk][row]
    auto factor = [&](int p, auto os_c, auto tk_c) {
        constexpr int OS = decltype(os_c)::value, TK = decltype(tk_c)::value;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int kr = 4 * p + kk, lk = kr & 63;
            const double piv = readlane_f64(col[OS][TK][kk], lk);
            const double rp = rcp(piv);
            zero_piv = zero_piv | (piv == 0.0);
            double pvj[4];
#pragma unroll
            for (int jj = kk + 1; jj < 4; ++jj) pvj[jj] = readlane_f64(col[OS][TK][jj], lk);
#pragma unroll
            for (int tile = 0; tile < 2; ++tile) {
                const int row = 64 * tile + lane;
                const double m = (row != kr && row < WR) ? col[OS][tile][kk] * rp : 0.0;    // rows above the pivot too
                gmax = fmax(gmax, (row > kr) ? fabs(m) : 0.0);
#pragma unroll
                for (int jj = kk + 1; jj < 4; ++jj) col[OS][tile][jj] = __builtin_fma(-m, pvj[jj], col[OS][tile][jj]);
                if (row < WR) s_m[((p & 1) * 4 + kk) * WR + row] = m;
            }
        }
    };
    // apply panel p (multipliers m, pivot rows in row tile TK) to the block in slot SL
    auto apply = [&](int p, auto sl_c, auto tk_c, const double (&m)[4][2]) {
        constexpr int SL = decltype(sl_c)::value, TK = decltype(tk_c)::value;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int lk = (4 * p + kk) & 63;
            double pv[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) pv[tt] = readlane_f64(col[SL][TK][tt], lk);
#pragma unroll
            for (int tile = 0; tile < 2; ++tile)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) col[SL][tile][tt] = __builtin_fma(-m[kk][tile], pv[tt], col[SL][tile][tt]);
        }
    };
    // `slot` is a run-time value: pick the register block with a (wave-uniform) switch
    auto with_slot = [&](int slot, auto&& f) {
        switch (slot) {
            case 0: f(std::integral_constant<int, 0>{}); break;
            case 1: f(std::integral_constant<int, 1>{}); break;
            case 2: f(std::integral_constant<int, 2>{}); break;
            case 3: f(std::integral_constant<int, 3>{}); break;
            case 4: f(std::integral_constant<int, 4>{}); break;
            default: f(std::integral_constant<int, 5>{}); break;
        }
    };
    __syncthreads();                               // every wave has its columns: the parked system is dead
    if (w == 0) factor(0, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    __syncthreads();
    // One barrier per panel: while the other waves apply panel p to their later blocks, the owner of panel p + 1 brings that
    // block up to date first, factors it and publishes its multipliers (look-ahead), then does the rest.
    double mprev[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    auto panels = [&](int p0, int p1, auto tk_c, auto tkprev_c) {   // pivots of panels [p0, p1) in row tile TK, of panel p0 - 1 in TKPREV
#pragma unroll 1
        for (int p = p0; p < p1; ++p) {
            double m[4][2];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                m[kk][0] = s_m[((p & 1) * 4 + kk) * WR + lane];
                m[kk][1] = (lane < WR - 64) ? s_m[((p & 1) * 4 + kk) * WR + 64 + lane] : 0.0;
            }
            const int nxt = p + 1;
            const bool owner_next = nxt < WNB && (nxt & 3) == w;
            const bool owner_this = p > 0 && (p & 3) == w;       // owned panel p: its other blocks still lack panel p - 1
            if (owner_next) {
                with_slot(nxt >> 2, [&](auto sl) {
                    apply(p, sl, tk_c, m);
                    if (nxt < 16) factor(nxt, sl, std::integral_constant<int, 0>{});
                    else factor(nxt, sl, std::integral_constant<int, 1>{});
                });
            } else {
                // the wave that factors the next panel leaves its other blocks for the next round (it is on the critical
                // path: one block update + one factorisation against six block updates of the others)
                auto own = [&](auto sl) {                  // this wave's block in slot SL
                    const int b = w + 4 * decltype(sl)::value;
                    if (b > p) {
                        if (owner_this) apply(p - 1, sl, tkprev_c, mprev);
                        apply(p, sl, tk_c, m);
                    }
                };
                own(std::integral_constant<int, 0>{}); own(std::integral_constant<int, 1>{}); own(std::integral_constant<int, 2>{});
                own(std::integral_constant<int, 3>{}); own(std::integral_constant<int, 4>{}); own(std::integral_constant<int, 5>{});
            }
            if (w == 3) {
                constexpr int TK = decltype(tk_c)::value;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int lk = (4 * p + kk) & 63;
                    const double pv = readlane_f64(rhs[TK], lk);
                    rhs[0] = __builtin_fma(-m[kk][0], pv, rhs[0]);
                    rhs[1] = __builtin_fma(-m[kk][1], pv, rhs[1]);
                }
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) { mprev[kk][0] = m[kk][0]; mprev[kk][1] = m[kk][1]; }
            if (p + 1 < WNB) __syncthreads();
        }
    };
    using T0 = std::integral_constant<int, 0>;
    using T1 = std::integral_constant<int, 1>;
    panels(0, 16, T0{}, T0{});
    panels(16, 17, T1{}, T0{});                    // panel 16's deferred predecessor (15) has its pivots in the first row tile
    panels(17, WNB, T1{}, T1{});
    // what is left is diagonal: x_k = y_k / d_k.  Publish d (the owner of each column) and y (wave 3).
#pragma unroll
    for (int s = 0; s < 6; ++s) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int j = 4 * (w + 4 * s) + tt;   // this column's diagonal entry sits in row j
            if (lane == (j & 63)) s_diag[j] = (j >> 6) ? col[s][1][tt] : col[s][0][tt];
        }
    }
    if (w == 3) {
        s_y[lane] = rhs[0];
        if (lane < WR - 64) s_y[64 + lane] = rhs[1];
    }
    {
        const unsigned long long anybad = __ballot(zero_piv | !(gmax <= 1.0));
        if (lane == 0) s_bad[w] = anybad != 0ull;
    }
    __syncthreads();
}

// ints of LDS wide_solve_pivoted keeps besides wide_solve's arrays: the pivot rows of the current and the next panel
// (double-buffered like s_m), info, and the pivot row of every column (the permutation)
constexpr int WPIV_INFO = 8, WPIV_PERM = 16, WPIV_INTS = WPIV_PERM + WR;

// max over the wave of values >= 0 (and -1 for "no candidate"), broadcast: wave_sum's DPP ladder with fmax.  The ladder fills
// lanes without a source with 0, so the result is max(0, the maximum): what the pivot search wants, a column without a
// positive candidate reads 0.  fmax drops a NaN operand.
__device__ __forceinline__ double wave_max_nonneg(double v)
{
    v = fmax(v, dpp_mov<0x111>(v));            // row_shr:1
    v = fmax(v, dpp_mov<0x112>(v));            // row_shr:2
    v = fmax(v, dpp_mov<0x114>(v));            // row_shr:4
    v = fmax(v, dpp_mov<0x118>(v));            // row_shr:8
    v = fmax(v, dpp_mov<0x142, 0xA>(v));       // row_bcast15 -> rows 1,3
    v = fmax(v, dpp_mov<0x143, 0xC>(v));       // row_bcast31 -> rows 2,3
    return readlane_f64(v, 63);
}

// wide_solve with PARTIAL PIVOTING as an implicit permutation: the same inputs, register layout, panels, look-ahead and one
// barrier per panel, but the pivot of column k is the largest |a| among the rows not yet used as a pivot (the lowest row wins
// ties: LAPACK's choice), and no row moves: row p_k stays where it is and every other row, used or not, is eliminated against
// it (Gauss-Jordan).  The panel's owner searches inside `factor`, column by column, and publishes p_k beside the multipliers
// (s_piv[(p & 1) * 4 + kk]); every wave reads pivot-row entries with readlane at the run-time lane p_k & 63 of row tile
// p_k >> 6 (wave-uniform).  Multipliers of unused rows are at most 1 by construction: there is no guard.
// Out: s_diag[k] = a[p_k][k], s_y[k] = y[p_k] (x_k = y_k / d_k as for wide_solve), s_piv[WPIV_PERM + k] = p_k,
// s_piv[WPIV_INFO] = 0, or k + 1 for the first column k without a non-zero candidate (LAPACK's info: exactly singular; the
// elimination goes on with that column's multipliers 0, its x is not a solution).
// Every loop has fixed bounds and every readlane index is masked to 0 .. 63.  Contains workgroup barriers: all waves call it,
// and the caller has a barrier between reading the outputs and the next call.
template <bool GAL>
static __device__ __attribute__((noinline)) void wide_solve_pivoted(const lds_double_t* S, lds_double_t* s_m, lds_double_t* s_diag,
                                                                    lds_double_t* s_y, lds_int_t* s_piv, int w, int lane, int r)
{
    double col[6][2][4], rhs[2];
    auto entry = [&](int i, int j) -> double {   // (Ar | br)[i][j]; LSPG: the lower blocks by symmetry
        int rr = i, cc = j;
        if (!GAL && j < WR && (i % 24) > (j % 24)) { rr = j; cc = i; }
        return S[rr * WPS + cc];
    };
#pragma unroll
    for (int tile = 0; tile < 2; ++tile) {
        const int row = 64 * tile + lane;
        const bool rin = row < WR;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int j = 4 * (w + 4 * s) + tt;
                double v = 0.0;
                if (rin) v = (row >= r || j >= r) ? ((row == j) ? 1.0 : 0.0) : entry(row, j);
                col[s][tile][tt] = v;
            }
        }
        rhs[tile] = (w == 3 && rin && row < r) ? -entry(row, WR) : 0.0;
    }
    bool used[2] = {false, lane >= WR - 64};       // this lane's row of each tile has been a pivot (rows beyond 96: never one)
    if (w == 0 && lane == 0) s_piv[WPIV_INFO] = 0;
    // entries of the row `pk` (wave-uniform) of a register block
    auto tile_of = [](int pk) -> bool { return ((pk >> 6) & 1) != 0; };
    auto mark_used = [&](int pk) {
        used[0] = used[0] | (lane == pk);
        used[1] = used[1] | (64 + lane == pk);
    };
    // factor the panel p held in slot OS: search the pivot of each of its columns, multipliers of all 96 rows -> s_m[p & 1][kk][row]
    auto factor = [&](int p, auto os_c) {
        constexpr int OS = decltype(os_c)::value;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = 4 * p + kk;
            const double c0 = used[0] ? -1.0 : fabs(col[OS][0][kk]), c1 = used[1] ? -1.0 : fabs(col[OS][1][kk]);
            const double vmax = wave_max_nonneg(fmax(c0, c1));
            const unsigned long long b0 = __ballot(c0 == vmax), b1 = __ballot(c1 == vmax);
            int pk = b0 ? (int)__builtin_ctzll(b0) : 64 + (b1 ? (int)__builtin_ctzll(b1) : 0);     // the lowest row among the largest
            pk = __builtin_amdgcn_readfirstlane(pk < WR ? pk : WR - 1);
            const int lk = pk & 63;
            const bool t1 = tile_of(pk);
            const double piv = readlane_f64(sel(t1, col[OS][1][kk], col[OS][0][kk]), lk);
            const bool singular = !(vmax > 0.0);
            const double rp = singular ? 0.0 : rcp(piv);
            double pvj[4];
#pragma unroll
            for (int jj = kk + 1; jj < 4; ++jj) pvj[jj] = readlane_f64(sel(t1, col[OS][1][jj], col[OS][0][jj]), lk);
#pragma unroll
            for (int tile = 0; tile < 2; ++tile) {
                const int row = 64 * tile + lane;
                const double m = (row != pk && row < WR) ? col[OS][tile][kk] * rp : 0.0;    // used rows too; 0 for the pivot row
#pragma unroll
                for (int jj = kk + 1; jj < 4; ++jj) col[OS][tile][jj] = __builtin_fma(-m, pvj[jj], col[OS][tile][jj]);
                if (row < WR) s_m[((p & 1) * 4 + kk) * WR + row] = m;
            }
            mark_used(pk);
            if (lane == 0) {
                s_piv[(p & 1) * 4 + kk] = pk;
                s_piv[WPIV_PERM + k] = pk;
                s_diag[k] = piv;                   // column k is not touched again: a[p_k][k] at the end
                if (singular && s_piv[WPIV_INFO] == 0) s_piv[WPIV_INFO] = k + 1;
            }
        }
    };
    // apply a panel (multipliers m, pivot rows pk) to the block in slot SL
    auto apply = [&](auto sl_c, const double (&m)[4][2], const int (&pk)[4]) {
        constexpr int SL = decltype(sl_c)::value;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int lk = pk[kk] & 63;
            const bool t1 = tile_of(pk[kk]);
            double pv[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) pv[tt] = readlane_f64(sel(t1, col[SL][1][tt], col[SL][0][tt]), lk);
#pragma unroll
            for (int tile = 0; tile < 2; ++tile)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) col[SL][tile][tt] = __builtin_fma(-m[kk][tile], pv[tt], col[SL][tile][tt]);
        }
    };
    // `slot` is a run-time value: pick the register block with a (wave-uniform) switch
    auto with_slot = [&](int slot, auto&& f) {
        switch (slot) {
            case 0: f(std::integral_constant<int, 0>{}); break;
            case 1: f(std::integral_constant<int, 1>{}); break;
            case 2: f(std::integral_constant<int, 2>{}); break;
            case 3: f(std::integral_constant<int, 3>{}); break;
            case 4: f(std::integral_constant<int, 4>{}); break;
            default: f(std::integral_constant<int, 5>{}); break;
        }
    };
    __syncthreads();                               // every wave has its columns: the parked system is dead
    if (w == 0) factor(0, std::integral_constant<int, 0>{});
    __syncthreads();
    // One barrier per panel and the look-ahead of wide_solve: while the other waves apply panel p to their later blocks, the
    // owner of panel p + 1 brings that block up to date first, factors it and publishes its multipliers and pivot rows.
    double mprev[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    int pkprev[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int p = 0; p < WNB; ++p) {
        double m[4][2];
        int pk[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            m[kk][0] = s_m[((p & 1) * 4 + kk) * WR + lane];
            m[kk][1] = (lane < WR - 64) ? s_m[((p & 1) * 4 + kk) * WR + 64 + lane] : 0.0;
            pk[kk] = __builtin_amdgcn_readfirstlane(s_piv[(p & 1) * 4 + kk]) & 127;
            mark_used(pk[kk]);
        }
        const int nxt = p + 1;
        const bool owner_next = nxt < WNB && (nxt & 3) == w;
        const bool owner_this = p > 0 && (p & 3) == w;       // owned panel p: its other blocks still lack panel p - 1
        if (owner_next) {
            with_slot(nxt >> 2, [&](auto sl) {
                apply(sl, m, pk);
                factor(nxt, sl);
            });
        } else {
            auto own = [&](auto sl) {                  // this wave's block in slot SL
                const int b = w + 4 * decltype(sl)::value;
                if (b > p) {
                    if (owner_this) apply(sl, mprev, pkprev);
                    apply(sl, m, pk);
                }
            };
            own(std::integral_constant<int, 0>{}); own(std::integral_constant<int, 1>{}); own(std::integral_constant<int, 2>{});
            own(std::integral_constant<int, 3>{}); own(std::integral_constant<int, 4>{}); own(std::integral_constant<int, 5>{});
        }
        if (w == 3) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const double pv = readlane_f64(sel(tile_of(pk[kk]), rhs[1], rhs[0]), pk[kk] & 63);
                rhs[0] = __builtin_fma(-m[kk][0], pv, rhs[0]);
                rhs[1] = __builtin_fma(-m[kk][1], pv, rhs[1]);
            }
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) { mprev[kk][0] = m[kk][0]; mprev[kk][1] = m[kk][1]; pkprev[kk] = pk[kk]; }
        if (p + 1 < WNB) __syncthreads();
    }
    // what is left is a row-scaled permutation: x_k = y[p_k] / a[p_k][k].  The diagonal went out with each pivot; wave 3
    // gathers y through the permutation (ds_bpermute: every lane of the wave takes part).
    if (w == 3) {
        const int pa = s_piv[WPIV_PERM + lane] & 127, pb = s_piv[WPIV_PERM + 64 + (lane & 31)] & 127;
        const double ya0 = from_lane_rot(rhs[0], 4 * (pa & 63)), ya1 = from_lane_rot(rhs[1], 4 * (pa & 63));
        const double yb0 = from_lane_rot(rhs[0], 4 * (pb & 63)), yb1 = from_lane_rot(rhs[1], 4 * (pb & 63));
        s_y[lane] = tile_of(pa) ? ya1 : ya0;
        if (lane < WR - 64) s_y[64 + lane] = tile_of(pb) ? yb1 : yb0;
    }
    __syncthreads();
}

struct WidePod {
    using Args = StreamRunArgs;
    static constexpr bool local = false;
    static constexpr int NB = WNB, PS = WPS, SW = WPS, NMAX = WNMAX;
    static constexpr bool cf_by_mesh_row = true;        // lo, di, up, R of all 512 mesh rows stay in LDS
    static constexpr bool mirror_lspg = false;          // wide_solve reads the lower blocks by symmetry
    static constexpr bool has_repair = false;           // marked samples go back to the caller

    // solve(Ar, -br) (:767): guarded pivot-free Gauss-Jordan, two row tiles, panels of four columns; two values of dq and q per lane.
    // BG_OPT_FORCE_PIVOTED (tests): every sample is handed back to the caller after its first solve.
    template <bool GAL, bool PIV, int W, class Lap>
    static __device__ __forceinline__ void solve_update(const StreamRunArgs& a, const StreamLds& L, int r, int lane, bool& aborted, int&,
                                                        double& nd, double& nq, const Lap& solved)
    {
        const double* S = L.slab;
        const double wtu0 = (lane < r) ? S[lane * WPS + WR + 1] : 0.0;                     // Phi^T u, rows 0 .. 63
        const double wtu1 = (64 + lane < r) ? S[(64 + lane) * WPS + WR + 1] : 0.0;         // rows 64 .. 95
        wide_solve<GAL>((lds_double_t*)S, (lds_double_t*)L.m, (lds_double_t*)L.diag, (lds_double_t*)L.y, (lds_int_t*)L.bad, W, lane, r);
        solved();
        const bool tripped = ((L.bad[0] | L.bad[1] | L.bad[2] | L.bad[3]) != 0) || a.force_pivoted;   // workgroup-uniform
        if (tripped) aborted = true;
        const double dq0 = (lane < r) ? L.y[lane] * rcp(L.diag[lane]) : 0.0;
        const double dq1 = (64 + lane < r) ? L.y[64 + lane] * rcp(L.diag[64 + lane]) : 0.0;
        const double q0 = wtu0 + dq0, q1 = wtu1 + dq1;
        wave_sum2(dq0 * dq0 + dq1 * dq1, q0 * q0 + q1 * q1, nd, nq);
        if (W == 0) {
            L.q[lane] = q0;
            if (lane < WR - 64) L.q[64 + lane] = q1;
        }
    }
};

}  // namespace bg
