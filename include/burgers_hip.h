/* burgers_hip.h -- C ABI of libburgers_hip.so (MI355X / gfx950).
 *
 * The reference (SADPR/1D-Burgers-Equation-ROMs) is pure Python on this path and
 * has no FFI of its own; each entry point below names the reference routine whose
 * inner loop it replaces (file:line relative to the reference checkout).  The
 * reference-side binding (a ctypes stub inside FEM/fem_burgers.py) is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch.Tensor.data_ptr()) unless
 *     it is marked "host";
 *   - all calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL =
 *     the null stream), allocate nothing, keep no global state and are thread-safe;
 *   - return value: BG_OK (0) or a negative BG_ERR_* code; nothing throws;
 *   - arrays are dense, row-major, float64 unless stated; "history" arrays are
 *     time-major per sample, hist[b][t][i] (the reference's (N, nT+1) C-order layout
 *     is produced by bg_transpose_batched);
 *   - one wavefront owns one (mu1, mu2) sample for the whole time loop.
 */
#ifndef BURGERS_HIP_H
#define BURGERS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BG_ABI_VERSION 1

enum {
    BG_OK = 0,
    BG_ERR_BAD_ARG = -1,        /* null pointer, negative size, ...                       */
    BG_ERR_UNSUPPORTED_N = -2,  /* N outside the range the wave-per-sample kernels cover  */
    BG_ERR_NONUNIFORM = -3,     /* mesh is not uniform (fast path only handles linspace)  */
    BG_ERR_LAUNCH = -4,         /* hipLaunchKernel failed; see bg_last_hip_error()        */
    BG_ERR_UNSUPPORTED_R = -5,  /* reduced dimension outside the supported range          */
    BG_ERR_PROJECTION = -6,     /* unknown projection enum                                */
    BG_ERR_WORKSPACE = -7       /* caller-provided workspace too small                    */
};

enum { BG_PROJ_GALERKIN = 0, BG_PROJ_LSPG = 1 };

/* option bits of the `supg` / `options` argument of the assembly-carrying entry points */
enum { BG_OPT_SUPG = 1,        /* include the SUPG vector (fom_burgers, pod_prom_burgers, pod_ann_prom) */
       BG_OPT_NONUNIFORM = 2,  /* x is not a linspace: use the per-element-length kernels          */
       BG_OPT_W_COLMAJOR = 4,  /* bg_rom_reduce*: W is [r][N] (per sample), not [N][r]             */
       BG_OPT_MFMA_16X16 = 8,  /* bg_rom_reduce*: use the v_mfma_f64_16x16x4 kernel for every r (A/B timing, tests) */
       BG_OPT_FORCE_PIVOTED = 16, /* bg_rom_run: take the partial-pivoting branch of the reduced solve every time (tests) */
       BG_OPT_NO_TANGENT_REUSE = 32, /* bg_ann_rom_run: evaluate the closure at every step start even when its float32 input is unchanged (tests) */
       BG_OPT_FOM_WIDE = 64,   /* bg_fom_run: one WORKGROUP per sample also for 64 < N <= 1536 (uniform mesh); measured slower than the default there */
       BG_OPT_FOM_WAVE = 128,  /* bg_fom_run: one WAVEFRONT per sample (the default for N <= 1536; overrides BG_OPT_FOM_WIDE) */
       BG_OPT_PIVOT_ON_DEVICE = 256 /* bg_hyper_rom_run_wide: a repair kernel redoes the samples that need row exchanges, nothing is handed back */ };

/* bg_rom_run: transient value of info[b] between its two kernels (never seen by the caller);
 * bg_rom_run_wide: info[b] of a sample the caller must redo with a pivoting solve */
#define BG_INFO_NEEDS_PIVOTING (-1)

/* per-sample status bits written to `flags` */
enum { BG_FLAG_HIT_CAP = 1, BG_FLAG_NONFINITE = 2 };

#define BG_COUNTER_SLOTS 16   /* partial counters of bg_lu_solve_update ...          */
#define BG_COUNTER_STRIDE 32  /* ... one per 128-byte line (stride in int32 elements) */

/* activation kinds of bg_mlp_act_jvp */
enum { BG_ACT_NONE = 0, BG_ACT_ELU = 1, BG_ACT_RELU = 2, BG_ACT_TANH = 3 };

/* kernels of bg_rbf_eval */
enum { BG_RBF_GAUSSIAN = 0, BG_RBF_IMQ = 1 };

int bg_abi_version(void);
const char *bg_strerror(int code);
/* hipError_t of the most recent failed launch on the calling thread (0 if none). */
int bg_last_hip_error(void);

/* Largest N of bg_fom_run / bg_fom_assemble / bg_tridiag_solve: 8192.  N <= 1536 runs one wavefront per
 * sample (rows per lane <= 24), 1536 < N <= 8192 one 256-thread workgroup per sample (rows per thread <= 32);
 * at 24 rows per lane and 32 per thread part of the state spills to AGPRs / scratch.  bg_fd_run switches to
 * the workgroup form above N = 2048 (same limit, 8192). */
int bg_fom_max_n(void);

/* ---------------------------------------------------------------------------------
 * bg_fom_run -- batched replacement of FEMBurgers.fom_burgers
 *   reference: FEM/fem_burgers.py:646-707 (time loop + Picard loop), with
 *   compute_convection_matrix :389-425, compute_forcing_vector :427-461,
 *   compute_supg_term :500-581 and scipy spsolve :692 fused into one kernel.
 *
 *   x      [N]               mesh nodes, strictly increasing; pass BG_OPT_NONUNIFORM in `supg` when
 *                            they are not a linspace (the host knows: X is host data in the reference)
 *   u0     [B][N]            initial state per sample
 *   mu1,mu2[B]               Dirichlet value u(0,t) and source exponent per sample
 *   hist   [B][nsteps+1][N]  hist[b][0] = u0[b]; hist[b][t+1] = state after step t
 *   iters  [B][nsteps]       Picard iterations taken per step (the reference's k)
 *   flags  [B]               BG_FLAG_* bits
 *   tol, max_it              the reference hard-codes 1e-6 and 20 (:663).  A step iterates while error > tol and k < max_it,
 *                            after a first iteration that always runs: tol = 0 and tol < 0 run every step to max_it, tol = inf
 *                            and tol = NaN (no comparison holds) give one iteration per step, flagged only where max_it = 1.
 *   supg                     option bits: BG_OPT_SUPG (fom_burgers has it) | BG_OPT_NONUNIFORM
 *
 *   The iteration: a time step starts with iterations that solve A(u) v = b for the new iterate v itself (du = v - u
 *   serves the stopping norm ||du|| / ||v|| only) and stays with them while the stopping test is missed by more than a
 *   factor of 16; from there on an iteration solves A(u) du = b - A(u) u for the increment, as the reference does, so
 *   that the state a step ends on is corrected below the accuracy of the pivot-free solve.  Counts are the reference's k.
 *   Where a thread's registers do not hold both loop bodies (N > 6144; a non-uniform mesh of 1024 < N <= 1536 or
 *   N > 4096) every iteration solves for the increment.
 *
 *   Range of the state: the SUPG quotients t_e / max(|u_e + u_{e+1}|, 2e-10) of four neighbouring elements share
 *   one reciprocal of the product of their denominators, which must stay below 1.8e308: every |u| <~ 5e76 is safe
 *   (the product cannot underflow).  Beyond that the reciprocal is 0 and its Newton step NaN: the sample turns
 *   non-finite, BG_FLAG_NONFINITE is set and its Picard loops end as for any NaN state; it is never silently wrong.
 *   bg_fom_run_traced and bg_fom_assemble share the assembly and the limit.
 * --------------------------------------------------------------------------------- */
int bg_fom_run(int N, int B, int nsteps, const double *x, const double *u0, const double *mu1,
               const double *mu2, double dt, double E, double tol, int max_it, int supg,
               double *hist, int32_t *iters, int32_t *flags, void *stream);

/* bg_fom_run_traced -- bg_fom_run that also stores the error of every Picard iteration, the value the reference prints
 *   per iteration (`print(f"Iteration: {k}, Error: {error_U}")`, FEM/fem_burgers.py:664; error_U = ||dU|| / ||U1|| of :698).
 *   errs [B][nsteps][max_it]: errs[b][t][k] = error after iteration k of step t (entries k >= iters[b][t] untouched).
 *   Same results as bg_fom_run; a separate kernel instantiation, N <= 1536 (BG_ERR_UNSUPPORTED_N beyond). */
int bg_fom_run_traced(int N, int B, int nsteps, const double *x, const double *u0, const double *mu1,
                      const double *mu2, double dt, double E, double tol, int max_it, int supg,
                      double *hist, int32_t *iters, int32_t *flags, double *errs, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_fom_assemble -- one Picard assembly, for inspection and tests
 *   reference: FEM/fem_burgers.py:666-689 (C, S, F, A with Dirichlet row, b, R).
 *   uk, un [B][N]; outputs lo/di/up/rhs [B][N]: the three diagonals of A(u_k)
 *   (lo[.][0] = up[.][N-1] = 0) and rhs = b - A u_k = -R.
 * --------------------------------------------------------------------------------- */
int bg_fom_assemble(int N, int B, const double *x, const double *uk, const double *un,
                    const double *mu1, const double *mu2, double dt, double E, int supg,
                    double *lo, double *di, double *up, double *rhs, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_tridiag_solve -- batched pivot-free tridiagonal solve, one wavefront per system
 *   reference: scipy.sparse.linalg.spsolve call at FEM/fem_burgers.py:692.
 *   lo/di/up/rhs [B][N] as produced by bg_fom_assemble; sol [B][N].
 * --------------------------------------------------------------------------------- */
int bg_tridiag_solve(int N, int B, const double *lo, const double *di, const double *up,
                     const double *rhs, double *sol, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_transpose_batched -- out[b][c][r] = in[b][r][c]
 *   turns the time-major history [B][nT+1][N] into the reference's (N, nT+1) C-order
 *   snapshot layout per sample (FEM/fem_burgers.py:650, np.save at
 *   FEM/paper_training_stage.py:52-53).
 * --------------------------------------------------------------------------------- */
int bg_transpose_batched(int B, int rows, int cols, const double *in, double *out, void *stream);

/* =================================================================================
 * Projection ROMs: one batched Picard / Gauss-Newton iteration is
 *     bg_rom_reduce  ->  bg_lu_solve  ->  (family-specific update, host side GEMMs)
 * ================================================================================= */

/* Largest N / r the register-resident MFMA reduce kernel covers (N <= 512, r <= 47). */
int bg_rom_max_n(void);
int bg_rom_max_r(void);

/* bg_forcing_setup -- per-sample load constants, once per run
 *   reference: compute_forcing_vector FEM/fem_burgers.py:427-461 (the reference recomputes
 *   it every iteration, :673) and the f_gp terms of compute_supg_term :556-558.
 *   fdt[b][i] = dt * F_i(mu2_b);  hfs[b][e] = h_e * (f(gp1) + f(gp2)), hfs[b][N-1] = 0. */
int bg_forcing_setup(int N, int B, const double *x, const double *mu2, double dt, int options,
                     double *fdt, double *hfs, void *stream);

/* bg_mass_rhs -- g[b] = M u^n[b] + dt F[b], once per time step
 *   reference: `M @ U[:, n] + At*F` at FEM/fem_burgers.py:683 / :746 / :1141 / :1214. */
int bg_mass_rhs(int N, int B, const double *x, const double *un, const double *fdt, int options,
                double *g, void *stream);

/* bg_rom_reduce -- fused assembly + projection of one iteration, fp64 MFMA
 *   reference: FEM/fem_burgers.py:730-762 (pod_prom_burgers), :1134-1156
 *   (pod_quadratic_manifold, supg = 0), :1203-1233 (pod_ann_prom).
 *   W        basis or tangent, [N][r] row-major shared by all samples (w_stride = 0) or
 *            [B][N][r] with w_stride = N*r elements; with BG_OPT_W_COLMAJOR in `supg` each
 *            sample's block is [r][N] instead (what one GEMM dN^T [B*r x m] . U_s^T [m x N] yields)
 *   U        [B][N] current iterate u_k;  G from bg_mass_rhs;  hfs from bg_forcing_setup
 *   active   [B] int32 or NULL: samples with 0 are skipped and their outputs left untouched
 *   Ar       [B][r][r]: W^T A W (BG_PROJ_GALERKIN) or (A W)^T (A W) (BG_PROJ_LSPG)
 *   br       [B][r]:    W^T R   or (A W)^T R,  R = A u_k - b
 *   wtu      [B][r] or NULL: W^T u_k (the `Phi.T @ U0` of :770)
 *   One kernel over two MFMA shapes: v_mfma_f64_4x4x4_4b (r <= 40) and v_mfma_f64_16x16x4 (r <= 47); staging,
 *   assembly, write-out and the order of every sum are shared.  BG_OPT_MFMA_16X16 in `supg` selects the second
 *   shape for every r, for A/B timing and tests (no environment is read). */
int bg_rom_reduce(int N, int B, int r, int projection, const double *x, const double *W,
                  long long w_stride, const double *U, const double *G, const double *hfs,
                  const double *mu1, double dt, double E, int supg, const int32_t *active,
                  double *Ar, double *br, double *wtu, void *stream);

/* bg_rom_reduce_indexed -- bg_rom_reduce with a small set of bases shared among the samples: sample b
 * uses the block W + w_index[b] * w_stride (local POD: the basis of its cluster; reference
 * local_prom_burgers, FEM/fem_burgers.py:1011-1013).  A workgroup keeps the fragments in registers
 * while consecutive samples of its stride use the same block. */
int bg_rom_reduce_indexed(int N, int B, int r, int projection, const double *x, const double *W,
                          long long w_stride, const int32_t *w_index, const double *U, const double *G,
                          const double *hfs, const double *mu1, double dt, double E, int supg,
                          const int32_t *active, double *Ar, double *br, double *wtu, void *stream);

/* bg_lu_solve -- x[b] = solve(A[b], sign * rhs[b]), partial pivoting, n <= 64
 *   reference: np.linalg.solve(Ar, -br) at FEM/fem_burgers.py:767 / :1161 / :1237
 *   (LAPACK gesv).  info[b] = 0, or k+1 when the pivot of step k is exactly zero (the first such step;
 *   numpy raises LinAlgError("Singular matrix") there).  info (may be NULL) is only ever written with a non-zero
 *   value: the caller zeroes it, and a system that is healthy or skipped leaves its entry as it was.  The same
 *   holds for the info of bg_lu_solve_update, which so keeps a singular system's mark across iterations. */
int bg_lu_solve(int n, int B, const double *A, const double *rhs, double sign, const int32_t *active,
                double *x, int32_t *info, void *stream);

/* bg_rom_reduce_lifted -- bg_rom_reduce for a shared basis Phi with the lift fused in:
 *   u_k = Phi q is formed from the register-resident basis, stored to U[b] and used for the
 *   assembly, so the state never round-trips through a GEMM.  reference: `U1 = Phi @ q` :773. */
int bg_rom_reduce_lifted(int N, int B, int r, int projection, const double *x, const double *Phi,
                         const double *q, double *U, const double *G, const double *hfs,
                         const double *mu1, double dt, double E, int supg, const int32_t *active,
                         double *Ar, double *br, double *wtu, void *stream);

/* bg_rom_lift -- U[b] = Phi q[b] only (end of a time step). */
int bg_rom_lift(int N, int B, int r, const double *x, const double *Phi, const double *q,
                const int32_t *active, double *U, void *stream);

/* bg_lu_solve_update -- bg_lu_solve(A, -rhs) fused with the reduced-coordinate update and the
 * convergence bookkeeping of one batched iteration.  Samples with active[b] == 0 are skipped.
 *   mode 1 (pod_prom_burgers :770-776):       q = wtu + dq;  err = |dq|/|q|;            go on while err > tol and k < max_it
 *   mode 2 (pod_quadratic_manifold :1161-69): q += dq;       err = |dq|/max(1e-14,|q|); stop when err < tol (cap max_it)
 *   mode 3 (pod_ann_prom :1237-1244):         q += dq;       err = |dq|/(|q|+1e-14);    go on while err > tol and k < max_it
 *   iters[b] += 1; active[b] <- go on; flags[b] |= BG_FLAG_*.
 *   counter [2][BG_COUNTER_SLOTS][BG_COUNTER_STRIDE] int32, element [.][s][0] used: row 0 sums to the
 *   number of samples still active, row 1 to the number of singular systems (sample b adds to slot
 *   b % SLOTS, one cache line per slot: 4096 atomics on one line cost 8 us); the caller zeroes it
 *   before the call and sums the slots. */
int bg_lu_solve_update(int n, int B, const double *A, const double *rhs, int mode, const double *wtu,
                       double *q, double *dq, double tol, int max_it, int32_t *active, int32_t *iters,
                       int32_t *flags, int32_t *counter, int32_t *info, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_rom_run -- batched replacement of FEMBurgers.pod_prom_burgers, the WHOLE time loop on the device
 *   reference: FEM/fem_burgers.py:709-785.  One workgroup owns one sample for all time steps and Picard iterations:
 *   assembly, fp64-MFMA projection (as bg_rom_reduce), the r x r solve, q = Phi^T u + dq, the stopping test
 *   err = |dq|/|q| > tol and k < max_it (:729, :776) and the lift u = Phi q run with no kernel boundary and no host
 *   in between; HBM sees u0 once and one N-row history write per time step.
 *   Phi    [N][r] row-major (the reference's U_modes .npy layout), shared by all samples; N <= 512, r <= 40
 *          (bg_rom_run_max_r) -- beyond that use bg_rom_reduce + bg_lu_solve_update (BG_ERR_UNSUPPORTED_R / _N)
 *   u0, mu1, mu2, hist, iters, flags: as bg_fom_run (hist[b][0] = u0[b]; flags BG_FLAG_*)
 *   tol, max_it   the stopping controls of EVERY device-side time loop of this header (bg_rom_run*, bg_hyper_*rom_run*,
 *          bg_quad_rom_run*, bg_ann_rom_run*, bg_rbf_rom_run*, bg_local_rom_run*); max_it >= 1.  As in bg_fom_run the first
 *          iteration of a step always runs, and there are two rules, those of bg_lu_solve_update:
 *            Picard and closure loops (modes 1 and 3): go on while err > tol and k < max_it; BG_FLAG_HIT_CAP whenever a
 *              step ends with k >= max_it, a step that converged in exactly max_it iterations included;
 *            quadratic-manifold loops (mode 2): stop once err < tol or k >= max_it; BG_FLAG_HIT_CAP only where the step
 *              at the cap did not converge ("Newton did not converge", :1171).
 *          tol = 0 and tol < 0: no step converges, every count is max_it and every sample is flagged, under both rules.
 *          tol = inf: one iteration per step; no flag unless max_it = 1 (quadratic: never).  The references' ``while``
 *          loops run no iteration at tol = inf; one iteration per step is what they give at max_it = 1.  The flag is
 *          sticky over the steps of a sample and is that sample's alone: a persistent workgroup starts every sample it
 *          takes with flags, info and the iteration counter cleared.  (tests/test_rom_controls_gpu.py)
 *   info   [B] (required): 0, or k+1 when the reduced matrix of a sample is exactly singular at elimination step k
 *          (np.linalg.solve raises LinAlgError there); that sample stops and its remaining history is undefined
 *   options BG_OPT_SUPG (pod_prom_burgers has it) | BG_OPT_NONUNIFORM | BG_OPT_FORCE_PIVOTED
 *   The reduced solve is np.linalg.solve's partial-pivoting elimination: as long as every multiplier stays <= 1 in
 *   modulus the pivot is the diagonal and no search is made (first kernel).  A sample in which a multiplier exceeds 1
 *   is marked in info and redone from u0 by a second kernel of the same call with the pivot search of bg_lu_solve;
 *   that kernel returns at once when nothing is marked.  BG_OPT_FORCE_PIVOTED sends every sample through it.
 *   order  NULL, or [B] int32 on the device: a permutation of 0 .. B-1 -- slot i of the launch works on sample order[i]
 *          (a scheduling hint, results are the same bit for bit: the samples are independent).  The workgroups are
 *          persistent, workgroup k of G takes the slots k, k + G, ... (G = min(B, 2 CUs); bg_rom_run_wide and
 *          bg_ann_rom_run alike with G = min(B, CUs) / min(B, 2 CUs)); in bg_quad_rom_run the slots 4 g .. 4 g + 3 share
 *          a workgroup AND its passes (every pass lasts until the slowest of the four has converged).  Iteration counts
 *          follow mu1 (correlation 0.99 on the bench sweep), so a caller that sorts the samples by mu1 and deals them out
 *          evenly (burgers_hip/rom.py::sample_order) removes the imbalance; measured at the bench sizes
 *          (tools/time_balance.py): quadratic + 2.5 %, POD-ANN + 1.8 %, r = 96 + 2.9 %, r = 40 + 0.5 %.  The reference-side
 *          binding passes NULL.
 * --------------------------------------------------------------------------------- */
int bg_rom_run_max_r(void);
int bg_rom_run(int N, int B, int r, int nsteps, int projection, const double *x, const double *Phi,
               const double *u0, const double *mu1, const double *mu2, double dt, double E, double tol,
               int max_it, int options, double *hist, int32_t *iters, int32_t *flags, int32_t *info,
               const int32_t *order, void *stream);

/* bg_rom_run_wide -- bg_rom_run for the thesis' larger bases, 40 < r <= 96 (bg_rom_run_wide_max_r), N <= 512
 *   reference: FEM/fem_burgers.py:709-785 with POD/modes/U_modes_tol_1e-04.npy (r = 96), POD/Results_thesis/prom_pod.py:35-58.
 *   Same arguments, outputs and semantics as bg_rom_run except:
 *   PhiP   [NPAD + 2][96], NPAD = N rounded up to 64 (bg_rom_run_wide_phi_elems(N) doubles, 16-byte aligned): Phi row i at
 *          row index i + 1, zero rows around and beyond the mesh, zero columns beyond r -- built once per basis by the caller;
 *   info   0, k + 1 for an exactly singular reduced system, or BG_INFO_NEEDS_PIVOTING for a sample whose pivot-free
 *          elimination met a multiplier above 1: the caller redoes that sample with a pivoting solve (there is no second
 *          kernel here; burgers_hip/rom.py sends it through the library path);
 *   order  [B] or NULL; entries outside [0, B) are skipped.
 *   The basis streams through LDS 64 mesh rows at a time, the accumulators of the reduced system are dealt to the four
 *   waves (csrc/rom_wide.hip).  options: BG_OPT_SUPG | BG_OPT_NONUNIFORM | BG_OPT_FORCE_PIVOTED (tests: every sample is
 *   handed back as if its elimination had needed a row exchange). */
int bg_rom_run_wide_max_r(void);
long long bg_rom_run_wide_phi_elems(int N);
int bg_rom_run_wide(int N, int B, int r, int nsteps, int projection, const double *x, const double *PhiP,
                    const double *u0, const double *mu1, const double *mu2, double dt, double E, double tol,
                    int max_it, int options, double *hist, int32_t *iters, int32_t *flags, int32_t *info,
                    const int32_t *order, void *stream);

/* bg_rom_run_blocked -- bg_rom_run_wide for the thesis' finest bases, r <= 256 (bg_rom_run_blocked_max_r), N <= 512
 *   reference: FEM/fem_burgers.py:709-785 with POD/modes/U_modes_tol_1e-05.npy (r = 160) and _1e-06.npy (r = 227).
 *   Opt-in: the facade routes r > bg_rom_run_wide_max_r() here only when asked (burgers_hip/rom.py, blocked=True).
 *   Same arguments, outputs and semantics as bg_rom_run_wide except:
 *   PhiP   [NPAD + 2][RP], NPAD = N rounded up to 8, RP = r rounded up to 16 (bg_rom_run_blocked_phi_elems(N, r) doubles):
 *          Phi row i at row index i + 1, zero rows around and beyond the mesh, zero columns beyond r;
 *   work   `slots` slots of bg_rom_run_blocked_work_elems(N, r) doubles, one per workgroup (contents need no
 *          initialisation and are garbage afterwards).  A slot holds the padded reduced system [RP][RP + 16]: Ar, then
 *          -br and 15 zero columns; the blocked elimination runs in place there.  Workgroup k of G = min(B, slots)
 *          takes the slots k, k + G, ... of `order` and only ever touches slot k of `work`.
 *   order  [B] or NULL; entries outside [0, B) are skipped.
 *   info   0; k + 1 when the pivot of column k is exactly zero together with the rest of its column (LAPACK's info);
 *          BG_INFO_NEEDS_PIVOTING for a sample whose pivot-free elimination met a multiplier above 1 below the diagonal
 *          (np.linalg.solve would have exchanged rows): the caller redoes it with a pivoting solve.
 *   Errors: N < 3, r < 1, B or nsteps < 0, max_it < 1, dt <= 0 or a null operand with B > 0: BG_ERR_BAD_ARG;
 *   N > 512: BG_ERR_UNSUPPORTED_N; r > 256: BG_ERR_UNSUPPORTED_R; work NULL or slots < 1 with B > 0: BG_ERR_WORKSPACE;
 *   an unknown projection: BG_ERR_PROJECTION; B = 0: BG_OK with nothing launched.
 *   One workgroup of four waves per slot, 16x16x4 fp64 matrix instructions for the projection and the elimination
 *   (csrc/rom_blocked.hip).  options: BG_OPT_SUPG | BG_OPT_NONUNIFORM | BG_OPT_FORCE_PIVOTED (every sample handed back). */
int bg_rom_run_blocked_max_r(void);
long long bg_rom_run_blocked_phi_elems(int N, int r);
long long bg_rom_run_blocked_work_elems(int N, int r);
int bg_rom_run_blocked(int N, int B, int r, int nsteps, int projection, const double *x, const double *PhiP,
                       const double *u0, const double *mu1, const double *mu2, double dt, double E, double tol,
                       int max_it, int options, double *work, int slots, double *hist, int32_t *iters,
                       int32_t *flags, int32_t *info, const int32_t *order, void *stream);

/* bg_rom_run_long -- bg_rom_run for long meshes: 3 <= N <= 1024 (bg_rom_run_long_max_n; meant for N > 512, where bg_rom_run
 *   ends), r <= 40 (bg_rom_run_long_max_r).  reference: FEM/fem_burgers.py:709-785.
 *   Opt-in: the facade routes N > 512 here only when asked (burgers_hip/rom.py, long_mesh=True).
 *   Same arguments, outputs and semantics as bg_rom_run except:
 *   PhiP   [NPAD + 2][40], NPAD = N rounded up to 64 (bg_rom_run_long_phi_elems(N, r) doubles, 16-byte aligned; 0 for an
 *          N or r the kernel does not cover): Phi row i at row index i + 1, zero rows around and beyond the mesh, zero
 *          columns beyond r -- built once per basis by the caller;
 *   order  [B] or NULL; entries outside [0, B) are skipped.
 *   info   0, or k + 1 when the reduced matrix of a sample is exactly singular at elimination step k.  Pivoting is repaired
 *          inside the call as in bg_rom_run: a sample whose pivot-free elimination meets a multiplier above 1 below the
 *          diagonal or a zero pivot is marked BG_INFO_NEEDS_PIVOTING by the first kernel and redone from u0 by a second
 *          kernel of the same call with the pivot search of bg_lu_solve, so the caller never sees that value.
 *   Errors: N < 3, r < 1, B or nsteps < 0, max_it < 1, dt <= 0, a null operand or output with B > 0, PhiP not 16-byte
 *   aligned: BG_ERR_BAD_ARG; N > 1024: BG_ERR_UNSUPPORTED_N; r > 40: BG_ERR_UNSUPPORTED_R; an unknown projection:
 *   BG_ERR_PROJECTION; B = 0: BG_OK with nothing launched.
 *   The basis streams through LDS 64 mesh rows at a time, the accumulators of the reduced system are dealt to the four
 *   waves (csrc/rom_long.hip); workgroup k of G = min(B, bg_rom_run_long_workgroups_per_cu() CUs) takes the slots k, k + G, ...
 *   options: BG_OPT_SUPG | BG_OPT_NONUNIFORM | BG_OPT_FORCE_PIVOTED (tests: every sample through the second kernel). */
int bg_rom_run_long_max_n(void);
int bg_rom_run_long_max_r(void);
int bg_rom_run_long_workgroups_per_cu(void);
long long bg_rom_run_long_phi_elems(int N, int r);
int bg_rom_run_long(int N, int B, int r, int nsteps, int projection, const double *x, const double *PhiP,
                    const double *u0, const double *mu1, const double *mu2, double dt, double E, double tol,
                    int max_it, int options, double *hist, int32_t *iters, int32_t *flags, int32_t *info,
                    const int32_t *order, void *stream);

/* bg_hyper_rom_run -- the POD PROM time loop HYPER-REDUCED: the reduced system is assembled from m sampled mesh rows with
 *   weights xi >= 0 (ECSW-style), Ar = sum_j xi_j w_j^T y_j and br = sum_j xi_j w_j^T R_j over the rows i_j = rows[j] only,
 *   y_j = (A Phi)[i_j], R_j = (A u - b)[i_j], w_j = Phi[i_j] (Galerkin) or y_j (LSPG).  3 <= N <= bg_fom_max_n(): the kernel
 *   never touches a vector of mesh length; r <= 40, m <= 256 (bg_hyper_rom_limits).  reference: FEM/fem_burgers.py:709-785
 *   with the sums over mesh rows restricted and weighted; with all rows and unit weights the loop is the reference's.
 *   Opt-in: nothing routes here unless asked (burgers_hip/rom.py, pod_prom_run_hyper; the facade's hyper=).
 *   rows   [m] int32, ascending, distinct, in [0, N) (the caller's duty: they live on the device and are not checked here);
 *   xi     [m] finite, >= 0 (likewise);
 *   xs     [m][3] the coordinates x[i-1], x[i], x[i+1] of every sampled row; slots outside the mesh are ignored.  Without
 *          BG_OPT_NONUNIFORM the spacing is (last stencil node - first stencil node) / (their index distance), which is
 *          (x[N-1] - x[0]) / (N - 1) when rows 0 and N - 1 are sampled;
 *   PhiS   [MPAD][3][42], MPAD = m rounded up to 32 (bg_hyper_rom_table_elems(m, r) doubles, 16-byte aligned; 0 for an m or r
 *          the kernel does not cover): rows Phi[i-1], Phi[i], Phi[i+1] of sampled row j at row indices 3 j .. 3 j + 2, zero
 *          rows outside the mesh and beyond m, zero columns beyond r -- built once per basis and sampling by the caller;
 *   q0     [B][r] = Phi^T u0;   u0s  [B][m][3] u0 at the stencil nodes (slots outside the mesh ignored);
 *   qhist  [B][nsteps+1][r] the reduced coordinates, row 0 = q0; the caller decodes U = Phi q;
 *   iters, flags, info, order, options: as bg_rom_run_long (pivoting repaired inside the call, so the caller never sees
 *          BG_INFO_NEEDS_PIVOTING; entries of order outside [0, B) are skipped).
 *   Row 0 is the Dirichlet row, row N - 1 has no right element.  The state at the stencil is PhiS q, except in the first
 *   iteration of the run, which assembles at u0s itself and takes u^n = u0s (the reference starts from u0, not from
 *   Phi Phi^T u0).  The update is q <- q + dq: equal to the reference's Phi^T u_k + dq for an orthonormal Phi, as
 *   u_k = Phi q; the stopping rule is |dq| / |q| > tol and k < max_it.
 *   Errors: N < 3, r < 1, m < 1, B or nsteps < 0, max_it < 1, dt <= 0, m > N, a null operand or output with B > 0, PhiS not
 *   16-byte aligned: BG_ERR_BAD_ARG; N > bg_fom_max_n(): BG_ERR_UNSUPPORTED_N; r > 40 or m > 256 (like the row and centre
 *   counts of the local loops): BG_ERR_UNSUPPORTED_R; an unknown projection: BG_ERR_PROJECTION; B = 0: BG_OK with nothing
 *   launched.  Sizes the kernel does not cover are refused, never rerouted.
 *   The table streams through LDS 32 sampled rows at a time, the accumulators of the reduced system are dealt to the four
 *   waves (csrc/rom_hyper.hip); workgroup k of G = min(B, 2 CUs) takes the slots k, k + G, ... */
int bg_hyper_rom_limits(int *max_r, int *max_m);
long long bg_hyper_rom_table_elems(int m, int r);
int bg_hyper_rom_run(int N, int B, int r, int m, int nsteps, int projection, const int32_t *rows, const double *xi,
                     const double *xs, const double *PhiS, const double *q0, const double *u0s, const double *mu1,
                     const double *mu2, double dt, double E, double tol, int max_it, int options, double *qhist,
                     int32_t *iters, int32_t *flags, int32_t *info, const int32_t *order, void *stream);

/* bg_hyper_rom_run_wide -- bg_hyper_rom_run for the larger bases: r <= 96 (meant for r > 40, where bg_hyper_rom_run ends),
 *   m <= 512 (bg_hyper_rom_wide_limits), 3 <= N <= bg_fom_max_n().  reference: FEM/fem_burgers.py:709-785 with the sums
 *   over mesh rows restricted and weighted.  Opt-in: burgers_hip/rom.py, pod_prom_run_hyper_wide; pod_prom_run_hyper and the
 *   facade's hyper= send bases of 41 .. 96 modes here.
 *   Arguments, semantics and return codes are bg_hyper_rom_run's, with these differences:
 *   PhiS   [MPAD][3][98], MPAD = m rounded up to 16 (bg_hyper_rom_wide_table_elems(m, r) doubles, 16-byte aligned; 0 for an m
 *          or r the kernel does not cover), otherwise laid out like bg_hyper_rom_run's table;
 *   info   the solve is bg_rom_run_wide's guarded pivot-free 96 x 96 elimination and there is no repair kernel: a sample whose
 *          elimination meets a multiplier above 1 or a zero pivot is marked BG_INFO_NEEDS_PIVOTING, its qhist and iters are
 *          then undefined, and the caller redoes it (rom.py: the weighted-row library iteration).  BG_OPT_FORCE_PIVOTED
 *          (tests) marks every sample after its first solve;
 *          with BG_OPT_PIVOT_ON_DEVICE in `options` a second kernel follows the first on the same stream, as in bg_hyper_rom_run:
 *          it redoes every marked sample from u0 with a 96 x 96 solve with partial pivoting in every iteration (the largest
 *          entry among the rows not yet used, the lowest row on ties: LAPACK's pivots; the same routine as
 *          bg_wide_solve_pivoted) and leaves info = 0, or k + 1 where column k of a reduced system had no non-zero
 *          candidate (exactly singular; the sample stops there, its later qhist and iters are undefined).  No sample comes
 *          back marked.  BG_OPT_FORCE_PIVOTED then sends every sample through the second kernel alone;
 *   Errors: r > 96 or m > 512: BG_ERR_UNSUPPORTED_R; m > N or PhiS not 16-byte aligned: BG_ERR_BAD_ARG; the rest as
 *          bg_hyper_rom_run.
 *   The table streams through LDS 16 sampled rows at a time (two buffers of 37 632 B, over which the 96 x 98 system is parked);
 *   one workgroup per compute unit (csrc/rom_hyper_wide.hip); workgroup k of G = min(B, CUs) takes the slots k, k + G, ... */
int bg_hyper_rom_wide_limits(int *max_r, int *max_m);
long long bg_hyper_rom_wide_table_elems(int m, int r);
int bg_hyper_rom_run_wide(int N, int B, int r, int m, int nsteps, int projection, const int32_t *rows, const double *xi,
                          const double *xs, const double *PhiS, const double *q0, const double *u0s, const double *mu1,
                          const double *mu2, double dt, double E, double tol, int max_it, int options, double *qhist,
                          int32_t *iters, int32_t *flags, int32_t *info, const int32_t *order, void *stream);

/* bg_hyper_rom_run_blocked -- bg_hyper_rom_run for the thesis' finest bases: r <= 256 (meant for r > 96, where
 *   bg_hyper_rom_run_wide ends), m <= 1024 (bg_hyper_rom_blocked_limits), 3 <= N <= bg_fom_max_n().  reference:
 *   FEM/fem_burgers.py:709-785 with the sums over mesh rows restricted and weighted; with all rows and unit weights the loop is
 *   the reference's, so it is also the exact device-side route of these bases on meshes of up to 1024 nodes.
 *   Opt-in: burgers_hip/rom.py, pod_prom_run_hyper_blocked; the facade's hyper= with blocked=True.
 *   rows, xi, xs, q0, u0s, qhist, iters, flags, order: as bg_hyper_rom_run.  The differences:
 *   PhiS   [MPAD][3][RP], MPAD = m rounded up to 8, RP = r rounded up to 16 (bg_hyper_rom_blocked_table_elems(m, r) doubles,
 *          16-byte aligned; 0 for an m or r the kernel does not cover): rows Phi[i-1], Phi[i], Phi[i+1] of sampled row j at row
 *          indices 3 j .. 3 j + 2, zero rows outside the mesh and beyond m, zero columns beyond r;
 *   work   `slots` slots of bg_hyper_rom_blocked_work_elems(r) = RP (RP + 16) doubles, one per workgroup, as bg_rom_run_blocked's
 *          (no initialisation needed, garbage afterwards): the padded system Ar | -br, eliminated in place.  Workgroup k of
 *          G = min(B, slots) takes the slots k, k + G, ... of `order` and only ever touches slot k of `work`;
 *   info   0; k + 1 when the pivot of column k is exactly zero together with the rest of its column (LAPACK's info; the sample
 *          stops there); BG_INFO_NEEDS_PIVOTING for a sample whose guarded pivot-free elimination met a multiplier above 1 below
 *          the diagonal: its qhist and iters are then undefined and the caller redoes it (rom.py: the weighted-row library
 *          iteration).  BG_OPT_FORCE_PIVOTED (tests) marks every sample after its first solve.  There is no repair kernel:
 *          BG_OPT_PIVOT_ON_DEVICE is refused with BG_ERR_BAD_ARG.
 *   Errors: as bg_hyper_rom_run_wide, with r > 256 or m > 1024: BG_ERR_UNSUPPORTED_R, and work NULL or slots < 1 with B > 0:
 *   BG_ERR_WORKSPACE; B = 0: BG_OK with nothing launched.
 *   One workgroup of four waves per slot, one per compute unit (148 KB of LDS at any m); the sampled rows pass through LDS in
 *   slabs of 8, 16x16x4 fp64 matrix instructions for the projection and the elimination (csrc/rom_hyper_blocked.hip, sharing
 *   csrc/rom_blocked_device.hpp with bg_rom_run_blocked).  options: BG_OPT_SUPG | BG_OPT_NONUNIFORM | BG_OPT_FORCE_PIVOTED. */
int bg_hyper_rom_blocked_limits(int *max_r, int *max_m);
long long bg_hyper_rom_blocked_table_elems(int m, int r);
long long bg_hyper_rom_blocked_work_elems(int r);
int bg_hyper_rom_run_blocked(int N, int B, int r, int m, int nsteps, int projection, const int32_t *rows, const double *xi,
                             const double *xs, const double *PhiS, const double *q0, const double *u0s, const double *mu1,
                             const double *mu2, double dt, double E, double tol, int max_it, int options, double *work,
                             int slots, double *qhist, int32_t *iters, int32_t *flags, int32_t *info, const int32_t *order,
                             void *stream);

/* bg_wide_solve_pivoted -- x[b] = solve(A[b], b[b]) for a batch of dense systems of 1 <= n <= 96 unknowns by Gauss-Jordan
 *   elimination with partial pivoting, one workgroup of four waves per system on a persistent grid (one per compute unit;
 *   csrc/wide_solve.hip).  The routine is the repair solve of bg_hyper_rom_run_wide (rom_wide_device.hpp, wide_solve_pivoted).
 *   A    [B][n][n] row-major;  b, x [B][n];
 *   piv  [B][n] or null: piv[b][k] is the row of A[b] used as the pivot of column k -- the largest |entry| of that column
 *        among the rows not used before, the lowest such row on ties (the rows LAPACK's getrf exchanges into place k);
 *   info [B]: 0, or k + 1 when column k had no non-zero candidate (exactly singular: x[b] and piv[b] are then undefined;
 *        the other systems of the batch are not affected).
 *   Returns BG_ERR_UNSUPPORTED_R for n outside 1 .. 96, BG_ERR_BAD_ARG for B < 0 or a null A, b, x or info, BG_OK without a
 *   launch for B = 0.  x may not overlap A or b. */
int bg_wide_solve_pivoted(int B, int n, const double *A, const double *b, double *x, int32_t *piv, int32_t *info, void *stream);

/* bg_hyper_ann_rom_run -- the POD-ANN PROM time loop HYPER-REDUCED: both projections of pod_ann_prom are assembled from m
 *   sampled mesh rows with weights xi >= 0, Ar = sum_j xi_j w_j^T y_j and br = sum_j xi_j w_j^T R_j with the tangent
 *   W = U_p + U_s dN(q_p), y_j = (A W)[i_j], R_j = (A u - b)[i_j], w_j = W[i_j] (Galerkin) or y_j (LSPG).
 *   3 <= N <= bg_fom_max_n(): the kernel never touches a vector of mesh length.  reference: FEM/fem_burgers.py:1177-1251
 *   with the sums over mesh rows restricted and weighted and without the re-projection q_p = U_p^T u^n at the start of a
 *   step (below).  Opt-in: nothing routes here unless asked (burgers_hip/rom.py, pod_ann_run_hyper; hyper= of pod_ann_run
 *   and of the facade).  The caller packs once per bases, sampling and mesh:
 *   node   [nodes] int32: the sorted distinct stencil nodes i - 1, i, i + 1 (inside the mesh) of the sampled rows, m <= nodes
 *          <= 3 m.  The stencil nodes of a sampled row are consecutive table entries: the table is a compacted mesh;
 *   xn     [nodes] their coordinates;
 *   pos    [m] int32: the table position of every sampled row (node[pos[j]] is the mesh row; distinct; entries outside
 *          [0, nodes) are skipped);   xi  [m] the weights, finite, >= 0;
 *   UTn    [m8][nodes], m8 = n + nbar rounded up to 8, 16-byte aligned: the rows of bg_ann_rom_run's UT = [U_p^T; U_s^T]
 *          restricted to the table nodes, zero rows from n + nbar;
 *   q0     [B][n] = U_p^T u0;   u0n  [B][nodes] u0 at the table nodes;
 *   the closure: n_layers, widths, wt, bias, acts, alphas exactly as bg_ann_rom_run takes them;
 *   qhist  [B][nsteps+1][n] q_p of every step, row 0 = q0;  qshist [B][nsteps+1][nbar] the closure value q_s = N(q_p) of
 *          every step's decode (row 0: zeros), so that U = U_p q_p + U_s q_s is the kernel's own decode;
 *   iters, flags, info, options (BG_OPT_SUPG, BG_OPT_NO_TANGENT_REUSE; the table is always read as a non-uniform mesh):
 *          as bg_ann_rom_run; order: as bg_rom_run, entries outside [0, B) are skipped.
 *   The first pass of the run assembles at u0n itself with the tangent at q0.  Afterwards q_p carries over from step to
 *   step: for orthonormal [U_p U_s] it equals the reference's U_p^T u^n, and the first pass of a step reuses the tangent
 *   of the previous evaluation.  Row 0 is the Dirichlet row, row N - 1 has no right element: decided by node[], so a table
 *   node that is only a neighbour contributes nothing.
 *   Limits (bg_hyper_ann_rom_limits): n <= 8, nbar <= 128, widths <= 256, layers <= 8, m <= 256, nodes <= 768.
 *   Errors: N < 3, n, nbar, m, nodes or n_layers < 1, B or nsteps < 0, max_it < 1, dt <= 0, m > N, nodes outside
 *   [m, min(3 m, N)], a null operand or output with B > 0, UTn not 16-byte aligned, a model that does not fit its widths:
 *   BG_ERR_BAD_ARG; N > bg_fom_max_n(): BG_ERR_UNSUPPORTED_N; m, nodes or the model beyond the limits:
 *   BG_ERR_UNSUPPORTED_R; an unknown projection: BG_ERR_PROJECTION; B = 0: BG_OK with nothing launched.  Sizes the
 *   kernel does not cover are refused, never rerouted.
 *   One 256-thread workgroup per sample runs bg_ann_rom_run's loop on the table (csrc/rom_ann_loop_device.hpp,
 *   csrc/rom_hyper_ann.hip), instantiated for nodes <= 256, <= 512 and <= 768;
 *   bg_hyper_ann_rom_workgroups_per_cu(nodes) of them are resident per CU (0: no such table). */
int bg_hyper_ann_rom_limits(int *max_n, int *max_nbar, int *max_width, int *max_layers, int *max_m, int *max_nodes);
int bg_hyper_ann_rom_workgroups_per_cu(int nodes);
int bg_hyper_ann_rom_run(int N, int B, int n, int nbar, int m, int nodes, int nsteps, int projection, const int32_t *node,
                         const double *xn, const int32_t *pos, const double *xi, const double *UTn, const double *q0,
                         const double *u0n, const double *mu1, const double *mu2, int n_layers, const int *widths,
                         const float *const *wt, const float *const *bias, const int *acts, const float *alphas, double dt,
                         double E, double tol, int max_it, int options, double *qhist, double *qshist, int32_t *iters,
                         int32_t *flags, int32_t *info, const int32_t *order, void *stream);

/* bg_hyper_ann_rom_run_wide -- bg_hyper_ann_rom_run for up to 20 primary modes (the reference's second POD-ANN model:
 *   n = 17, nbar = 79), 3 <= N <= bg_fom_max_n().  reference: FEM/fem_burgers.py:1177-1251, 1254-1275 with the sums over
 *   mesh rows restricted and weighted and without the re-projection q_p = U_p^T u^n at the start of a step.  Opt-in:
 *   nothing routes here unless asked (burgers_hip/rom.py, pod_ann_run_hyper_wide; hyper= of pod_ann_run and of the facade
 *   send a sampling of a model with more than 8 primary modes here).
 *   Arguments, order, types, semantics and return codes are bg_hyper_ann_rom_run's, with these differences:
 *   UTn    [n + nbar][ut_ld], ut_ld = bg_hyper_ann_rom_wide_ut_ld(nodes) (512 up to 512 nodes, 768 beyond), 16-byte
 *          aligned: the rows of bg_ann_rom_run_wide's UT = [U_p^T; U_s^T] restricted to the table nodes, zero columns
 *          from nodes (the layout of bg_hyper_rbf_rom_run, not the row-padded one of bg_hyper_ann_rom_run);
 *   options BG_OPT_NO_TANGENT_REUSE is accepted and changes nothing: as in bg_ann_rom_run_wide the tangent is evaluated
 *          at the first pass of every step, at the q_p carried over;
 *   a sampled row whose neighbour the table does not hold is left out.
 *   The stopping rule is bg_ann_rom_run_wide's, |dq| / (|q_p| + 1e-14).
 *   Limits (bg_hyper_ann_rom_wide_limits): n <= 20, nbar <= 128, widths <= 256, layers <= 8, m <= 256, nodes <= 768.
 *   Checked in this order: N < 3, n, nbar, m, nodes or n_layers < 1, B or nsteps < 0, max_it < 1, dt <= 0:
 *   BG_ERR_BAD_ARG; an unknown projection: BG_ERR_PROJECTION; N > bg_fom_max_n(): BG_ERR_UNSUPPORTED_N; m or nodes beyond
 *   the limits: BG_ERR_UNSUPPORTED_R; m > N or nodes outside [m, min(3 m, N)]: BG_ERR_BAD_ARG; the model beyond the limits:
 *   BG_ERR_UNSUPPORTED_R, or not fitting its widths: BG_ERR_BAD_ARG; B = 0: BG_OK with nothing launched; a null operand or
 *   output, UTn not 16-byte aligned: BG_ERR_BAD_ARG.  Sizes the kernel does not cover are refused, never rerouted.
 *   One 256-thread workgroup per sample runs bg_ann_rom_run_wide's loop on the table (csrc/rom_ann_wide_loop_device.hpp,
 *   csrc/rom_hyper_ann_wide.hip), instantiated for nodes <= 256, <= 512 and <= 768;
 *   bg_hyper_ann_rom_wide_workgroups_per_cu(nodes) of them are resident per CU (2, 2, 1; 0: no such table). */
int bg_hyper_ann_rom_wide_limits(int *max_n, int *max_nbar, int *max_width, int *max_layers, int *max_m, int *max_nodes);
int bg_hyper_ann_rom_wide_workgroups_per_cu(int nodes);
int bg_hyper_ann_rom_wide_ut_ld(int nodes);
int bg_hyper_ann_rom_run_wide(int N, int B, int n, int nbar, int m, int nodes, int nsteps, int projection,
                              const int32_t *node, const double *xn, const int32_t *pos, const double *xi, const double *UTn,
                              const double *q0, const double *u0n, const double *mu1, const double *mu2, int n_layers,
                              const int *widths, const float *const *wt, const float *const *bias, const int *acts,
                              const float *alphas, double dt, double E, double tol, int max_it, int options, double *qhist,
                              double *qshist, int32_t *iters, int32_t *flags, int32_t *info, const int32_t *order,
                              void *stream);

/* bg_hyper_rbf_rom_run -- the POD-RBF PROM time loop HYPER-REDUCED: both projections of pod_rbf_prom are assembled from m
 *   sampled mesh rows with weights xi >= 0, Ar = sum_j xi_j w_j^T y_j and br = sum_j xi_j w_j^T R_j with the tangent
 *   W = U_p + U_s J(q_p), y_j = (A W)[i_j], R_j = (A u - b)[i_j], w_j = W[i_j] (Galerkin) or y_j (LSPG).
 *   3 <= N <= bg_fom_max_n(): the kernel never touches a vector of mesh length; the mesh side of an iteration costs what
 *   the table costs, the closure evaluation (Ns nbar n) what it costs in bg_rbf_rom_run.  reference:
 *   FEM/fem_burgers.py:1278-1398 with the sums over mesh rows restricted and weighted and without the re-projection
 *   q_p = U_p^T U0 of every iteration (below).  Opt-in: nothing routes here unless asked (burgers_hip/rom.py,
 *   pod_rbf_run_hyper; hyper= of pod_rbf_run and of the facade).  The caller packs once per bases, closure, sampling and mesh:
 *   node, xn, pos, xi: the table of the sorted distinct stencil nodes of the sampled rows, exactly as bg_hyper_ann_rom_run
 *          takes it (m <= nodes <= 3 m; pos entries outside [0, nodes) are skipped; a sampled row whose neighbour the
 *          table does not hold is left out);
 *   UTn    [n + nbar][ut_ld], ut_ld = bg_hyper_rbf_rom_ut_ld(nodes) (512 up to 512 nodes, 1024 beyond), 16-byte aligned:
 *          the rows of bg_rbf_rom_run's UT = [U_p^T; U_s^T] restricted to the table nodes, zero columns from nodes;
 *   XtT, Wd, bias, x_min, dx, eps, kind: the closure exactly as bg_rbf_rom_run takes it;
 *   q0     [B][n] = U_p^T u0;   u0n  [B][nodes] u0 at the table nodes;
 *   qhist  [B][nsteps+1][n] q_p of every step, row 0 = q0;  qshist [B][nsteps+1][nbar] the closure value f(q_p) of every
 *          step's decode (row 0: zeros), so that U = U_p q_p + U_s q_s is the kernel's own decode;
 *   iters, flags, info, options (BG_OPT_SUPG; the table is always read as a non-uniform mesh): as bg_rbf_rom_run;
 *          order: as bg_rom_run, entries outside [0, B) are skipped.
 *   The first iteration of the run assembles at u0n itself.  q_p carries over between iterations and steps: for
 *   orthonormal [U_p U_s] it equals the reference's U_p^T U0.  The stopping rule is bg_rbf_rom_run's (|dq| / |q_new|, |dq|
 *   when |q_new| = 0).  Row 0 is the Dirichlet row, row N - 1 has no right element: decided by node[], so a table node
 *   that is only a neighbour contributes nothing.
 *   Limits (bg_hyper_rbf_rom_limits): n <= 20, nbar <= 128, Ns <= 65536, m <= 256, nodes <= 768.
 *   Checked in this order: N < 3, n, nbar, Ns, m or nodes < 1, B or nsteps < 0, max_it < 1, dt <= 0: BG_ERR_BAD_ARG; an
 *   unknown kind: BG_ERR_BAD_ARG; an unknown projection: BG_ERR_PROJECTION; N > bg_fom_max_n(): BG_ERR_UNSUPPORTED_N; n,
 *   nbar, Ns, m or nodes beyond the limits: BG_ERR_UNSUPPORTED_R; m > N or nodes outside [m, min(3 m, N)]: BG_ERR_BAD_ARG;
 *   B = 0: BG_OK with nothing launched; a null operand or output, UTn or Wd not 16-byte aligned: BG_ERR_BAD_ARG.  Sizes
 *   the kernel does not cover are refused, never rerouted.
 *   One workgroup per sample runs bg_rbf_rom_run's loop on the table (csrc/rom_rbf_loop_device.hpp,
 *   csrc/rom_hyper_rbf.hip): 256 threads for nodes <= 256 and <= 512, 512 threads (the bg_rbf_rom_run_long profile) for
 *   nodes <= 768; bg_hyper_rbf_rom_workgroups_per_cu(nodes) of them are resident per CU (2, 1; 0: no such table). */
int bg_hyper_rbf_rom_limits(int *max_n, int *max_nbar, int *max_ns, int *max_m, int *max_nodes);
int bg_hyper_rbf_rom_workgroups_per_cu(int nodes);
int bg_hyper_rbf_rom_ut_ld(int nodes);
int bg_hyper_rbf_rom_run(int N, int B, int n, int nbar, int Ns, int m, int nodes, int nsteps, int projection, int kind,
                         const int32_t *node, const double *xn, const int32_t *pos, const double *xi, const double *UTn,
                         const double *XtT, const double *Wd, const double *bias, const double *x_min, const double *dx,
                         double eps, const double *q0, const double *u0n, const double *mu1, const double *mu2, double dt,
                         double E, double tol, int max_it, int options, double *qhist, double *qshist, int32_t *iters,
                         int32_t *flags, int32_t *info, const int32_t *order, void *stream);

/* bg_rom_run_long_wide -- bg_rom_run_wide for long meshes: 3 <= N <= 1024 (bg_rom_run_long_wide_max_n; meant for N > 512,
 *   where bg_rom_run_wide ends), r <= 96 (bg_rom_run_long_wide_max_r; meant for r > 40, where bg_rom_run_long ends).
 *   reference: FEM/fem_burgers.py:709-785.
 *   Opt-in: the facade routes 40 < r <= 96 on N > 512 here only when asked (burgers_hip/rom.py, long_wide=True).
 *   Same arguments, outputs and semantics as bg_rom_run_wide except:
 *   PhiP   [NPAD + 2][96], NPAD = N rounded up to 64 (bg_rom_run_long_wide_phi_elems(N) doubles, 16-byte aligned; 0 for an N
 *          the kernel does not cover): bg_rom_run_wide's layout -- Phi row i at row index i + 1, zero rows around and beyond
 *          the mesh, zero columns beyond r -- built once per basis by the caller;
 *   order  [B] or NULL; entries outside [0, B) are skipped.
 *   info   0, or BG_INFO_NEEDS_PIVOTING for a sample whose guarded pivot-free elimination met a multiplier above 1 below
 *          the diagonal or a zero pivot: the caller redoes that sample with a pivoting solve (there is no second kernel
 *          here; burgers_hip/rom.py sends it through the library path).
 *   Errors: N < 3, r < 1, B or nsteps < 0, max_it < 1, dt <= 0, a null operand or output with B > 0, PhiP not 16-byte
 *   aligned: BG_ERR_BAD_ARG; N > 1024: BG_ERR_UNSUPPORTED_N; r > 96: BG_ERR_UNSUPPORTED_R; an unknown projection:
 *   BG_ERR_PROJECTION; B = 0: BG_OK with nothing launched.
 *   The loop and the 96 x 96 solve by all four waves are bg_rom_run_wide's with u, g, h_f and dt F of 1024 mesh rows and
 *   the coefficients of one 64-row slab in LDS (csrc/rom_long_wide.hip: 147 824 B); workgroup k of G = min(B, CUs) takes
 *   the slots k, k + G, ...  options: BG_OPT_SUPG | BG_OPT_NONUNIFORM | BG_OPT_FORCE_PIVOTED (tests: every sample is handed
 *   back as if its elimination had needed a row exchange). */
int bg_rom_run_long_wide_max_n(void);
int bg_rom_run_long_wide_max_r(void);
long long bg_rom_run_long_wide_phi_elems(int N);
int bg_rom_run_long_wide(int N, int B, int r, int nsteps, int projection, const double *x, const double *PhiP,
                         const double *u0, const double *mu1, const double *mu2, double dt, double E, double tol,
                         int max_it, int options, double *hist, int32_t *iters, int32_t *flags, int32_t *info,
                         const int32_t *order, void *stream);

/* =================================================================================
 * bg_fd_run -- batched replacement of FDBurgers.fom_burgers_newton (analytical Jacobian)
 *   reference: FD/fd_burgers.py:59-107 (time + Newton loops), residual :28-35, Jacobian :37-44,
 *   boundary values :19-22 (U[0] = mu1, U[-1] = U[-2]).  Central differences with the lagged
 *   artificial viscosity nu = 0.25 dx max|U|; stop on max|R| < tol or max|dU|/max|U| < tol.
 *   Arrays as in bg_fom_run; x must be the linspace(a, b, N) of the reference; N <= 8192.
 *   iters[b][t] = Newton solves taken in step t; flags: BG_FLAG_HIT_CAP when max_it ran out in some step,
 *   BG_FLAG_NONFINITE when a sample's state went non-finite: the three maxima are NaN when an entry is, as the
 *   reference's np.max, so such a sample takes max_it solves in every later step and is never reported as converged.
 * ================================================================================= */
int bg_fd_run(int N, int B, int nsteps, const double *x, const double *u0, const double *mu1,
              const double *mu2, double dt, double tol, int max_it, double *hist, int32_t *iters,
              int32_t *flags, void *stream);

/* ---------------------------------------------------------------------------------
 * Quadratic-manifold tangent, fused with the layout the MFMA reduce kernel wants
 *   reference: tangent(q) = Phi + H @ get_dQ_dq(q)   FEM/fem_burgers.py:1120-1123, :292-312
 *   H3 [N][n][NP] = H[i][pair(a,c)] * (1 + delta_ac), q [B][NP]: last dimension zero-padded to
 *                   NP = bg_rom_frag_pad(n) (a multiple of 8; built once / padded on the host side)
 *   bg_rom_frag_elems(N, r): doubles per sample of the fragment-major layout (0 if N > 512 or r > 40)
 *   bg_quad_tangent:        Wfrag[b] = Phi + H3 . q[b]   for every active sample
 *   bg_rom_reduce_frag:     bg_rom_reduce with W given in that layout (stride = bg_rom_frag_elems)
 * --------------------------------------------------------------------------------- */
/* bg_quad_features -- feat[b] = [q[b] | Q(q[b])], Q = the n(n+1)/2 unique products q_i q_j (j >= i) in the order of
 *   get_sym (FEM/fem_burgers.py:263-273): the left operand of the decode u = Phi q + H Q(q) (:1116-1118) as one matrix, so
 *   that the decode is ONE GEMM against [Phi^T; H^T].  q [B][n]; pair_i, pair_j [n(n+1)/2] int32 (row-major upper
 *   triangle); feat [B][n + n(n+1)/2]. */
int bg_quad_features(int B, int n, const double *q, const int32_t *pair_i, const int32_t *pair_j, double *feat,
                     void *stream);
long long bg_rom_frag_elems(int N, int r);
int bg_rom_frag_pad(int r);
int bg_quad_tangent(int N, int B, int n, const double *Phi, const double *H3, const double *q,
                    const int32_t *active, double *Wfrag, void *stream);
int bg_rom_reduce_frag(int N, int B, int r, int projection, const double *x, const double *Wfrag,
                       const double *U, const double *G, const double *hfs, const double *mu1, double dt,
                       double E, int supg, const int32_t *active, double *Ar, double *br, double *wtu,
                       void *stream);

/* bg_mlp_act_jvp -- activation stage of a forward-mode MLP evaluation, float32, in place
 *   reference: compute_ann_jacobian FEM/fem_burgers.py:1254-1275 (per-sample autograd Jacobian of the
 *   POD-ANN closure) and the model call at :1241; the linear layers are library GEMMs over B*n1 rows.
 *   z      [B][n1][h]: row 0 = W x (no bias yet), rows 1..n1-1 = W (dx/dq_k)
 *   bias   [h] or NULL
 *   out:   row 0 <- act(row 0 + bias); rows k >= 1 <- act'(row 0 + bias) * row k
 *   act    BG_ACT_NONE | BG_ACT_ELU (alpha) | BG_ACT_RELU | BG_ACT_TANH */
int bg_mlp_act_jvp(int B, int n1, int h, float *z, const float *bias, int act, float alpha, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_quad_rom_run -- batched replacement of FEMBurgers.pod_quadratic_manifold, the WHOLE time loop on the device
 *   reference: FEM/fem_burgers.py:1081-1175 (decoder :1116-1118, tangent :1120-1123 with get_dQ_dq :292-312 folded
 *   in, Newton loop :1126-1173); called by Quadratic_manifold/quadratic_prom_simulation.py:49-55.
 *   One 256-thread workgroup owns FOUR samples for all time steps and iterations: tangent T = Phi + H3 q of the four
 *   samples on v_mfma_f64_4x4x4_4b (H3 streamed once per four sample-iterations), decode u = 1/2 (Phi q + T q) from
 *   the same rows, assembly, projection and the n x n solve per wave (csrc/quad_fused.hip).  No SUPG term (:1142).
 *   N <= 512, n <= bg_quad_rom_max_n() (40).  Operand copies, built once per basis by the caller (zero padded):
 *     PhiT [40][NPAD]               Phi^T, NPAD = N rounded up to 64
 *     Phif [NG][10][16]             Phi[4 rg + blk][4 c + i] at [rg][c][4 i + blk], NG = ceil(N / 4)
 *     H3f  [NG][28][64][2]          H3[i][a][c] = H[i][pair(a, c)] (1 + delta_ac) is symmetric in (a, c): only its upper 4 x 4
 *                                   blocks (A <= B, row-major, 55 per mesh-row group) are stored, two per 16-byte slot:
 *                                   block p = 2 slot + e of row group rg holds, at lane 16 k + 4 blk + i,
 *                                   H3[4 rg + blk][4 A + i][4 B + k]   (the A operand of the matrix instruction; block 55 = 0)
 *     sizes: bg_quad_rom_phif_elems(N), bg_quad_rom_h3f_elems(N) doubles.
 *   Outputs as bg_rom_run: hist [B][nsteps+1][N], iters [B][nsteps] (Newton iterations per step), flags [B]
 *   (BG_FLAG_HIT_CAP = "Newton did not converge" :1171, BG_FLAG_NONFINITE), info [B]: 0, or k + 1 when the reduced
 *   system met an exactly zero pivot at elimination step k (np.linalg.solve :1161 raises LinAlgError: so does the facade).
 *   options: BG_OPT_NONUNIFORM.
 * --------------------------------------------------------------------------------- */
int bg_quad_rom_max_n(void);
long long bg_quad_rom_h3f_elems(int N);
long long bg_quad_rom_phif_elems(int N);
int bg_quad_rom_run(int N, int B, int n, int nsteps, int projection, const double *x, const double *PhiT,
                    const double *Phif, const double *H3f, const double *u0, const double *mu1, const double *mu2,
                    double dt, double E, double tol, int max_it, int options, double *hist, int32_t *iters,
                    int32_t *flags, int32_t *info, const int32_t *order, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_quad_rom_run_long -- bg_quad_rom_run for meshes of 513 <= N <= bg_quad_rom_run_long_max_n() (1024) nodes,
 *   n <= bg_quad_rom_run_long_max_r() (40) (csrc/quad_long.hip).  Same argument list, operand meaning, mathematics and
 *   outputs as bg_quad_rom_run; the per-node arrays g = M u^n + dt F and dt F live in the registers of the wave that
 *   owns the sample instead of LDS.  N <= 512 is REFUSED with BG_ERR_UNSUPPORTED_N (bg_quad_rom_run covers it), as is
 *   N > 1024.  Operand copies, built once per basis by the caller (zero padded; the layouts of bg_quad_rom_run):
 *     PhiT [40][NPAD]               Phi^T, NPAD = N rounded up to 64; 16-byte aligned
 *     Phif [NG][10][16]             Phi[4 rg + blk][4 c + i] at [rg][c][4 i + blk], NG = ceil(N / 4)
 *     H3f  [NG][28][64][2]          the upper 4 x 4 blocks of the symmetric tangent tensor in A-operand order, exactly as
 *                                   documented for bg_quad_rom_run; 16-byte aligned
 *     sizes: bg_quad_rom_run_long_phit_elems(N), _phif_elems(N), _h3f_elems(N) doubles (0 for an N that is not covered).
 *   order: wave w of workgroup slot g works on sample order[4 g + w]; entries outside [0, B) are skipped (their rows of
 *   hist, iters, flags, info are not written).  A sample's result does not depend on the samples that share its
 *   workgroup or launch.  The launch uses min(ceil(B / 4), CUs * bg_quad_rom_run_long_workgroups_per_cu()) workgroups.
 *   Checked before any launch: N < 3, B < 0, n < 1, nsteps < 0, max_it < 1, dt <= 0: BG_ERR_BAD_ARG; an unknown
 *   projection: BG_ERR_PROJECTION; N outside 513 .. 1024: BG_ERR_UNSUPPORTED_N; n > 40: BG_ERR_UNSUPPORTED_R; B = 0: BG_OK
 *   (pointers may be null); a null operand or output with B > 0, or a misaligned PhiT / H3f: BG_ERR_BAD_ARG.
 *   options: BG_OPT_NONUNIFORM.
 * --------------------------------------------------------------------------------- */
int bg_quad_rom_run_long_max_n(void);
int bg_quad_rom_run_long_max_r(void);
int bg_quad_rom_run_long_workgroups_per_cu(void);
long long bg_quad_rom_run_long_phit_elems(int N);
long long bg_quad_rom_run_long_phif_elems(int N);
long long bg_quad_rom_run_long_h3f_elems(int N);
int bg_quad_rom_run_long(int N, int B, int n, int nsteps, int projection, const double *x, const double *PhiT,
                         const double *Phif, const double *H3f, const double *u0, const double *mu1, const double *mu2,
                         double dt, double E, double tol, int max_it, int options, double *hist, int32_t *iters,
                         int32_t *flags, int32_t *info, const int32_t *order, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_hyper_quad_rom_run -- the quadratic-manifold PROM time loop HYPER-REDUCED: both projections of pod_quadratic_manifold
 *   are assembled from m sampled mesh rows with weights xi >= 0, Ar = sum_j xi_j w_j^T y_j and br = sum_j xi_j w_j^T R_j
 *   with the tangent T = Phi + H dQ/dq(q), y_j = (A T)[i_j], R_j = (A u - b)[i_j], w_j = T[i_j] (Galerkin) or y_j (LSPG).
 *   3 <= N <= bg_fom_max_n(): the kernel never touches a vector of mesh length, and a pass streams the H3 rows of the table
 *   alone.  reference: FEM/fem_burgers.py:1081-1175 with the sums over mesh rows restricted and weighted and without the
 *   re-projection q = Phi^T u^n at the start of a step (below).  No SUPG term (:1142).  Opt-in: nothing routes here unless
 *   asked (burgers_hip/rom.py, quadratic_run_hyper; hyper= of quadratic_run and of the facade).  The caller packs once per
 *   manifold, sampling and mesh:
 *   xn, node, pos, xi: the table of the sorted distinct stencil nodes of the sampled rows, as bg_hyper_ann_rom_run takes
 *          it, the coordinates first (xn [nodes]; node [nodes] int32 ascending, m <= nodes <= 3 m; pos [m] int32, entries
 *          outside [0, nodes) are skipped; xi [m] finite, >= 0);
 *   Phif   [NG][10][16], H3f [NG][28][64][2] (16-byte aligned), NG = ceil(nodes / 4): bg_quad_rom_run's operand copies built
 *          from Phi[node] and H[node], the table in place of the mesh; sizes bg_hyper_quad_rom_phif_elems(nodes),
 *          bg_hyper_quad_rom_h3f_elems(nodes) doubles (0 outside 1 .. 768).  No PhiT: nothing is re-projected;
 *   q0     [B][n] = Phi^T u0;   u0n  [B][nodes] u0 at the table nodes;
 *   qhist  [B][nsteps+1][n] q of every step, row 0 = q0: U = Phi q + H Q(q) is the kernel's own decode;
 *   iters, flags, info: as bg_quad_rom_run; options: not read (the table is always a non-uniform mesh);
 *   order: as bg_quad_rom_run_long, entries outside [0, B) are skipped.
 *   The mass row of the first step reads u0n itself; every pass assembles at the decode of its q.  q carries over from step
 *   to step: for orthonormal Phi and Phi^T H = 0 (a manifold fitted on the residual of the projection) it equals the
 *   reference's Phi^T u^n.  Row 0 is the Dirichlet row, row N - 1 has no right element: decided by node[], so a table node
 *   that is only a neighbour contributes nothing.
 *   Limits (bg_hyper_quad_rom_limits): n <= 40, m <= 256, nodes <= 768.
 *   Errors, in this order: N < 3, n, m or nodes < 1, B or nsteps < 0, max_it < 1, dt <= 0: BG_ERR_BAD_ARG; an unknown
 *   projection: BG_ERR_PROJECTION; N > bg_fom_max_n(): BG_ERR_UNSUPPORTED_N; n, m or nodes beyond the limits:
 *   BG_ERR_UNSUPPORTED_R; m > N or nodes outside [m, min(3 m, N)]: BG_ERR_BAD_ARG; B = 0: BG_OK with nothing launched
 *   (pointers may be null); a null operand or output with B > 0, H3f not 16-byte aligned: BG_ERR_BAD_ARG.  Sizes the kernel
 *   does not cover are refused, never rerouted.
 *   One 256-thread workgroup owns four samples and runs bg_quad_rom_run's loop on the table (csrc/quad_device.hpp,
 *   csrc/quad_hyper.hip), instantiated for nodes <= 512 and <= 768; bg_hyper_quad_rom_workgroups_per_cu(nodes) of them
 *   are resident per CU (0: no such table).
 * --------------------------------------------------------------------------------- */
int bg_hyper_quad_rom_limits(int *max_n, int *max_m, int *max_nodes);
int bg_hyper_quad_rom_workgroups_per_cu(int nodes);
long long bg_hyper_quad_rom_phif_elems(int nodes);
long long bg_hyper_quad_rom_h3f_elems(int nodes);
int bg_hyper_quad_rom_run(int N, int B, int n, int m, int nodes, int nsteps, int projection, const double *xn,
                          const int32_t *node, const int32_t *pos, const double *xi, const double *Phif, const double *H3f,
                          const double *q0, const double *u0n, const double *mu1, const double *mu2, double dt, double E,
                          double tol, int max_it, int options, double *qhist, int32_t *iters, int32_t *flags,
                          int32_t *info, const int32_t *order, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_ann_rom_run -- batched replacement of FEMBurgers.pod_ann_prom, the WHOLE time loop on the device
 *   reference: FEM/fem_burgers.py:1177-1251 (loop), compute_ann_jacobian :1254-1275, model POD-ANN/pod_ann.py:38-56.
 *   One workgroup owns one sample for all time steps and Gauss-Newton iterations: assembly, fp64-MFMA projection of the
 *   tangent W = U_p + U_s dN (:1224), the n x n solve (:1237), q_p += dq with err = |dq| / (|q_p| + 1e-14) (:1238-1244),
 *   the closure N(q_p) with its input-Jacobian in one float32 forward-mode pass (the reference evaluates the model in
 *   float32 too), and the decode u = U_p q_p + U_s N(q_p) (:1242).  At the start of a time step q_p = U_p^T u (:1197).
 *   UT     [m8][N] row-major, m8 = (n + nbar) rounded up to a multiple of 8: rows 0 .. n-1 = U_p^T (the columns of U_p,
 *          contiguous), rows n .. n+nbar-1 = U_s^T, the rest zero; n <= 8, nbar <= 128, N <= 512.  One array because the
 *          decode and the tangent are ONE sweep over all n + nbar modes, eight at a time.
 *   the closure, layer l = 0 .. n_layers-1 (n_layers <= 8), all four arrays HOST arrays of length n_layers (widths:
 *   n_layers + 1, widths[0] = n, widths[n_layers] = nbar, every width <= 256):
 *     wt[l]    DEVICE pointer, 16-byte aligned, float32 [in4][ld] row-major = the TRANSPOSE of torch's Linear.weight
 *              zero-padded to in4 = widths[l] rounded up to 4 rows and ld = widths[l+1] rounded up to 8 columns (a thread
 *              fetches the weights of 8 outputs of one input as two 16-byte loads, unguarded)
 *     bias[l]  DEVICE pointer, float32 [widths[l+1]], or NULL
 *     acts[l]  BG_ACT_* applied after layer l, alphas[l] its ELU alpha
 *   limits are reported by bg_ann_rom_limits; a model outside them returns BG_ERR_UNSUPPORTED_R (use the per-iteration
 *   entry points bg_mlp_act_jvp + bg_rom_reduce + bg_lu_solve_update instead).
 *   u0, mu1, mu2, hist, iters, flags, info: as bg_rom_run; options BG_OPT_SUPG (pod_ann_prom has it) | BG_OPT_NONUNIFORM |
 *   BG_OPT_NO_TANGENT_REUSE.  The first-pass tangent of a time step is dN at float32(U_p^T u^n) (:1197, :1219); when those
 *   floats are bitwise the input of the previous step's last evaluation (the rule: u^n is that step's decode), the tangent is
 *   still on chip and the evaluation, which would reproduce it bit for bit, is skipped.
 *   The n x n solve is np.linalg.solve's elimination with the pivot search, always (one kernel): the columns of
 *   U_p + U_s dN are far from orthonormal and LAPACK does leave the diagonal on these systems.
 * --------------------------------------------------------------------------------- */
int bg_ann_rom_limits(int *max_n, int *max_nbar, int *max_width, int *max_layers);
int bg_ann_rom_run(int N, int B, int n, int nbar, int nsteps, int projection, const double *x, const double *UT,
                   const double *u0, const double *mu1, const double *mu2, int n_layers,
                   const int *widths, const float *const *wt, const float *const *bias, const int *acts,
                   const float *alphas, double dt, double E, double tol, int max_it, int options, double *hist,
                   int32_t *iters, int32_t *flags, int32_t *info, const int32_t *order, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_ann_rom_run_wide -- bg_ann_rom_run for models of up to 20 primary modes (the reference's n = 17, nbar = 79 POD-ANN model)
 *   reference: FEM/fem_burgers.py:1177-1251 (loop), compute_ann_jacobian :1254-1275, model POD-ANN/pod_ann.py:38-56.
 *   The mathematics, phases, result contract, flags and info of bg_ann_rom_run (csrc/rom_ann_wide.hip): one workgroup owns
 *   one sample for all time steps and Gauss-Newton iterations; q_p = U_p^T u^n at the start of a time step only (:1197),
 *   q_p += dq, err = |dq| / (|q_p| + 1e-14) (:1238-1244); the closure N(q_p) and its input-Jacobian in ONE float32
 *   forward-mode pass (:1219, :1241), everything else fp64.  The mesh side is bg_rbf_rom_run's: the tangent
 *   W = U_p + U_s dN (:1224) is formed in the projection's fragment registers from an nbar x 20 table, five 4-column MFMA
 *   blocks, and the n x n solve (:1237) is np.linalg.solve's elimination with the pivot search, always; info = k + 1 on an
 *   exactly zero pivot.
 *   UT     [n + nbar][512] row-major, 16-byte aligned: rows 0 .. n-1 = U_p^T, rows n .. n+nbar-1 = U_s^T, every row
 *          with zero columns from N to 511 (the layout bg_rbf_rom_run reads: the mesh-side code is the same).
 *   the closure: n_layers, widths, wt, bias, acts, alphas exactly as bg_ann_rom_run takes them (wt[l] float32 [in4][ld],
 *          16-byte aligned, in4 = widths[l] rounded up to 4 rows, ld = widths[l+1] rounded up to 8 columns, zero fill;
 *          a thread fetches the weights of 4 outputs of one input as one 16-byte load, unguarded).
 *   Limits (bg_ann_rom_run_wide_limits: max_n 20, max_nbar 128, max_width 256, max_layers 8; every output optional):
 *   2 <= N <= 512, 1 <= n <= 20 (n <= 8 is accepted on purpose: the two entry points can be compared on one model).
 *   Checks, in this order: BG_ERR_BAD_ARG (N < 2, B < 0, n < 1, nbar < 1, nsteps < 0, max_it < 1, dt <= 0, n_layers < 1),
 *   BG_ERR_PROJECTION, BG_ERR_UNSUPPORTED_N (N > 512), BG_ERR_UNSUPPORTED_R (n > 20, nbar > 128, n_layers > 8), then
 *   BG_ERR_BAD_ARG for a null closure array, widths[0] != n or widths[n_layers] != nbar, per layer BG_ERR_UNSUPPORTED_R
 *   for a width outside 1 .. 256 and BG_ERR_BAD_ARG for a null or misaligned wt[l] or an unknown activation; B = 0 returns
 *   BG_OK before any batch pointer is looked at; then null batch pointers and a misaligned UT are BG_ERR_BAD_ARG.
 *   u0, mu1, mu2, hist, iters, flags (BG_FLAG_HIT_CAP, BG_FLAG_NONFINITE), info: as bg_ann_rom_run.  order: as bg_rom_run;
 *   entries outside [0, B) are skipped.  options BG_OPT_SUPG | BG_OPT_NONUNIFORM | BG_OPT_NO_TANGENT_REUSE: the tangent is
 *   not resident across the projection, so the closure is evaluated at every step start and the last option changes nothing.
 * --------------------------------------------------------------------------------- */
int bg_ann_rom_run_wide_limits(int *max_n, int *max_nbar, int *max_width, int *max_layers);
int bg_ann_rom_run_wide(int N, int B, int n, int nbar, int nsteps, int projection, const double *x, const double *UT,
                        const double *u0, const double *mu1, const double *mu2, int n_layers, const int *widths,
                        const float *const *wt, const float *const *bias, const int *acts, const float *alphas,
                        double dt, double E, double tol, int max_it, int options, double *hist, int32_t *iters,
                        int32_t *flags, int32_t *info, const int32_t *order, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_rbf_rom_run -- batched replacement of FEMBurgers.pod_rbf_prom, the WHOLE time loop on the device
 *   reference: FEM/fem_burgers.py:1278-1398 (loop), the scaled RBF closure :160-260 (interpolate_with_rbf_scaled
 *   :225-236, compute_rbf_jacobian_full :238-260).
 *   One workgroup owns one sample for all time steps and Gauss-Newton iterations (csrc/rom_rbf_fused.hip).  Per iteration:
 *   q_p = U_p^T u, recomputed from the current iterate (:1352); the closure Jacobian at q_p; the tangent
 *   W = U_p + U_s J (:1361); assembly with SUPG and the projection; the n x n solve with partial pivoting (:1365);
 *   q_new = q_p + dq with err = |dq| / |q_new|, or |dq| when |q_new| = 0 (:1366-1390); the closure value at q_new and the
 *   decode u = U_p q_new + U_s f(q_new) (:1378-1381).  All fp64.
 *   The closure, with xs = 2 (q - x_min) / dx - 1, r2_i = |xs - Xt_i|^2 (kind BG_RBF_GAUSSIAN: phi = exp(-eps^2 r2),
 *   BG_RBF_IMQ: phi = (1 + eps^2 r2)^(-1/2)):  f(q) = phi(q) Wd + bias, J = d f / d q (the forms of bg_rbf_eval).
 *   Operand copies, built once per closure and basis by the caller (burgers_hip/rom.py::RbfFusedPlan):
 *     UT     [n + nbar][512], 16-byte aligned: rows 0 .. n-1 = U_p^T, rows n .. n+nbar-1 = U_s^T, zero columns from N
 *     XtT    [n][Ns]     the centres X_train transposed (centre index fastest)
 *     Wd     [Ns][128], 16-byte aligned: W diag(dy / 2), zero columns from nbar (dy = y_max - y_min, entries below 1e-15 -> 1)
 *     bias   [128]       dy / 2 + y_min, zero from nbar
 *     x_min  [n], dx [n] x_max - x_min with entries below 1e-15 replaced by 1
 *   Limits (bg_rbf_rom_limits): N <= 512 (BG_ERR_UNSUPPORTED_N), n <= 20, nbar <= 128, Ns <= 65536 (BG_ERR_UNSUPPORTED_R);
 *   the centres stream through LDS in tiles.  N < 3, n, nbar, Ns < 1, an unknown kind or a null operand: BG_ERR_BAD_ARG.
 *   u0, mu1, mu2, hist, iters, flags, info, order: as bg_rom_run (order entries outside [0, B) are skipped); flags:
 *   BG_FLAG_HIT_CAP when an iteration count reaches max_it, BG_FLAG_NONFINITE for a non-finite error; info: 0, or k + 1
 *   when the reduced system met an exactly zero pivot at elimination step k (the sample stops there).
 *   options: BG_OPT_SUPG (pod_rbf_prom has it) | BG_OPT_NONUNIFORM.
 * --------------------------------------------------------------------------------- */
int bg_rbf_rom_limits(int *max_n, int *max_nbar, int *max_ns);
int bg_rbf_rom_run(int N, int B, int n, int nbar, int Ns, int nsteps, int projection, int kind, const double *x,
                   const double *UT, const double *XtT, const double *Wd, const double *bias, const double *x_min,
                   const double *dx, double eps, const double *u0, const double *mu1, const double *mu2, double dt,
                   double E, double tol, int max_it, int options, double *hist, int32_t *iters, int32_t *flags,
                   int32_t *info, const int32_t *order, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_rbf_rom_run_long -- bg_rbf_rom_run for meshes of 513 <= N <= 1024 nodes
 *   The same kernel source, mathematics, phases, result contract, flags and info as bg_rbf_rom_run, instantiated for ONE
 *   512-thread workgroup of eight waves per compute unit: 128 owners of 8 mesh rows, the register profile and the two waves
 *   per SIMD of bg_rbf_rom_run at N = 512, eight per-wave partial systems summed in a fixed order; 141 KB of LDS.
 *   Operand copies as bg_rbf_rom_run except
 *     UT     [n + nbar][1024], 16-byte aligned, zero columns from N   (burgers_hip/rom.py::RbfFusedPlan(long_mesh=True))
 *   Limits (bg_rbf_rom_run_long_limits: max_n 1024, max_r 20, max_nbar 128, max_ns 65536; every output optional):
 *   N > 1024 and N <= 512 are BG_ERR_UNSUPPORTED_N (bg_rbf_rom_run covers the short meshes: what is accepted is what is
 *   tested); n > 20, nbar > 128, Ns > 65536: BG_ERR_UNSUPPORTED_R.  BG_ERR_BAD_ARG and BG_ERR_PROJECTION as bg_rbf_rom_run,
 *   checked in the same order; B = 0 returns BG_OK before any pointer is looked at.
 * --------------------------------------------------------------------------------- */
int bg_rbf_rom_run_long_limits(int *max_n, int *max_r, int *max_nbar, int *max_ns);
int bg_rbf_rom_run_long(int N, int B, int n, int nbar, int Ns, int nsteps, int projection, int kind, const double *x,
                        const double *UT, const double *XtT, const double *Wd, const double *bias, const double *x_min,
                        const double *dx, double eps, const double *u0, const double *mu1, const double *mu2, double dt,
                        double E, double tol, int max_it, int options, double *hist, int32_t *iters, int32_t *flags,
                        int32_t *info, const int32_t *order, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_local_rom_run -- batched replacement of FEMBurgers.local_prom_burgers, the WHOLE time loop on the device
 *   reference: FEM/fem_burgers.py:979-1079.  bg_rom_run with one basis per time step (csrc/rom_fused.hip, the LOCAL
 *   variant of the same kernel): at the start of every step the sample's cluster is c = argmin_c |q_g - centres[c]|^2
 *   with q_g = U_g^T u^n (kmeans.predict, :1011-1012; the distance summed in j order, the first index of the minimum);
 *   the step then iterates like pod_prom_burgers in that cluster's basis of width widths[c] (:1013-1060).  A workgroup
 *   reloads its register-resident basis only when the cluster changes (kept across the samples it works on).
 *   bases    [C][N][rmax] row-major: cluster c's basis in columns 0 .. widths[c]-1, zeros beyond
 *   widths   [C] int32, 1 .. rmax
 *   UgT      [m][N]: U_global[:, :m] transposed (m = num_global_modes)
 *   centres  [C][m] (the KMeans cluster_centers_)
 *   clusters [B][nsteps] int32 or NULL: the cluster of every sample and step
 *   Limits (bg_local_rom_limits): N <= 512 (BG_ERR_UNSUPPORTED_N), rmax <= 40, m <= 64, C <= 64 (BG_ERR_UNSUPPORTED_R).
 *   N < 2, B, nsteps < 0, C, rmax, m, max_it < 1, dt <= 0 or a null operand with B > 0: BG_ERR_BAD_ARG.
 *   u0, mu1, mu2, hist, iters, flags, info, order: as bg_rom_run, including the repair kernel that redoes a sample whose
 *   pivot-free elimination met a multiplier above 1 (it takes the same cluster path).
 *   options: BG_OPT_SUPG (local_prom_burgers has it) | BG_OPT_NONUNIFORM | BG_OPT_FORCE_PIVOTED.
 * --------------------------------------------------------------------------------- */
int bg_local_rom_limits(int *max_r, int *max_m, int *max_clusters);
int bg_local_rom_run(int N, int B, int C, int rmax, int m, int nsteps, int projection, const double *x,
                     const double *bases, const int32_t *widths, const double *UgT, const double *centres,
                     const double *u0, const double *mu1, const double *mu2, double dt, double E, double tol,
                     int max_it, int options, double *hist, int32_t *iters, int32_t *flags, int32_t *info,
                     int32_t *clusters, const int32_t *order, void *stream);

/* bg_local_rom_run_long -- bg_local_rom_run for long meshes: 3 <= N <= 1024 (meant for N > 512, where bg_local_rom_run
 *   ends), widths <= 40, m <= 64, C <= 64 (bg_local_rom_run_long_limits).  reference: FEM/fem_burgers.py:979-1079.
 *   Opt-in: the facade routes N > 512 here only when asked (burgers_hip/rom.py, fused=True, long_mesh=True).
 *   The loop of bg_rom_run_long (csrc/rom_local_long.hip: the basis streams through LDS) with the cluster pick of
 *   bg_local_rom_run at the start of every step, in the same arithmetic; the step's sweeps stream the picked cluster's
 *   block of the stack, and the solve gives the unknowns at and beyond widths[c] a zero correction.
 *   Same arguments, outputs and semantics as bg_local_rom_run except:
 *   bases  [C][NPAD + 2][40], NPAD = N rounded up to 64 (bg_local_rom_run_long_bases_elems(N, C) doubles, 16-byte
 *          aligned; 0 for an N or C the kernel does not cover): block c is cluster c's basis laid out like
 *          bg_rom_run_long's PhiP -- basis row i at row index i + 1, zero rows around and beyond the mesh, zero columns
 *          beyond widths[c] -- built once per clustering by the caller;
 *   rmax   the widest width (widths[c] is clamped to it);
 *   order  [B] or NULL; entries outside [0, B) are skipped.
 *   Errors: N < 3, B or nsteps < 0, C, rmax, m, max_it < 1, dt <= 0, a null operand or output with B > 0, bases not
 *   16-byte aligned: BG_ERR_BAD_ARG; N > 1024: BG_ERR_UNSUPPORTED_N; rmax > 40, m > 64, C > 64: BG_ERR_UNSUPPORTED_R; an
 *   unknown projection: BG_ERR_PROJECTION; B = 0: BG_OK with nothing launched.
 *   info, the repair kernel inside the call (it takes the same cluster path) and the workgroups per CU
 *   (bg_rom_run_long_workgroups_per_cu) are as in bg_rom_run_long.
 *   options: BG_OPT_SUPG | BG_OPT_NONUNIFORM | BG_OPT_FORCE_PIVOTED (tests: every sample through the second kernel). */
int bg_local_rom_run_long_limits(int *max_n, int *max_r, int *max_m, int *max_clusters);
long long bg_local_rom_run_long_bases_elems(int N, int C);
int bg_local_rom_run_long(int N, int B, int C, int rmax, int m, int nsteps, int projection, const double *x,
                          const double *bases, const int32_t *widths, const double *UgT, const double *centres,
                          const double *u0, const double *mu1, const double *mu2, double dt, double E, double tol,
                          int max_it, int options, double *hist, int32_t *iters, int32_t *flags, int32_t *info,
                          int32_t *clusters, const int32_t *order, void *stream);

/* bg_hyper_local_rom_run -- the local POD PROM time loop HYPER-REDUCED: bg_hyper_rom_run with one basis per time step, the
 *   reduced system of every cluster assembled from the SAME m sampled mesh rows and weights (one sampling for all clusters).
 *   3 <= N <= bg_fom_max_n(): the kernel never touches a vector of mesh length, so the pick and the change of basis work on
 *   reduced coordinates.  widths <= 40, m <= 256, mg <= 64, C <= 64 (bg_hyper_local_rom_limits).
 *   reference: FEM/fem_burgers.py:979-1079 with the sums over mesh rows restricted and weighted; with all rows, unit weights
 *   and orthonormal bases the loop is the reference's.  Opt-in: nothing routes here unless asked (burgers_hip/rom.py,
 *   local_prom_run_hyper; the facade's hyper=).
 *   The state of a sample is (p, q): the cluster held and the coordinates in its basis, u = Phi_p q.
 *   rows, xi, xs, u0s, mu1, mu2, iters, flags, info, order, options: as bg_hyper_rom_run;
 *   PhiS     [C][MPAD][3][42] (bg_hyper_local_rom_table_elems(C, m) doubles, 16-byte aligned; 0 for a C or m the kernel does
 *            not cover): block c is bg_hyper_rom_run's table of cluster c's basis, zero columns beyond widths[c];
 *   widths   [C] int32, 1 .. rmax (clamped to rmax);
 *   trans    [C][C][40][40]: trans[c][p] = Phi_c^T Phi_p, zero rows beyond widths[c] and zero columns beyond widths[p];
 *   pick     [C][mg][40]: pick[p] = U_g^T Phi_p with U_g the first mg global modes, zero columns beyond widths[p];
 *   centres  [C][mg] (the KMeans cluster_centers_);
 *   qg0      [B][mg] = U_g^T u0;   pu0  [B][C][rmax] = Phi_c^T u0 for every cluster, zero beyond widths[c];
 *   qhist    [B][nsteps+1][rmax]: entry n + 1 holds the coordinates in the basis of clusters[b][n], zero beyond its width;
 *            entry 0 is pu0 of the first cluster; the caller decodes U = Phi_c q;
 *   clusters [B][nsteps] int32 or NULL: the cluster of every sample and step.
 *   Step n >= 1 starts with q_g = pick[p] q and c = argmin_c |q_g - centres[c]|^2 (the distance summed in j order, the first
 *   index of the minimum, a NaN distance counting as the smallest: the pick of bg_local_rom_run); step 0 picks from qg0 and
 *   starts from pu0 and u0s.  If c != p, one lift-only sweep over table p leaves u^n = Phi_p q at the stencil nodes, which
 *   the first iteration of the step assembles at (g = M u^n + dt F, A and R, as the reference does with U0 = u^n outside the
 *   new span) while Y and W come from table c; the base of the update is q <- trans[c][p] q, the reference's
 *   q = Phi_c^T U0 + dq.  From the second iteration on, and in steps without a switch, the step is bg_hyper_rom_run's with
 *   the width widths[c]: unknowns at and beyond it get a unit diagonal and a zero correction.  A step without a switch
 *   costs no sweep more than bg_hyper_rom_run's.  The repair kernel redoes a marked sample from u0 and recomputes its picks.
 *   Errors: N < 3, C, rmax, mg, m, max_it < 1, B or nsteps < 0, dt <= 0, m > N, a null operand or output with B > 0
 *   (clusters may be null), PhiS not 16-byte aligned: BG_ERR_BAD_ARG; N > bg_fom_max_n(): BG_ERR_UNSUPPORTED_N; rmax > 40,
 *   m > 256, mg > 64 or C > 64: BG_ERR_UNSUPPORTED_R; an unknown projection: BG_ERR_PROJECTION; B = 0: BG_OK with nothing
 *   launched.  Sizes the kernel does not cover are refused, never rerouted.
 *   csrc/rom_hyper_local.hip: the LOCAL instantiations of csrc/rom_hyper.hip's loop; workgroup k of G = min(B, 2 CUs) takes
 *   the slots k, k + G, ... */
int bg_hyper_local_rom_limits(int *max_r, int *max_m, int *max_mg, int *max_clusters);
long long bg_hyper_local_rom_table_elems(int C, int m);
int bg_hyper_local_rom_run(int N, int B, int C, int rmax, int mg, int m, int nsteps, int projection, const int32_t *rows,
                           const double *xi, const double *xs, const double *PhiS, const int32_t *widths,
                           const double *trans, const double *pick, const double *centres, const double *qg0,
                           const double *pu0, const double *u0s, const double *mu1, const double *mu2, double dt, double E,
                           double tol, int max_it, int options, double *qhist, int32_t *iters, int32_t *flags, int32_t *info,
                           int32_t *clusters, const int32_t *order, void *stream);

/* bg_decode_modes_bf16 -- the contraction of the non-intrusive POD-ANN decoder (bf16 tier of BASELINE config 5)
 *   reference: `Uhat = U_modes @ Qhat.T`, Non-Instrusive/predict_pod_ann.py:73-80, for a batch of (mu1, mu2) samples
 *   out[b][i][t] = sum_k Um[i][k] * Q[b * Nt + t][k]: bf16 operands, float32 accumulate, each result written once as
 *   float64 in the (N, Nt) C-order snapshot layout per sample.
 *   Um  [N][n] bf16 (raw 16-bit patterns), Q [B * Nt][n] bf16 (the MLP output), both 16-byte aligned; out [B][N][Nt]
 *   N a multiple of 32, n a multiple of 16, n <= 256 (BG_ERR_UNSUPPORTED_N / _R otherwise: use a library GEMM). */
int bg_decode_modes_bf16(int N, int n, int B, int Nt, const uint16_t *Um, const uint16_t *Q, double *out, void *stream);

/* bg_decode_mlp_bf16 -- the whole non-intrusive decoder in ONE kernel: MLP + contraction (bf16 tier of BASELINE config 5)
 *   reference: Non-Instrusive/predict_pod_ann.py:60-80 (standardised (mu1, mu2, t) -> model -> Qhat -> U_modes @ Qhat.T)
 *   A workgroup evaluates the MLP for its own 128 (sample, time level) columns -- activations as bf16 in LDS, bf16 MFMA with
 *   float32 accumulate, the rounding points of the PyTorch bf16 module (Linear output -> bf16, activation in float32 -> bf16)
 *   -- and contracts them with U_modes as bg_decode_modes_bf16 does: no activation or coefficient ever crosses HBM.
 *     z1 [B], z2 [B]  standardised mu1, mu2 (float64; rounded to bf16 through float32 in the kernel, as `.to(bfloat16)`)
 *     ztau [Nt]       standardised time levels
 *     layer l (host arrays of n_layers entries; DEVICE pointers inside):
 *       W[l]     [wout[l]][win[l]] bf16 row-major = torch Linear.weight zero padded: win[0] = 16 (the 3 inputs padded),
 *                win[l] = wout[l-1], every wout a multiple of 32 (padding features: zero rows, zero bias), wout[last] = n
 *       bias[l]  [wout[l]] bf16 or NULL;  acts[l] BG_ACT_* after layer l, alphas[l] its ELU alpha
 *   Um [N][n] bf16, out [B][N][Nt] float64.  N a multiple of 32, n a multiple of 32, widths <= 256, n_layers <= 8
 *   (BG_ERR_UNSUPPORTED_N / _R otherwise: run the model in PyTorch and call bg_decode_modes_bf16). */
int bg_decode_mlp_bf16(int N, int n, int B, int Nt, const uint16_t *Um, const double *z1, const double *z2, const double *ztau,
                       int n_layers, const int *win, const int *wout, const uint16_t *const *W, const uint16_t *const *bias,
                       const int *acts, const float *alphas, double *out, void *stream);

/* bg_jacobi_sweep -- n_steps steps of a one-sided (Hestenes) Jacobi SVD sweep, the accurate small core of
 * the snapshot SVD (reference: np.linalg.svd at POD/pod.py:84, build_quadratic_manifold.py:29).
 *   G      [m][ld] row-major: the m rows are orthogonalised in place by plane rotations
 *   J      [m][ld]: receives the same rotations (start from the identity)
 *   pairs  [n_steps][n_pairs][2] int32: disjoint row pairs of every step (round-robin ordering);
 *          an entry < 0 marks a bye
 *   tol    rows p, q are rotated when |g_p . g_q| > tol |g_p| |g_q|
 *   rotations [1] int32: += number of rotations applied (0 after a full sweep = converged)
 * After convergence the row norms of G are the singular values of the input, G[j]/|G[j]| its left
 * singular vectors (as rows), J its right singular vectors (as rows).
 * This is bg_jacobi_sweep_batched with count = 1: one kernel and one launch loop serve both. */
int bg_jacobi_sweep(int m, int ld, double *G, double *J, const int32_t *pairs, int n_steps, int n_pairs,
                    double tol, int32_t *rotations, void *stream);

/* bg_jacobi_sweep_batched -- the sweep on `count` matrices of one size in the launches of one (the per-cluster cores of
 * the local POD builder, burgers_hip/pod.py jacobi_svd_batched): the matrix is the second grid dimension of the one sweep
 * kernel.  Matrix k is G + k * stride and J + k * stride (stride in doubles, >= (m - 1) ld + m); all share m, ld, pairs
 * and tol.
 *   rotations [count] int32: += the rotations applied to matrix k
 * Every matrix comes out bitwise as it does on its own, whatever its batch-mates; one that has converged makes no rotation.
 * count == 0: BG_OK, nothing is touched.  count > 65535 (a grid dimension) or an overlapping stride: BG_ERR_BAD_ARG. */
int bg_jacobi_sweep_batched(int m, int ld, int count, long long stride, double *G, double *J, const int32_t *pairs,
                            int n_steps, int n_pairs, double tol, int32_t *rotations, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_kmeans_assign / bg_kmeans_update -- the two halves of a Lloyd iteration over snapshots in global POD coordinates:
 *   the offline clustering behind the local POD PROM (burgers_hip/pod.py kmeans, build_local_bases; csrc/kmeans.hip).
 *   q        [Ns][m] row-major: the points, q_g = U_global[:, :m]^T u of every snapshot
 *   centres  [C][m]
 *   Limits (bg_kmeans_limits): m <= 64, C <= 64, those of bg_local_rom_limits (BG_ERR_UNSUPPORTED_R beyond them).
 *   Ns < 0, m < 1, C < 1, a negative or NaN overlap, or a null pointer with Ns > 0: BG_ERR_BAD_ARG.  Ns == 0: BG_OK.
 * bg_kmeans_assign: for every point the squared distance to every centre, the first index of the minimum and that minimum,
 *   with the arithmetic of the online pick (bg_local_rom_run: the distance summed in j order by FMA, the first index on ties,
 *   a NaN distance counts as smallest), so a training snapshot is labelled as the time loop would label the same q_g.
 *   overlap  membership factor, >= 0 (read only when member is given)
 *   labels   [Ns] int32, in/out: the labels of the previous pass come in (anything, e.g. -1, before the first)
 *   d2min    [Ns]: the squared distance to the nearest centre
 *   member   [Ns] uint64 or NULL: bit c is set iff c == label or d2[i][c] < overlap * d2min[i]
 *   changed  [1] int32: += the number of points whose label differs from the one passed in (an integer atomic)
 * bg_kmeans_update: centres[c] = mean of the points labelled c; a cluster without points keeps its centre.
 *   centres  [C][m], in/out;  counts [C] int32: the points of every cluster
 *   No floating-point atomics: the sum of a cluster is taken over its points in input order with a fixed grouping of their
 *   ranks within the cluster, so it is bitwise reproducible and does not depend on the other clusters' points.
 *   Ns > INT32_MAX - 1024: BG_ERR_BAD_ARG.
 * --------------------------------------------------------------------------------- */
int bg_kmeans_limits(int *max_m, int *max_clusters);
int bg_kmeans_assign(int Ns, int m, int C, const double *q, const double *centres, double overlap, int32_t *labels,
                     double *d2min, uint64_t *member, int32_t *changed, void *stream);
int bg_kmeans_update(int Ns, int m, int C, const double *q, const int32_t *labels, double *centres, int32_t *counts,
                     void *stream);

/* bg_rbf_eval -- kernel values and gradient factors of the scaled RBF closure of pod_rbf_prom
 *   reference: FEM/fem_burgers.py:160-260 (scaled gaussian / inverse-multiquadric closure and its Jacobian).
 *   qp [B][n] reduced coordinates; x_min, dx [n] input scaling (xs = 2 (qp - x_min)/dx - 1);
 *   XtT [n][Ns] training centres, transposed;  eps shape parameter
 *   phi [B][Ns]     <- k(|xs - Xt_i|)                                            (NULL = skip)
 *   GT  [B][n][Ns]  <- d phi_i / d qp_k  (chain rule through the input scaling included) (NULL = skip)
 * The closure value and Jacobian follow as phi . W and GT . W (one GEMM each). */
int bg_rbf_eval(int B, int n, int Ns, int kind, double eps, const double *qp, const double *x_min,
                const double *dx, const double *XtT, double *phi, double *GT, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_rbf_gram / bg_chol_factor / bg_chol_solve -- the offline fit of the closure bg_rbf_eval and bg_rbf_rom_run evaluate:
 *   the weights W solve (K + ridge I) W = Y, K[i][j] = k(|Xt_i - Xt_j|) over the Ns scaled centres (burgers_hip/pod.py
 *   fit_rbf_weights, build_rbf_closure; csrc/rbf_fit.hip).  All three work in 64 x 64 tiles, mask a ragged last tile
 *   themselves, use no workspace and no floating-point atomics: every element is summed in a fixed order, so the results
 *   are bitwise reproducible and an element's bits depend on its own row and column of tiles alone.
 *   Orders up to bg_chol_max_n() = 16384 (BG_ERR_UNSUPPORTED_R beyond); indices are size_t.
 * bg_rbf_gram: A [Ns][lda] <- the full symmetric kernel matrix plus ridge on the diagonal.
 *   XtT  [n][Ns] scaled centres, centre index fastest (the layout of bg_rbf_eval);  kind BG_RBF_GAUSSIAN or BG_RBF_IMQ
 *   r2 = sum_k d_k^2 by FMA in the order of k, phi as in bg_rbf_eval; the two triangles are equal bit for bit and
 *   A[i][i] = 1 + ridge exactly.  Columns Ns .. lda - 1 are not touched.
 *   Ns < 0, n < 1, lda < Ns, an unknown kind, a negative or non-finite ridge, or a null operand with Ns > 0:
 *   BG_ERR_BAD_ARG.  Ns == 0: BG_OK with nothing launched.
 * bg_chol_factor: A [n][lda] symmetric positive definite, lower triangle <- L with A = L L^T (blocked, right-looking).
 *   The upper triangle is not read and is left as it was.
 *   info [1] device int <- 0, or k + 1 for the first pivot k that is not a positive finite number (LAPACK dpotrf's info);
 *        the launches after that pivot return at once and A holds nothing of use.  Written with a plain store.
 *   n < 0, lda < n or a null pointer with n > 0: BG_ERR_BAD_ARG.  n == 0: BG_OK with nothing launched (info untouched).
 * bg_chol_solve: Bm [n][ldb] <- (L L^T)^-1 Bm in place, nrhs columns, L as bg_chol_factor left it (forward, then backward
 *   substitution in 64-row blocks).  The result of a column does not depend on the other columns of the call.
 *   n or nrhs < 0, lda < n, ldb < nrhs or a null pointer with work to do: BG_ERR_BAD_ARG.  n == 0 or nrhs == 0: BG_OK.
 * --------------------------------------------------------------------------------- */
int bg_chol_max_n(void);
int bg_rbf_gram(int Ns, int n, int kind, double eps, double ridge, const double *XtT, double *A, int lda, void *stream);
int bg_chol_factor(int n, double *A, int lda, int *info, void *stream);
int bg_chol_solve(int n, int nrhs, const double *L, int lda, double *Bm, int ldb, void *stream);

/* ---------------------------------------------------------------------------------
 * bg_nnls_pick / bg_nnls_append / bg_nnls_solve / bg_nnls_residual / bg_nnls_mark -- the steps of the active-set NNLS
 *   (Lawson-Hanson) behind the hyper-reduction row samplings: min |G x - b|, x >= 0, over the columns of G, with a thin QR
 *   of the active columns kept on the device (burgers_hip/pod.py nnls_rows_device follows pod.nnls_rows; csrc/nnls.hip).
 *   The host queues residual, pick, append and solve and reads one bg_nnls_status (64 bytes) per solve; the append and the
 *   solve look at the status the pick left and do nothing unless it says BG_NNLS_GO.
 *   At      [n][ld] the candidate columns of G, each contiguous over its `rows` entries; ld >= rows, ld even, 16-byte aligned
 *   b, res  [rows] right-hand side and current residual (res 16-byte aligned)
 *   Q       [kmax][ld] orthonormal columns in insertion order, 16-byte aligned
 *   R       [kmax][ldr] upper triangular, stored by columns: R[c * ldr + i] is row i of column c, i <= c
 *   z       [kmax] Q^T b;  x [kmax] the weights in insertion order;  order [kmax] int32 the active columns in that order
 *   active, tabu  [n] int32 masks (0 / 1);  w [n] scratch for the gradient;  work [bg_nnls_work_elems(ld)], 16-byte aligned
 *   status  [1] bg_nnls_status on the device, zeroed by the caller before the first pick
 *   Limits (bg_nnls_limits, needs no device): at most max_active = 512 active columns (kmax; the 511 free rows of
 *   bg_hyper_rom_run_wide and one more) out of at most max_cols = 65536 candidates; BG_ERR_UNSUPPORTED_R beyond them.
 *   No floating-point atomics, plain vector stores: every sum runs in an order the shapes fix, so two calls give the same bits.
 * bg_nnls_pick: w[j] = At[j] . res for every column neither active nor tabu (one wave per column, fixed tree), then into
 *   status: pick = the index of the largest w (the lowest index on ties, -1 when every column is masked; At and res must be
 *   finite: a NaN entry of w is not singled out as np.argmax would single it out), w, resnorm = |res|,
 *   rel = resnorm / dnorm (0 for dnorm = 0), fit_done = rel <= tau, and stop = the head of nnls_rows' loop: BG_NNLS_DONE for
 *   fit_done with count >= min_cols, else BG_NNLS_NO_COLUMN for no pick, a non-finite w or (not fit_done and w <= 0), else
 *   BG_NNLS_FULL for count + 1 > max_cols, else BG_NNLS_GO; dependent, accepted and pick_active are cleared, p0 = count.
 *   rows, n, min_cols or max_cols < 0, ld < rows, an odd ld, a negative or NaN dnorm or tau, a null or misaligned operand
 *   with n > 0: BG_ERR_BAD_ARG.  n == 0: BG_OK with nothing launched.  n > max_cols or max_cols > max_active: _UNSUPPORTED_R.
 * bg_nnls_append: v = At[j] with j = status.pick (rebuild = 0) or j = order[k] (rebuild = 1: the repair after a drop);
 *   h = Q[:k] v, v -= Q[:k]^T h, twice (classical Gram-Schmidt, the sums over the columns in insertion order).  Then
 *   R[:k, k] = h1 + h2, R[k, k] = |v|, Q[k] = v / |v|, z[k] = Q[k] . b, active[j] = 1, status.count = k + 1, and for
 *   rebuild = 0 order[k] = j, x[k] = 0.  status.ratio = |v| / |At[j]|.  If |v| <= BG_NNLS_DEPENDENT_MULTIPLE * 2^-52 * |At[j]|
 *   the column is numerically dependent on the active ones: nothing is appended, tabu[j] = 1 and status.dependent = 1
 *   (with rebuild = 1 that cannot be: status.stop = BG_NNLS_FAULT).
 *   rows, k or ldr < 0, ld < rows, ldr <= k, an odd ld, a null or misaligned operand with rows > 0: BG_ERR_BAD_ARG.
 *   rows == 0: BG_OK with nothing launched.  k >= max_active: BG_ERR_UNSUPPORTED_R.
 * bg_nnls_solve: one workgroup back-substitutes R[:k, :k] s = z[:k].  Every s > 0: x = s, status.accepted = 1.  Otherwise
 *   nnls_rows' step: ratio = x / (x - s) over the entries with s <= 0 (0 for x = 0, also where s = 0 makes that 0 / 0), alpha its minimum, x = max(x + alpha (s - x), 0) with
 *   the entries at ratio <= alpha set to 0 (rounded as the host rounds them: no fused multiply-add); every entry now <= 0
 *   leaves: active cleared, order and x compacted, status.accepted = 0, p0 = the first position that left, count = what
 *   stays.  Q, R and z are valid up to p0; the caller appends order[p0 .. count) again with rebuild = 1 and solves again.
 *   status.pick_active says whether the pick is among the columns that stay.  A k that is not status.count: BG_NNLS_FAULT.
 *   k < 0, ldr < k or a null operand with k > 0: BG_ERR_BAD_ARG.  k == 0: BG_OK with nothing launched.
 * bg_nnls_residual: res = b - sum_c x[c] At[order[c]] over c < k in insertion order (the columns themselves, not b - Q z).
 *   rows or k < 0, ld < rows, a null operand with work to do: BG_ERR_BAD_ARG.  rows == 0: BG_OK with nothing launched.
 * bg_nnls_mark: tabu[j] = value (0 / 1), or every entry for j < 0.  n < 0, j >= n, a null tabu with n > 0: BG_ERR_BAD_ARG.
 * --------------------------------------------------------------------------------- */
#define BG_NNLS_DEPENDENT_MULTIPLE 1048576.0   /* 2^20: |v| / |At[j]| <= 2.3e-10 counts as dependent */
enum { BG_NNLS_GO = 0, BG_NNLS_DONE = 1, BG_NNLS_NO_COLUMN = 2, BG_NNLS_FULL = 3, BG_NNLS_FAULT = 4 };
typedef struct bg_nnls_status {
    int32_t stop, pick, fit_done, dependent, accepted, p0, count, pick_active;
    double w, resnorm, rel, ratio;
} bg_nnls_status;
int bg_nnls_limits(int *max_active, int *max_cols);
long long bg_nnls_work_elems(int ld);
int bg_nnls_pick(int rows, int n, int ld, const double *At, const double *res, const int32_t *active, const int32_t *tabu,
                 double dnorm, double tau, int min_cols, int max_cols, double *w, bg_nnls_status *status, void *stream);
int bg_nnls_append(int rows, int ld, int k, int rebuild, const double *At, const double *b, double *Q, double *R, int ldr,
                   double *z, double *x, int32_t *order, int32_t *active, int32_t *tabu, double *work,
                   bg_nnls_status *status, void *stream);
int bg_nnls_solve(int k, const double *R, int ldr, const double *z, double *x, int32_t *order, int32_t *active,
                  bg_nnls_status *status, void *stream);
int bg_nnls_residual(int rows, int ld, int k, const double *At, const double *b, const double *x, const int32_t *order,
                     double *res, void *stream);
int bg_nnls_mark(int n, int32_t *tabu, int j, int value, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BURGERS_HIP_H */
