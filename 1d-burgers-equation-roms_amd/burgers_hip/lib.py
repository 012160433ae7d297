"""ctypes binding of libburgers_hip.so (the C ABI declared in include/burgers_hip.h).

There is no CPU fallback: if the shared object is missing, or a call is made without a
HIP device, this module raises.  torch is imported first so that the process uses one
HIP runtime (torch's) for device memory, streams and our kernels alike.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch  # noqa: F401  (must precede the CDLL load: one libamdhip64 per process)

from . import build as _build

c_double_p = ctypes.c_void_p      # raw device pointers travel as integers
c_int_p = ctypes.c_void_p

BG_OK = 0
BG_ERR_BAD_ARG = -1
BG_ERR_UNSUPPORTED_N = -2
BG_ERR_NONUNIFORM = -3
BG_ERR_LAUNCH = -4
BG_ERR_UNSUPPORTED_R = -5
BG_ERR_PROJECTION = -6
BG_ERR_WORKSPACE = -7
BG_PROJ_GALERKIN, BG_PROJ_LSPG = 0, 1
BG_FLAG_HIT_CAP, BG_FLAG_NONFINITE = 1, 2
BG_OPT_SUPG, BG_OPT_NONUNIFORM, BG_OPT_W_COLMAJOR, BG_OPT_MFMA_16X16, BG_OPT_FORCE_PIVOTED, BG_OPT_NO_TANGENT_REUSE = 1, 2, 4, 8, 16, 32
BG_OPT_FOM_WIDE, BG_OPT_FOM_WAVE, BG_OPT_PIVOT_ON_DEVICE = 64, 128, 256
BG_ACT_NONE, BG_ACT_ELU, BG_ACT_RELU, BG_ACT_TANH = 0, 1, 2, 3
BG_COUNTER_SLOTS, BG_COUNTER_STRIDE = 16, 32
BG_RBF_GAUSSIAN, BG_RBF_IMQ = 0, 1
BG_INFO_NEEDS_PIVOTING = -1
BG_NNLS_GO, BG_NNLS_DONE, BG_NNLS_NO_COLUMN, BG_NNLS_FULL, BG_NNLS_FAULT = 0, 1, 2, 3, 4
# bg_nnls_status (include/burgers_hip.h): 64 bytes
NNLS_STATUS = np.dtype([(k, np.int32) for k in ("stop", "pick", "fit_done", "dependent", "accepted", "p0", "count", "pick_active")] +
                       [(k, np.float64) for k in ("w", "resnorm", "rel", "ratio")])

# Fragments of the argument list the device-side time loops share (include/burgers_hip.h), in the order _loop puts them
_LOOP_BATCH = [c_double_p] * 3                                              # u0, mu1, mu2
_LOOP_STEP = [ctypes.c_double] * 3 + [ctypes.c_int] * 2                      # dt, E, tol, max_it, options
_LOOP_OUT = [c_double_p] + [c_int_p] * 4 + [ctypes.c_void_p]                 # hist, iters, flags, info, order, stream
_LOOP_OUT_CLUSTERS = [c_double_p] + [c_int_p] * 5 + [ctypes.c_void_p]        # ... info, clusters, order, stream
_ANN_MLP = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
            ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)]   # layers, widths, wt, bias, acts, alphas: HOST arrays
_LOCAL_OPERANDS = [c_double_p, c_int_p, c_double_p, c_double_p]              # stack, widths, UgT, centres


def _loop(ints, operands, after_batch=(), workspace=(), out=_LOOP_OUT):
    """(restype, argtypes) of a device-side time loop: ``ints`` leading ints, x, ``operands``, the batch, ``after_batch``
    (bg_ann_rom_run's MLP), the step, ``workspace`` (bg_rom_run_blocked's work, slots), the outputs."""
    return (ctypes.c_int, [ctypes.c_int] * ints + [c_double_p] + list(operands) + _LOOP_BATCH + list(after_batch) +
            _LOOP_STEP + list(workspace) + out)


_SIGNATURES = {
    # name: (restype, argtypes)
    "bg_abi_version": (ctypes.c_int, []),
    "bg_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "bg_last_hip_error": (ctypes.c_int, []),
    "bg_fom_max_n": (ctypes.c_int, []),
    "bg_fom_run": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p,
                                  c_double_p, c_double_p, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_double, ctypes.c_int, ctypes.c_int, c_double_p, c_int_p,
                                  c_int_p, ctypes.c_void_p]),
    "bg_fom_run_traced": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p,
                                         c_double_p, c_double_p, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_double, ctypes.c_int, ctypes.c_int, c_double_p, c_int_p,
                                         c_int_p, c_double_p, ctypes.c_void_p]),
    "bg_fom_assemble": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                       c_double_p, c_double_p, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p,
                                       ctypes.c_void_p]),
    "bg_tridiag_solve": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                        c_double_p, c_double_p, ctypes.c_void_p]),
    "bg_transpose_batched": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                                            c_double_p, ctypes.c_void_p]),
    "bg_fd_run": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                 c_double_p, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_double_p, c_int_p,
                                 c_int_p, ctypes.c_void_p]),
    "bg_rom_max_n": (ctypes.c_int, []),
    "bg_rom_max_r": (ctypes.c_int, []),
    "bg_forcing_setup": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_double,
                                        ctypes.c_int, c_double_p, c_double_p, ctypes.c_void_p]),
    "bg_mass_rhs": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p, ctypes.c_int,
                                   c_double_p, ctypes.c_void_p]),
    "bg_rom_reduce": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                                     c_double_p, ctypes.c_longlong, c_double_p, c_double_p, c_double_p,
                                     c_double_p, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_int_p,
                                     c_double_p, c_double_p, c_double_p, ctypes.c_void_p]),
    "bg_rom_reduce_indexed": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                                             c_double_p, ctypes.c_longlong, c_int_p, c_double_p, c_double_p, c_double_p,
                                             c_double_p, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_int_p,
                                             c_double_p, c_double_p, c_double_p, ctypes.c_void_p]),
    "bg_rom_reduce_lifted": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                                            c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                            c_double_p, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_int_p,
                                            c_double_p, c_double_p, c_double_p, ctypes.c_void_p]),
    "bg_rom_run_max_r": (ctypes.c_int, []),
    "bg_rom_run": _loop(5, [c_double_p]),
    "bg_quad_rom_max_n": (ctypes.c_int, []),
    "bg_quad_rom_h3f_elems": (ctypes.c_longlong, [ctypes.c_int]),
    "bg_quad_rom_phif_elems": (ctypes.c_longlong, [ctypes.c_int]),
    "bg_quad_rom_run": _loop(5, [c_double_p] * 3),
    "bg_quad_rom_run_long_max_n": (ctypes.c_int, []),
    "bg_quad_rom_run_long_max_r": (ctypes.c_int, []),
    "bg_quad_rom_run_long_workgroups_per_cu": (ctypes.c_int, []),
    "bg_quad_rom_run_long_phit_elems": (ctypes.c_longlong, [ctypes.c_int]),
    "bg_quad_rom_run_long_phif_elems": (ctypes.c_longlong, [ctypes.c_int]),
    "bg_quad_rom_run_long_h3f_elems": (ctypes.c_longlong, [ctypes.c_int]),
    "bg_quad_rom_run_long": _loop(5, [c_double_p] * 3),
    "bg_hyper_quad_rom_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 3),
    "bg_hyper_quad_rom_workgroups_per_cu": (ctypes.c_int, [ctypes.c_int]),
    "bg_hyper_quad_rom_phif_elems": (ctypes.c_longlong, [ctypes.c_int]),
    "bg_hyper_quad_rom_h3f_elems": (ctypes.c_longlong, [ctypes.c_int]),
    # N, B, n, m, nodes, nsteps, projection, xn, then node, pos, xi, Phif, H3f, q0, the batch (u0n for u0), ..., qhist for hist
    "bg_hyper_quad_rom_run": _loop(7, [c_int_p, c_int_p] + [c_double_p] * 4),
    "bg_rom_run_wide_max_r": (ctypes.c_int, []),
    "bg_rom_run_wide_phi_elems": (ctypes.c_longlong, [ctypes.c_int]),
    "bg_rom_run_wide": _loop(5, [c_double_p]),
    "bg_rom_run_blocked_max_r": (ctypes.c_int, []),
    "bg_rom_run_blocked_phi_elems": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    "bg_rom_run_blocked_work_elems": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    "bg_rom_run_blocked": _loop(5, [c_double_p], workspace=[c_double_p, ctypes.c_int]),
    "bg_rom_run_long_max_n": (ctypes.c_int, []),
    "bg_rom_run_long_max_r": (ctypes.c_int, []),
    "bg_rom_run_long_workgroups_per_cu": (ctypes.c_int, []),
    "bg_rom_run_long_phi_elems": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    "bg_rom_run_long": _loop(5, [c_double_p]),
    "bg_hyper_rom_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 2),
    "bg_hyper_rom_table_elems": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    # N, B, r, m, nsteps, projection, rows, xi, xs, PhiS, q0, u0s, mu1, mu2, the step, the outputs (qhist for hist)
    "bg_hyper_rom_run": (ctypes.c_int, [ctypes.c_int] * 6 + [c_int_p] + [c_double_p] * 7 + _LOOP_STEP + _LOOP_OUT),
    "bg_hyper_rom_wide_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 2),
    "bg_hyper_rom_wide_table_elems": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    "bg_hyper_rom_run_wide": (ctypes.c_int, [ctypes.c_int] * 6 + [c_int_p] + [c_double_p] * 7 + _LOOP_STEP + _LOOP_OUT),      # as bg_hyper_rom_run
    "bg_hyper_rom_blocked_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 2),
    "bg_hyper_rom_blocked_table_elems": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    "bg_hyper_rom_blocked_work_elems": (ctypes.c_longlong, [ctypes.c_int]),
    "bg_hyper_rom_run_blocked": (ctypes.c_int, [ctypes.c_int] * 6 + [c_int_p] + [c_double_p] * 7 + _LOOP_STEP +
                                 [c_double_p, ctypes.c_int] + _LOOP_OUT),      # as bg_hyper_rom_run, with work and slots before qhist
    # B, n, A, b, x, piv (int32 or null), info (int32), stream
    "bg_wide_solve_pivoted": (ctypes.c_int, [ctypes.c_int] * 2 + [c_double_p] * 3 + [c_int_p] * 2 + [ctypes.c_void_p]),
    "bg_hyper_ann_rom_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 6),
    "bg_hyper_ann_rom_workgroups_per_cu": (ctypes.c_int, [ctypes.c_int]),
    # N, B, n, nbar, m, nodes, nsteps, projection, node, xn, pos, xi, UTn, q0, u0n, mu1, mu2, the MLP, the step, qhist, qshist, ...
    "bg_hyper_ann_rom_run": (ctypes.c_int, [ctypes.c_int] * 8 + [c_int_p, c_double_p, c_int_p] + [c_double_p] * 6 + _ANN_MLP +
                             _LOOP_STEP + [c_double_p] + _LOOP_OUT),
    "bg_hyper_ann_rom_wide_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 6),
    "bg_hyper_ann_rom_wide_workgroups_per_cu": (ctypes.c_int, [ctypes.c_int]),
    "bg_hyper_ann_rom_wide_ut_ld": (ctypes.c_int, [ctypes.c_int]),
    "bg_hyper_ann_rom_run_wide": (ctypes.c_int, [ctypes.c_int] * 8 + [c_int_p, c_double_p, c_int_p] + [c_double_p] * 6 + _ANN_MLP +
                                  _LOOP_STEP + [c_double_p] + _LOOP_OUT),      # as bg_hyper_ann_rom_run
    "bg_hyper_rbf_rom_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 5),
    "bg_hyper_rbf_rom_workgroups_per_cu": (ctypes.c_int, [ctypes.c_int]),
    "bg_hyper_rbf_rom_ut_ld": (ctypes.c_int, [ctypes.c_int]),
    # N, B, n, nbar, Ns, m, nodes, nsteps, projection, kind, node, xn, pos, xi, UTn, XtT, Wd, bias, x_min, dx, eps, q0, u0n, mu1,
    # mu2, the step, qhist, qshist, ...
    "bg_hyper_rbf_rom_run": (ctypes.c_int, [ctypes.c_int] * 10 + [c_int_p, c_double_p, c_int_p] + [c_double_p] * 7 +
                             [ctypes.c_double] + [c_double_p] * 4 + _LOOP_STEP + [c_double_p] + _LOOP_OUT),
    "bg_rom_run_long_wide_max_n": (ctypes.c_int, []),
    "bg_rom_run_long_wide_max_r": (ctypes.c_int, []),
    "bg_rom_run_long_wide_phi_elems": (ctypes.c_longlong, [ctypes.c_int]),
    "bg_rom_run_long_wide": _loop(5, [c_double_p]),
    "bg_rom_lift": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                   c_int_p, c_double_p, ctypes.c_void_p]),
    "bg_quad_features": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_double_p, c_int_p, c_int_p, c_double_p, ctypes.c_void_p]),
    "bg_rom_frag_elems": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    "bg_rom_frag_pad": (ctypes.c_int, [ctypes.c_int]),
    "bg_quad_tangent": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                       c_int_p, c_double_p, ctypes.c_void_p]),
    "bg_rom_reduce_frag": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                                          c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                          ctypes.c_double, ctypes.c_double, ctypes.c_int, c_int_p, c_double_p,
                                          c_double_p, c_double_p, ctypes.c_void_p]),
    "bg_lu_solve_update": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int,
                                          c_double_p, c_double_p, c_double_p, ctypes.c_double, ctypes.c_int,
                                          c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, ctypes.c_void_p]),
    "bg_lu_solve": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_double,
                                   c_int_p, c_double_p, c_int_p, ctypes.c_void_p]),
    "bg_jacobi_sweep": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_int_p, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_double, c_int_p, ctypes.c_void_p]),
    "bg_jacobi_sweep_batched": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, c_double_p, c_double_p,
                                               c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_int_p, ctypes.c_void_p]),
    "bg_kmeans_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 2),
    # Ns, m, C, q, centres, overlap, labels (int32), d2min, member (uint64 or null), changed (int32), stream
    "bg_kmeans_assign": (ctypes.c_int, [ctypes.c_int] * 3 + [c_double_p, c_double_p, ctypes.c_double, c_int_p, c_double_p,
                                        ctypes.c_void_p, c_int_p, ctypes.c_void_p]),
    # Ns, m, C, q, labels, centres (in/out), counts (int32), stream
    "bg_kmeans_update": (ctypes.c_int, [ctypes.c_int] * 3 + [c_double_p, c_int_p, c_double_p, c_int_p, ctypes.c_void_p]),
    "bg_rbf_eval": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_double_p,
                                   c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, ctypes.c_void_p]),
    "bg_chol_max_n": (ctypes.c_int, []),
    # Ns, n, kind, eps, ridge, XtT, A, lda, stream
    "bg_rbf_gram": (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_double] * 2 + [c_double_p, c_double_p, ctypes.c_int, ctypes.c_void_p]),
    # n, A (in/out), lda, info (int32), stream
    "bg_chol_factor": (ctypes.c_int, [ctypes.c_int, c_double_p, ctypes.c_int, c_int_p, ctypes.c_void_p]),
    # n, nrhs, L, lda, B (in/out), ldb, stream
    "bg_chol_solve": (ctypes.c_int, [ctypes.c_int] * 2 + [c_double_p, ctypes.c_int, c_double_p, ctypes.c_int, ctypes.c_void_p]),
    "bg_nnls_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 2),
    "bg_nnls_work_elems": (ctypes.c_longlong, [ctypes.c_int]),
    # rows, n, ld, At, res, active, tabu (int32), dnorm, tau, min_cols, max_cols, w, status, stream
    "bg_nnls_pick": (ctypes.c_int, [ctypes.c_int] * 3 + [c_double_p] * 2 + [c_int_p] * 2 + [ctypes.c_double] * 2 +
                     [ctypes.c_int] * 2 + [c_double_p, ctypes.c_void_p, ctypes.c_void_p]),
    # rows, ld, k, rebuild, At, b, Q, R, ldr, z, x, order, active, tabu (int32), work, status, stream
    "bg_nnls_append": (ctypes.c_int, [ctypes.c_int] * 4 + [c_double_p] * 4 + [ctypes.c_int] + [c_double_p] * 2 + [c_int_p] * 3 +
                       [c_double_p, ctypes.c_void_p, ctypes.c_void_p]),
    # k, R, ldr, z, x, order, active (int32), status, stream
    "bg_nnls_solve": (ctypes.c_int, [ctypes.c_int, c_double_p, ctypes.c_int] + [c_double_p] * 2 + [c_int_p] * 2 +
                      [ctypes.c_void_p, ctypes.c_void_p]),
    # rows, ld, k, At, b, x, order (int32), res, stream
    "bg_nnls_residual": (ctypes.c_int, [ctypes.c_int] * 3 + [c_double_p] * 3 + [c_int_p, c_double_p, ctypes.c_void_p]),
    # n, tabu (int32), j, value, stream
    "bg_nnls_mark": (ctypes.c_int, [ctypes.c_int, c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "bg_mlp_act_jvp": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int, ctypes.c_float, ctypes.c_void_p]),
    "bg_decode_modes_bf16": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_void_p, c_double_p, ctypes.c_void_p]),
    # win / wout / acts (int[]), W / bias (void*[]) and alphas (float[]) are HOST arrays built by the caller
    "bg_decode_mlp_bf16": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          c_double_p, c_double_p, c_double_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_float), c_double_p, ctypes.c_void_p]),
    "bg_ann_rom_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 4),
    "bg_ann_rom_run": _loop(6, [c_double_p], after_batch=_ANN_MLP),
    "bg_ann_rom_run_wide_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 4),
    "bg_ann_rom_run_wide": _loop(6, [c_double_p], after_batch=_ANN_MLP),
    "bg_rbf_rom_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 3),
    "bg_rbf_rom_run": _loop(8, [c_double_p] * 6 + [ctypes.c_double]),
    "bg_rbf_rom_run_long_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 4),
    "bg_rbf_rom_run_long": _loop(8, [c_double_p] * 6 + [ctypes.c_double]),
    "bg_local_rom_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 3),
    "bg_local_rom_run": _loop(7, _LOCAL_OPERANDS, out=_LOOP_OUT_CLUSTERS),
    "bg_local_rom_run_long_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 4),
    "bg_local_rom_run_long_bases_elems": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    "bg_local_rom_run_long": _loop(7, _LOCAL_OPERANDS, out=_LOOP_OUT_CLUSTERS),
    "bg_hyper_local_rom_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)] * 4),
    "bg_hyper_local_rom_table_elems": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    # N, B, C, rmax, mg, m, nsteps, projection, rows, xi, xs, PhiS, widths, trans, pick, centres, qg0, pu0, u0s, mu1, mu2, the step,
    # the outputs with clusters (qhist for hist)
    "bg_hyper_local_rom_run": (ctypes.c_int, [ctypes.c_int] * 8 + [c_int_p] + [c_double_p] * 3 + [c_int_p] + [c_double_p] * 8 +
                               _LOOP_STEP + _LOOP_OUT_CLUSTERS),
}

_lib = None


class BurgersHipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = _lib.bg_strerror(code).decode() if _lib is not None else str(code)
        extra = f" (hipError {_lib.bg_last_hip_error()})" if code == BG_ERR_LAUNCH and _lib else ""
        super().__init__(f"{where}: {msg}{extra} [code {code}]")


def library_path():
    # BG_LIB_PATH: load an experimental build of the same ABI (kernel A/B timing); default in-tree
    return os.environ.get("BG_LIB_PATH") or _build.LIB_PATH


def load(build_if_missing=False):
    """Load the shared object and bind every declared symbol.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        if build_if_missing:
            _build.build_library()
        else:
            raise ImportError(
                f"{path} is missing: build it with `python __graft_entry__.py build` "
                "(there is no CPU fallback for the HIP path)")
    L = ctypes.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if L.bg_abi_version() != 1:
        raise ImportError(f"ABI mismatch: library reports {L.bg_abi_version()}, binding expects 1")
    _lib = L
    return L


def declared_symbols():
    return sorted(_SIGNATURES)


def check(code, where):
    if code != BG_OK:
        raise BurgersHipError(code, where)


def limits(name, count):
    """The ``count`` ints a ``*_limits`` entry point reports through its out-parameters.  Needs no device."""
    out = [ctypes.c_int() for _ in range(count)]
    check(getattr(load(), name)(*[ctypes.byref(v) for v in out]), name)
    return tuple(v.value for v in out)


def require_device(device=None):
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: the Burgers HIP kernels need an MI355X (no CPU fallback)")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:      # 'cuda' -> 'cuda:<current>': tensors report an indexed device
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


PINNED_MIN_BYTES = 1 << 20


def to_host(t):
    """Device tensor -> numpy array.  Results of a sweep are gigabytes, and a copy into fresh
    pageable memory runs far below the PCIe rate, so anything over 1 MiB goes through torch's
    caching pinned-host allocator: the returned ndarray is a view of the pinned block, which
    returns to that cache when the array is dropped.  BG_PINNED_RESULTS=0 keeps pageable memory."""
    t = t.detach()
    if (t.is_cuda and t.numel() * t.element_size() >= PINNED_MIN_BYTES
            and os.environ.get("BG_PINNED_RESULTS", "1") != "0"):
        try:
            host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        except RuntimeError:            # pinning refused (ulimit, fragmentation): pageable copy
            return t.cpu().numpy()
        host.copy_(t, non_blocking=True)
        torch.cuda.current_stream(t.device).synchronize()
        return host.numpy()
    return t.cpu().numpy()


def mesh_options(X, supg=True):
    """Option bits for the assembly-carrying entry points: SUPG on/off, uniform/non-uniform mesh."""
    return (BG_OPT_SUPG if supg else 0) | (0 if mesh_is_uniform(X) else BG_OPT_NONUNIFORM)


def mesh_is_uniform(X, rtol=1e-9):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 1 or len(X) < 2:
        return False
    d = np.diff(X)
    h = (X[-1] - X[0]) / (len(X) - 1)
    return bool(h > 0 and np.all(np.abs(d - h) <= rtol * abs(h)))
