"""The NumPy / SciPy references of the POD-RBF builder tests (test_rbf_builder_abi.py, test_rbf_builder_gpu.py): the fit rule
of tests/golden/make_golden.py fx_rbf, the backward error and its gate, a block-64 right-looking Cholesky as a second
summation order, the spread between two reference solvers, and the input makers.  Nothing here imports the code under test."""
import functools

import numpy as np
import scipy.linalg

from conftest import load_golden

KERNELS = (("gaussian", 2.0), ("imq", 1.5))                # the fixture's kernels and shape parameters


def kernel_matrix(Xs, eps, kernel, ridge=0.0):
    """k(eps |x_i - x_j|) + ridge I, r^2 summed over the coordinates in their order."""
    r2 = np.zeros((len(Xs), len(Xs)))
    for k in range(Xs.shape[1]):
        d = Xs[:, None, k] - Xs[None, :, k]
        r2 += d * d
    K = np.exp(-eps * eps * r2) if kernel == "gaussian" else 1.0 / np.sqrt(1.0 + eps * eps * r2)
    K[np.diag_indices(len(Xs))] = 1.0 + ridge
    return K


def backward_error(A, W, Y):
    """|A W - Y|_F / (|A|_2 |W|_F + |Y|_F)."""
    W, Y = W.reshape(len(A), -1), Y.reshape(len(A), -1)
    return np.linalg.norm(A @ W - Y) / (np.linalg.norm(A, 2) * np.linalg.norm(W) + np.linalg.norm(Y))


def gate(n):
    """The Cholesky backward-error bound at order n: 4 n 2^-53."""
    return 4.0 * n * 2.0 ** -53


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def lu_solve(A, Y):
    return np.linalg.solve(A, Y)


def chol_solve(A, Y):
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), Y)


def spread(A, Y):
    """s: the relative difference between SciPy's Cholesky solve and NumPy's LU solve of A W = Y."""
    return rel(chol_solve(A, Y), lu_solve(A, Y))


def block_cholesky(A, nb=64):
    """Right-looking blocked lower Cholesky: factor the diagonal block, solve the panel below, update the trailing matrix."""
    L = np.tril(A).astype(np.float64)
    n = len(A)
    for k in range(0, n, nb):
        e = min(k + nb, n)
        L[k:e, k:e] = np.linalg.cholesky(L[k:e, k:e] + np.tril(L[k:e, k:e], -1).T)
        if e < n:
            L[e:, k:e] = scipy.linalg.solve_triangular(L[k:e, k:e], L[e:, k:e].T, lower=True).T
            L[e:, e:] -= np.tril(L[e:, k:e] @ L[e:, k:e].T)
    return L


def spd_matrix(n, seed=0):
    """I + G G^T / n, G standard normal: condition below 10."""
    G = np.random.default_rng([seed, n]).normal(size=(n, n))
    return np.eye(n) + G @ G.T / n


def rhs(n, nrhs, seed=1):
    return np.random.default_rng([seed, n, nrhs]).normal(size=(n, nrhs))


def centre_rows(centres, Ns_all):
    if centres is None:
        return np.arange(Ns_all)
    if np.ndim(centres) == 0:
        return np.linspace(0, Ns_all - 1, int(centres)).astype(int)
    return np.asarray(centres, dtype=np.int64)


def fit_rule(S, U, n, nbar, eps, kernel, ridge, centres=None, max_cond=None):
    """The rule of fx_rbf on snapshots S with the singular vectors U given: a dict with the bases, the ranges over all
    snapshots, the centre rows, the scaled data, the ridge matrix A, and the LU and Cholesky solutions W_lu, W_chol."""
    U_p, U_s = U[:, :n], U[:, n:n + nbar]
    Q, Qb = (U_p.T @ S).T, (U_s.T @ S).T
    x_min, x_max, y_min, y_max = Q.min(0), Q.max(0), Qb.min(0), Qb.max(0)
    dx, dy = x_max - x_min, y_max - y_min
    dx[dx < 1e-15] = 1.0
    dy[dy < 1e-15] = 1.0
    idx = centre_rows(centres, S.shape[1])
    Xs = 2.0 * (Q[idx] - x_min) / dx - 1.0
    Ys = 2.0 * (Qb[idx] - y_min) / dy - 1.0
    A = kernel_matrix(Xs, eps, kernel, ridge)
    if max_cond is not None:
        assert np.linalg.cond(A) <= max_cond, np.linalg.cond(A)
    return dict(U_p=U_p, U_s=U_s, Q=Q, Qb=Qb, x_min=x_min, x_max=x_max, y_min=y_min, y_max=y_max, idx=idx, Xs=Xs, Ys=Ys, A=A,
                W_lu=lu_solve(A, Ys), W_chol=chol_solve(A, Ys))


def closure_value(q, Xs, W, eps, kernel, x_min, x_max, y_min, y_max):
    """The scaled closure at the rows of q (B, n): unscale(k(|scale(q) - x_i|) W)."""
    dx, dy = x_max - x_min, y_max - y_min
    dx[dx < 1e-15] = 1.0
    dy[dy < 1e-15] = 1.0
    xs = 2.0 * (q - x_min) / dx - 1.0
    r2 = ((xs[:, None, :] - Xs[None, :, :]) ** 2).sum(2)
    phi = np.exp(-eps * eps * r2) if kernel == "gaussian" else 1.0 / np.sqrt(1.0 + eps * eps * r2)
    return (phi @ W + 1.0) * (0.5 * dy) + y_min


@functools.lru_cache(maxsize=None)
def builder_snapshots():
    """(S, U): every sixth column of loop_cases.training_snapshots(96, 0.05) (302 snapshots) and their singular vectors."""
    from loop_cases import training_snapshots
    S = np.ascontiguousarray(training_snapshots(96, 0.05)[1][:, ::6])
    return S, np.linalg.svd(S, full_matrices=False)[0]


BUILDER = dict(n=8, nbar=20)
CENTRES = (None, 93, tuple(range(3, 300, 2)))               # every snapshot, the fixture's subsampling, an index array


@functools.lru_cache(maxsize=None)
def builder_case(kernel, eps, ridge, centres):
    """fit_rule on builder_snapshots, computed once per case and left as it is.  At ridge 1e-3 the condition is asserted to
    be at most 1e6, so that LU and Cholesky weights agree far inside 1e-10."""
    S, U = builder_snapshots()
    return fit_rule(S, U, BUILDER["n"], BUILDER["nbar"], eps, kernel, ridge, None if centres is None else
                    (centres if np.ndim(centres) == 0 else np.asarray(centres)), max_cond=1e6 if ridge >= 1e-3 else None)


@functools.lru_cache(maxsize=None)
def golden_system(kernel):
    """(g, Xs, eps, A, Ys, W_golden): the fixture's scaled centres, A = K + 1e-8 I and Ys := A W_golden."""
    g = load_golden("rbf_n17.npz")
    Xs, eps, W = np.ascontiguousarray(g["X_train"]), float(g["eps_" + kernel]), np.ascontiguousarray(g["W_" + kernel])
    A = kernel_matrix(Xs, eps, kernel, 1e-8)
    return g, Xs, eps, A, A @ W, W
