"""NumPy model of the pivoting rule of wide_solve_pivoted (csrc/rom_wide_device.hpp): Gauss-Jordan elimination with partial
pivoting as an implicit permutation.  The pivot of column k is the FIRST maximum of |a| among the rows not yet used as a
pivot; no row moves; every other row, used or not, is eliminated against it; x_k = y[p_k] / a[p_k][k].  A column without a
non-zero candidate ends the solve with info = k + 1 (LAPACK's info of an exactly singular matrix)."""
import numpy as np


def solve_pivoted(A, b):
    """(x, piv, info): piv[k] is the row used for column k.  info = 0, or k + 1 with x NaN and piv[k:] = -1."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    W = np.concatenate([A, np.asarray(b, dtype=np.float64).reshape(n, 1)], axis=1)
    used = np.zeros(n, dtype=bool)
    piv = np.full(n, -1, dtype=np.int64)
    for k in range(n):
        cand = np.where(used, -1.0, np.abs(W[:, k]))
        p = int(np.argmax(cand))                # the first maximum: the lowest row wins ties
        if cand[p] == 0.0:
            return np.full(n, np.nan), piv, k + 1
        m = W[:, k] / W[p, k]
        m[p] = 0.0
        W[:, k + 1:] -= np.outer(m, W[p, k + 1:])      # columns up to k are done with: only a[p_k][k] is read again
        used[p] = True
        piv[k] = p
    return W[piv, n] / W[piv, np.arange(n)], piv, 0


def lapack_pivot_rows(ipiv):
    """The row of the original matrix that getrf's interchanges ``ipiv`` (0-based, scipy.linalg.lu_factor) bring to place k."""
    perm = np.arange(len(ipiv))
    for k, p in enumerate(ipiv):
        perm[[k, p]] = perm[[p, k]]
    return perm


def backward_error(A, x, b):
    """Normwise backward error |A x - b| / (|A|_2 |x| + |b|)."""
    return float(np.linalg.norm(A @ x - b) / (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b)))


SIZES = (1, 4, 41, 64, 65, 77, 96)


def gaussian_systems(n, count=8, seed=5):
    """``count`` Gaussian systems of n unknowns from default_rng(seed), drawn size by size in the order of SIZES."""
    rng = np.random.default_rng(seed)
    for size in SIZES:
        A, b = rng.standard_normal((count, size, size)), rng.standard_normal((count, size))
        if size == n:
            return A, b
    raise ValueError(n)


def scaled_permutation(n, seed=3):
    """(A, b, perm): A[perm[k], k] = s_k with 1e-3 <= |s_k| <= 1e3 and zero elsewhere, so the pivot row of column k is perm[k]."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    A = np.zeros((n, n))
    A[perm, np.arange(n)] = 10.0 ** rng.uniform(-3, 3, n) * rng.choice([-1.0, 1.0], n)
    return A, rng.standard_normal(n), perm
