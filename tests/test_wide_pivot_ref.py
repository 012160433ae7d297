"""The NumPy model of wide_solve_pivoted's pivoting rule (tests/wide_pivot_ref.py) against LAPACK: the same pivot rows as
getrf, a backward error beside numpy.linalg.solve's, a row-scaled permutation, and info of an exactly singular matrix."""
import numpy as np
import pytest

from wide_pivot_ref import SIZES, backward_error, gaussian_systems, lapack_pivot_rows, scaled_permutation, solve_pivoted


@pytest.mark.parametrize("n", SIZES)
def test_model_picks_lapacks_pivot_rows_on_gaussian_systems(n):
    from scipy.linalg import lu_factor
    A, b = gaussian_systems(n)
    assert A.shape == (8, n, n)
    worst, ref = 0.0, 0.0
    for Ab, bb in zip(A, b):
        x, piv, info = solve_pivoted(Ab, bb)
        assert info == 0
        assert np.array_equal(piv, lapack_pivot_rows(lu_factor(Ab)[1]))
        worst = max(worst, backward_error(Ab, x, bb))
        ref = max(ref, backward_error(Ab, np.linalg.solve(Ab, bb), bb))
    print(f"n = {n}: backward error of the model {worst:.2e}, of numpy.linalg.solve {ref:.2e}")
    assert worst <= 16.0 * max(ref, np.finfo(np.float64).eps / 2)


@pytest.mark.parametrize("n", [1, 77, 96])
def test_model_solves_a_row_scaled_permutation(n):
    A, b, perm = scaled_permutation(n)
    x, piv, info = solve_pivoted(A, b)
    assert info == 0 and np.array_equal(piv, perm)
    assert np.allclose(x, b[perm] / A[perm, np.arange(n)], rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("n,j", [(1, 0), (77, 10), (77, 70), (96, 95)])
def test_model_reports_a_zero_column(n, j):
    A, b = gaussian_systems(n)
    A0 = A[0].copy()
    A0[:, j] = 0.0
    x, piv, info = solve_pivoted(A0, b[0])
    assert info == j + 1 and np.isnan(x).all() and (piv[:j] >= 0).all() and (piv[j:] == -1).all()
