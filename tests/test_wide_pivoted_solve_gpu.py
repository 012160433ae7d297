"""bg_wide_solve_pivoted (csrc/wide_solve.hip): the pivoted 96 x 96 solve of the wide hyper-reduced loop's repair kernel
(wide_solve_pivoted, csrc/rom_wide_device.hpp) on inputs a time loop cannot be steered to.  The pivot rows are LAPACK's, the
normwise backward error is held against numpy.linalg.solve's on the same systems, and exactly singular systems report
LAPACK's info without touching their neighbours in the batch.

The gate: the kernel's worst backward error over a case is at most 16 x numpy.linalg.solve's worst.  The NumPy model of the
same rule (tests/wide_pivot_ref.py) stays within 5.5 x on the CPU; the kernel differs from it by fused multiply-adds and a
reciprocal multiply, and the 16 x is a margin over that, not a target."""
import numpy as np
import pytest
import torch

from wide_pivot_ref import SIZES, backward_error, gaussian_systems, lapack_pivot_rows, scaled_permutation

pytestmark = pytest.mark.gpu
GATE = 16.0


def device_solve(hip, A, b, want_piv=True):
    """(x, piv, info) of bg_wide_solve_pivoted on the batch A (B, n, n), b (B, n), as numpy arrays."""
    B, n = b.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    Ad, bd = torch.as_tensor(np.ascontiguousarray(A), device=dev), torch.as_tensor(np.ascontiguousarray(b), device=dev)
    x = torch.full((B, n), -7.0, dtype=torch.float64, device=dev)
    piv = torch.full((B, n), -7, dtype=torch.int32, device=dev) if want_piv else None
    info = torch.full((B,), -7, dtype=torch.int32, device=dev)
    rc = hip.load().bg_wide_solve_pivoted(B, n, hip.ptr(Ad), hip.ptr(bd), hip.ptr(x), hip.ptr(piv), hip.ptr(info), hip.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    return x.cpu().numpy(), (piv.cpu().numpy() if want_piv else None), info.cpu().numpy()


def check_gate(A, x, b, label):
    worst = max(backward_error(Ab, xb, bb) for Ab, xb, bb in zip(A, x, b))
    ref = max(backward_error(Ab, np.linalg.solve(Ab, bb), bb) for Ab, bb in zip(A, b))
    print(f"{label}: backward error of the kernel {worst:.2e}, of numpy.linalg.solve {ref:.2e}, ratio {worst / ref:.2f}")
    assert np.isfinite(x).all() and worst <= GATE * ref, (label, worst, ref)


@pytest.mark.parametrize("n,B", [(n, 8) for n in SIZES] + [(96, 300)])
def test_gaussian_systems_lapacks_pivot_rows_and_backward_error(hip, n, B):
    from scipy.linalg import lu_factor
    A, b = gaussian_systems(n, count=B)
    x, piv, info = device_solve(hip, A, b)
    assert (info == 0).all()
    for s in range(B):
        assert np.array_equal(piv[s], lapack_pivot_rows(lu_factor(A[s])[1])), (n, s)
    check_gate(A, x, b, f"n = {n}, B = {B}")


def test_first_pivot_in_the_second_row_tile(hip):
    A, b = gaussian_systems(96, count=2)
    A = A.copy()
    A[:, 95, 0] = 50.0                                   # far above a Gaussian entry: the column-0 maximum sits in row 95
    x, piv, info = device_solve(hip, A, b)
    assert (info == 0).all() and (piv[:, 0] == 95).all()
    from scipy.linalg import lu_factor
    for s in range(2):
        assert np.array_equal(piv[s], lapack_pivot_rows(lu_factor(A[s])[1]))
    check_gate(A, x, b, "n = 96, column-0 maximum in row 95")


def test_row_scaled_permutation(hip):
    A, b, perm = scaled_permutation(96)
    x, piv, info = device_solve(hip, A[None], b[None])
    assert info[0] == 0 and np.array_equal(piv[0], perm)
    check_gate(A[None], x, b[None], "n = 96, row-scaled permutation")
    assert np.allclose(x[0], b[perm] / A[perm, np.arange(96)], rtol=4 * np.finfo(np.float64).eps, atol=0.0)


def test_singular_systems_report_info_and_leave_their_neighbours_alone(hip):
    A, b = gaussian_systems(77, count=4)
    A = A.copy()
    A[1, :, 10] = 0.0
    A[2, :, 70] = 0.0
    x, piv, info = device_solve(hip, A, b)
    assert info.tolist() == [0, 11, 71, 0]
    check_gate(A[[0, 3]], x[[0, 3]], b[[0, 3]], "n = 77, the regular systems beside two singular ones")
    alone, piv_alone, _ = device_solve(hip, A[[0, 3]], b[[0, 3]])
    assert np.array_equal(alone, x[[0, 3]]) and np.array_equal(piv_alone, piv[[0, 3]])


def test_one_unknown_and_no_piv_output(hip):
    A, b = gaussian_systems(1, count=8)
    x, piv, info = device_solve(hip, A, b)
    assert (info == 0).all() and (piv == 0).all()
    check_gate(A, x, b, "n = 1")
    x2, _, info2 = device_solve(hip, A, b, want_piv=False)
    assert np.array_equal(x2, x) and (info2 == 0).all()
    zero = np.zeros((1, 1, 1))
    _, _, info0 = device_solve(hip, zero, np.ones((1, 1)))
    assert info0.tolist() == [1]
