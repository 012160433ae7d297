"""bg_fd_run (csrc/fd.hip) against oracle.burgers_ref.fd_newton at the rows-per-lane rungs, the 64 R boundaries and the
exits the rest of the suite never takes: the iteration cap, the residual exit, a mesh that does not start at 0 and a
non-finite state.  Tolerances are this stepper's own (tests/test_fom_gpu.py): rel-L2 < 1e-10 on the history, identical
iteration counts.  What each group would catch is said in its docstring."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import burgers_ref as br

pytestmark = pytest.mark.gpu
TOL = 1e-10
# rows per lane 1 (N <= 64), 2 (<= 128), 4 (<= 256), 8 (<= 512), 12 (<= 768) in the wave form, on and around 64 R;
# 16 rows per thread (3073 ... 4096) in the workgroup form
WAVE_SIZES = [3, 4, 5, 63, 64, 65, 128, 129, 256, 257, 513, 768, 769]
WIDE_SIZES = [3073, 4096]


def _shape(N):
    """(B, nsteps): five samples are one full workgroup of four waves and one with a single live wave."""
    return (5, 6) if N <= 2048 else (2, 4)


@functools.lru_cache(maxsize=None)
def _inputs(N):
    B, nT = _shape(N)
    rng = np.random.default_rng(7000 + N)
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    X = np.linspace(0.0, 100.0, N)
    u0 = 1.0 + 0.3 * np.sin(np.outer(rng.uniform(0.5, 2.0, B), X / 100 * np.pi))
    return mu1, mu2, u0, min(0.5, 0.05 * 512 / N), nT


@functools.lru_cache(maxsize=None)
def _oracle(N, max_iter=30, tol=1e-8):
    """(hist (B, nT + 1, N), iters (B, nT)) of the reference on _inputs(N); computed once, read only."""
    mu1, mu2, u0, dt, nT = _inputs(N)
    out = [br.fd_newton(0.0, 100.0, N, dt, nT, u0[b], mu1[b], mu2[b], max_iter=max_iter, tol=tol, return_iters=True)
           for b in range(len(mu1))]
    hist = np.stack([U.T for U, _ in out]); iters = np.stack([it for _, it in out])
    assert np.isfinite(hist).all()
    hist.setflags(write=False); iters.setflags(write=False)
    return hist, iters


def _run(N, **kw):
    from burgers_hip import fom
    mu1, mu2, u0, dt, nT = _inputs(N)
    res = fom.fd_run(0.0, 100.0, N, u0, mu1, mu2, dt, nT, **kw)
    torch.cuda.synchronize()
    return res.hist.cpu().numpy(), res.iters.cpu().numpy(), res.flags.cpu().numpy()


def _check(N, got, ref):
    (h, it, _), (ho, ito) = got, ref
    for b in range(len(h)):
        err = rel_l2(h[b], ho[b])
        print(f"N={N} sample {b}: rel-L2 {err:.2e}, solves {it[b].tolist()} / {ito[b].tolist()}")
        assert err < TOL, (N, b, err)
        assert np.array_equal(it[b], ito[b]), (N, b)


@pytest.mark.parametrize("N", WAVE_SIZES + WIDE_SIZES)
def test_rungs_and_boundaries(hip, N):
    """Every instantiation the suite did not run (1, 4, 12 rows per lane; 16 per thread) and the sizes on either side of a
    rung.  A rung built with the wrong row mask, a halo taken from a lane past the last row or a boundary row owned by the
    wrong lane changes the history at once; a wave that does not return at s >= B writes past `flags`."""
    got = _run(N)
    _check(N, got, _oracle(N))
    assert (got[2] == 0).all(), got[2]


def test_interval_not_starting_at_zero(hip):
    """x in [-20, 60]: the source term reads x[i] (not i dx) and dx comes from both ends."""
    from burgers_hip import fom
    N, B, dt, nT = 200, 5, 0.05, 6
    rng = np.random.default_rng(11)
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    X = np.linspace(-20.0, 60.0, N)
    u0 = 1.0 + 0.3 * np.sin(np.outer(rng.uniform(0.5, 2.0, B), (X + 20.0) / 80 * np.pi))
    res = fom.fd_run(-20.0, 60.0, N, u0, mu1, mu2, dt, nT)
    torch.cuda.synchronize()
    for b in range(B):
        Uo, ito = br.fd_newton(-20.0, 60.0, N, dt, nT, u0[b], mu1[b], mu2[b], return_iters=True)
        assert np.isfinite(Uo).all()
        assert rel_l2(res.hist[b].cpu().numpy().T, Uo) < TOL, b
        assert np.array_equal(res.iters[b].cpu().numpy(), ito), b
    assert not bool(res.flags.any())


@pytest.mark.parametrize("N", WAVE_SIZES + WIDE_SIZES)
def test_iteration_cap(hip, N):
    """max_iter = 2: every step stops at the cap, with the state of the second solve, and says so.  Catches a cap that is
    off by one, a flag set from the wrong condition and a count written before the last solve."""
    from burgers_hip import lib
    got = _run(N, max_iter=2)
    ref = _oracle(N, max_iter=2)
    assert (ref[1] == 2).all()
    _check(N, got, ref)
    assert (got[1] == 2).all()
    assert ((got[2] & lib.BG_FLAG_HIT_CAP) != 0).all() and ((got[2] & lib.BG_FLAG_NONFINITE) == 0).all(), got[2]


@pytest.mark.parametrize("N", [3, 63, 64, 129, 256, 769, 3073])
def test_residual_exit(hip, N):
    """tol = 1e-3: steps end on the residual test at the top of an iteration, and a step then takes fewer solves than its
    neighbours (the reference's counts here: 1 or 2 at N = 3, one sample with [3, 3, 2, 2, 2, 2] at N = 769, 3 elsewhere).
    Catches a residual test placed after the solve, or a count that includes the iteration that only tested."""
    got = _run(N, tol=1e-3)
    ref = _oracle(N, tol=1e-3)
    _check(N, got, ref)
    assert (got[2] == 0).all(), got[2]


def _nonfinite_case(N, B, nT, max_iter, bad, row, value):
    """bg_fd_run with u0[bad, row] = value (``row`` None: mu2[bad] = value, a finite state with a NaN source term) beside the
    same batch left healthy; the reference on the bad sample."""
    from burgers_hip import fom
    rng = np.random.default_rng(N + (row or 0))
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    mu1[bad], mu2[bad] = 5.0, 0.02
    dt = 0.05 * min(1.0, 512 / N)
    u0 = np.ones((B, N))
    healthy = fom.fd_run(0.0, 100.0, N, u0, mu1, mu2, dt, nT, max_iter=max_iter)
    torch.cuda.synchronize()
    if row is None:
        mu2[bad] = value
    else:
        u0[bad, row] = value
    res = fom.fd_run(0.0, 100.0, N, u0, mu1, mu2, dt, nT, max_iter=max_iter)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        Uo, ito = br.fd_newton(0.0, 100.0, N, dt, nT, u0[bad], mu1[bad], mu2[bad], max_iter=max_iter, return_iters=True)
    return res, healthy, Uo, ito


def _check_nonfinite(res, healthy, Uo, ito, bad, max_iter):
    from burgers_hip import lib
    assert (ito == max_iter).all(), ito                          # np.max propagates NaN: neither stopping test ever holds
    it, fl = res.iters.cpu().numpy(), res.flags.cpu().numpy()
    print(f"bad sample: solves {it[bad].tolist()} / {ito.tolist()}, flags {int(fl[bad])}")
    assert np.array_equal(it[bad], ito)
    assert fl[bad] & lib.BG_FLAG_NONFINITE and fl[bad] & lib.BG_FLAG_HIT_CAP
    assert np.array_equal(np.isfinite(res.hist[bad].cpu().numpy().T), np.isfinite(Uo))
    keep = [b for b in range(len(it)) if b != bad]
    assert torch.equal(res.hist[keep], healthy.hist[keep]) and torch.equal(res.iters[keep], healthy.iters[keep])
    assert torch.equal(res.flags[keep], healthy.flags[keep])


@pytest.mark.parametrize("bad,row,value", [(1, 40, np.nan), (4, 100, np.inf)])
def test_nonfinite_state_is_flagged_not_converged(hip, bad, row, value):
    """A NaN (or an Inf, which turns into NaN in the first residual) in one sample's state.  The reference's maxima are
    np.max, NaN then, so it takes max_iter solves per step and reports non-convergence.  A kernel whose maxima drop NaN
    (plain fmax) sees a residual of 0 and ends every step as converged with flags == 0: before its maxima carried a
    NaN bit bg_fd_run returned the counts [1, 0, 0] and flags 0 for both of these samples, beside a NaN history."""
    res, healthy, Uo, ito = _nonfinite_case(256, 6, 3, 7, bad, row, value)
    _check_nonfinite(res, healthy, Uo, ito, bad, 7)


def test_nonfinite_state_workgroup_form(hip):
    """The same through the workgroup form, whose maxima also cross the four waves through LDS (counts [1, 0] and flags 0
    before the fix).  max_iter = 4 caps the healthy sample too: it must be what it is in the healthy run."""
    res, healthy, Uo, ito = _nonfinite_case(2049, 2, 2, 4, 1, 40, np.nan)
    _check_nonfinite(res, healthy, Uo, ito, 1, 4)


@pytest.mark.parametrize("N,B,nT,max_iter", [(256, 6, 3, 7), (2049, 2, 2, 4)])
def test_nan_residual_on_a_finite_state(hip, N, B, nT, max_iter):
    """mu2 = NaN in one sample: the state is finite, the source term and with it every interior residual is NaN.  The
    maximum of the residual drops them all and is 0 < tol, so this is the one case that reaches the look at the rows the
    kernel takes before it leaves on the residual test; in the workgroup form that look holds a barrier inside a uniform
    branch.  The reference takes max_iter solves per step."""
    res, healthy, Uo, ito = _nonfinite_case(N, B, nT, max_iter, 1, None, np.nan)
    _check_nonfinite(res, healthy, Uo, ito, 1, max_iter)
