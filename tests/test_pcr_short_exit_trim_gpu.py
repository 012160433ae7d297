"""The short exit of the interface PCR without its exact no-ops (csrc/fom_device.hpp, pcr64) and the scalar non-finite test
of the Picard loops (csrc/wave_ops.hpp, uniform_nonfinite).

On the short exit every coupling is <= tau = 2^-31, so the new diagonal of the stride-8 step, B_n = fma(-A_p, C, fma(-C_m, A, 1)),
is exactly 1.0, rcp1(1.0) is 1.0 and D = D_n * 1.0 is D_n: the kernel forms D_n alone.  The first test restates both forms of
that step on the CPU (exact fused multiply-adds through rationals) and requires them to agree bit for bit; the GPU tests run
both exits through the solver, the non-finite flag through the time loop, and the time loops against the oracles.

Gates: rel-L2 < 1e-12 against the pivoted banded solve for the solver (the gate of test_pcr_early_exit_gpu, whose systems
these are), rel-L2 <= 1e-10 and identical iteration counts against the oracles for the time loops.

Flags: the four samples of test_nonfinite_flag_per_sample were also run on the parent commit's library (BG_LIB_PATH, same
GPU, same session): flags [0, 2, 2, 2] and iteration counts [[6, 5, 5], [1, 1, 1], [1, 1, 1], [1, 1, 1]], the values
asserted here and those of the C oracle."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from oracle import burgers_ref as br
from oracle import burgers_ref_c as bc
from test_pcr_early_exit_gpu import EXIT, TAU, _batch, interface_m3

SOLVE_TOL = 1e-12
RUN_TOL = 1e-10
BG_FLAG_NONFINITE = 2                                           # include/burgers_hip.h


# ---- CPU: the stride-8 step of the short exit in both forms --------------------------------------------------------------
def _fma(a, b, c):
    """Elementwise fma with one rounding: exact in rationals, then rounded to nearest even by float()."""
    f = lambda x, y, z: float(Fraction(x) * Fraction(y) + Fraction(z))
    return np.vectorize(f, otypes=[np.float64])(a, b, c)


def _row_shift(v, s):
    """v[j - s] at j inside each row of 16 lanes, zero filled at the row ends (row_shr:s; s < 0: row_shl:|s|)."""
    v = v.reshape(4, 16)
    out = np.zeros_like(v)
    if s > 0:
        out[:, s:] = v[:, :-s]
    else:
        out[:, :s] = v[:, -s:]
    return out.reshape(64)


def _stride8_last_step(A, C, D):
    """(B_n, D of the parent's LAST step, D of the new short exit); stride 8 is row_shr / row_shl 2 after the transpose."""
    Cm, Ap = _row_shift(C, 2), _row_shift(A, -2)
    Dm, Dp = _row_shift(D, 2), _row_shift(D, -2)
    Bn = _fma(-Ap, C, _fma(-Cm, A, np.ones(64)))
    Dn = _fma(-Dp, C, _fma(-Dm, A, D))
    r = 1.0 / Bn                                                # rcp1 with an exact seed: one Newton step on top of it
    r = _fma(r, _fma(-Bn, r, np.ones(64)), r)
    return Bn, Dn * r, Dn


@functools.lru_cache(maxsize=None)
def _couplings(scale):
    """Draws of (A, C, D) with |A|, |C| <= scale: uniform ones, every lane at an end point (both signs, and alternating,
    so that neighbours two lanes apart multiply to the largest product), all zero, and zeros mixed into a uniform draw."""
    rng = np.random.default_rng(8062)
    alt = np.where(np.arange(64) % 4 < 2, scale, -scale)
    draws = [(rng.uniform(-scale, scale, 64), rng.uniform(-scale, scale, 64)) for _ in range(6)]
    draws += [(np.full(64, scale), np.full(64, scale)), (np.full(64, -scale), np.full(64, scale)),
              (np.full(64, -scale), np.full(64, -scale)), (alt, -alt), (np.zeros(64), np.zeros(64))]
    a, c = (rng.uniform(-scale, scale, 64) for _ in range(2))
    a[::3] = 0.0; c[1::5] = 0.0; a[7] = scale; c[9] = -scale
    draws.append((a, c))
    out = []
    for a, c in draws:
        d = rng.standard_normal(64) * 10.0 ** rng.integers(-3, 4, 64)
        d[5] = 0.0; d[6] = -0.0
        out.append((a, c, d))
    return out


def test_short_stride8_step_is_its_right_hand_side_alone():
    for A, C, D in _couplings(TAU):
        assert np.abs(A).max() <= TAU and np.abs(C).max() <= TAU
        Bn, D_parent, D_new = _stride8_last_step(A, C, D)
        assert np.all(Bn == 1.0)
        assert np.array_equal(D_parent.view(np.int64), D_new.view(np.int64))


def test_a_coupling_above_the_threshold_moves_the_diagonal():
    """Not vacuous: at 2^-26 the products reach 2^-52 and B_n leaves 1."""
    scale = 2.0 ** -26
    Bn, _, _ = _stride8_last_step(np.full(64, scale), np.full(64, scale), np.ones(64))
    assert np.any(Bn != 1.0)


# ---- GPU: solver ---------------------------------------------------------------------------------------------------------
def _solve(lo, di, up, rhs):
    from burgers_hip import fom
    sol = fom.tridiag_solve(*[torch.tensor(np.asarray(a), device="cuda") for a in (lo, di, up, rhs)])
    torch.cuda.synchronize()
    return sol.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [64, 128, 1000, 1024, 2048])
def test_both_exits_after_the_trim(hip, N):
    """R = 1, R = 2, padded rows, the bench's size, the workgroup solver; six systems, so both exits share a workgroup."""
    kinds, lo, di, up, rhs, ref = _batch(N)
    assert len(kinds) == 6
    if N <= 1536:                                               # interface_m3 restates the one-wavefront partition
        for b, kind in enumerate(kinds):
            m3 = interface_m3(lo[b], di[b], up[b])
            if EXIT[kind] == "short":
                assert m3 <= TAU / 4, f"N={N} {kind}: m3/tau = {m3 / TAU:.3g}, not safely on the short exit"
            else:
                assert m3 >= TAU * 4, f"N={N} {kind}: m3/tau = {m3 / TAU:.3g}, not safely on the full exit"
    sol = _solve(lo, di, up, rhs)
    for b, kind in enumerate(kinds):
        e = rel_l2(sol[b], ref[b])
        print(f"N={N} {kind}: rel-L2 {e:.2e}")
        assert e < SOLVE_TOL, f"N={N} sample {b} ({kind}, {EXIT[kind]} exit): {e:.2e}"


# ---- GPU: the non-finite flag --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nonfinite_flag_per_sample(hip):
    """finite | NaN in u0 | u0 = 1e160 (the norm of u overflows to inf in the first iteration, while u is still finite) |
    mu1 = inf.  The exponent test on the high word must flag exactly the last three."""
    from burgers_hip import fom
    N, B, nsteps, dt = 128, 4, 3, 0.025
    X, _ = mesh(N)
    u0 = np.ones((B, N)); u0[1, 37] = np.nan; u0[2] = 1e160
    mu1 = np.array([4.7, 4.7, 4.7, np.inf]); mu2 = np.full(B, 0.02)
    res = fom.fom_run(X, u0, mu1, mu2, dt, nsteps)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        ho, ito = bc.fom_run(X, u0, mu1, mu2, dt, nsteps)
    flags, iters = res.flags.cpu().numpy(), res.iters.cpu().numpy()
    print("flags", flags.tolist(), "iters", iters.tolist(), "oracle iters", ito.tolist())
    assert np.array_equal(iters, ito)
    assert ((flags & BG_FLAG_NONFINITE) != 0).tolist() == [False, True, True, True]
    e = rel_l2(res.hist[0].cpu().numpy(), ho[0])
    print(f"finite sample: rel-L2 {e:.2e}")
    assert e <= RUN_TOL


# ---- GPU: time loops -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 1000])
def test_fom_run_against_the_oracle(hip, N):
    from burgers_hip import fom
    rng = np.random.default_rng(177 + N)
    B, nsteps, dt = 5, 8, 0.025
    X, _ = mesh(N)
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    res = fom.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps)
    torch.cuda.synchronize()
    ho, ito = bc.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps)
    e = rel_l2(res.hist.cpu().numpy(), ho)
    print(f"fom_run N={N}: rel-L2 {e:.2e}")
    assert e <= RUN_TOL
    assert np.array_equal(res.iters.cpu().numpy(), ito)
    assert not (res.flags.cpu().numpy() & BG_FLAG_NONFINITE).any()


@pytest.mark.gpu
def test_fd_run_against_the_oracle(hip):
    from burgers_hip import fom
    rng = np.random.default_rng(178)
    N, B, nsteps, dt = 1024, 2, 4, 0.025
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    res = fom.fd_run(0.0, 100.0, N, np.ones(N), mu1, mu2, dt, nsteps)
    torch.cuda.synchronize()
    for b in range(B):
        Uo, ito = br.fd_newton(0.0, 100.0, N, dt, nsteps, np.ones(N), mu1[b], mu2[b], return_iters=True)
        e = rel_l2(res.hist[b].cpu().numpy().T, Uo)
        print(f"fd_run sample {b}: rel-L2 {e:.2e}")
        assert e <= RUN_TOL
        assert np.array_equal(res.iters[b].cpu().numpy(), ito)
    assert not (res.flags.cpu().numpy() & BG_FLAG_NONFINITE).any()
