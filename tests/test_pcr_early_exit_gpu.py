"""The two exits of the interface PCR (csrc/fom_device.hpp, pcr64): after its stride-4 step a wave whose couplings are all
<= tau = 2^-31 runs the stride-8 step in its last form and drops strides 16 and 32 ("short"), every other wave runs all six
steps ("full").  Which exit a system takes is decided here on the CPU by a NumPy restatement of the Wang interface equation
and the first three PCR steps, with a factor of four to either side of tau, so that rounding differences between host and
device cannot flip a case and no case can silently stop covering its exit.

Gates: rel-L2 < 1e-12 against the pivoted banded solve for the solver (the gate of
test_fom_gpu.test_cross_lane_primitives_via_tridiag_solve; the systems have condition numbers <= 13, so the reference is five
orders inside it), rel-L2 <= 1e-10 and identical iteration counts against the oracles for the time loops."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from oracle import burgers_ref as br
from oracle import burgers_ref_c as bc

TAU = 2.0 ** -31
ROWS_PER_LANE = (1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 16, 24)       # dispatch_r of csrc/fom.hip
SIZES = (64, 100, 128, 1000, 1024, 1536)                       # one wavefront per system
WIDE_SIZES = (2048, 4096)                                      # one workgroup per system
FAMILIES = ("dominant", "skew", "half")
EXIT = {"dominant": "short", "skew": "full", "half": "full"}
SOLVE_TOL = 1e-12
RUN_TOL = 1e-10


def _family(kind, N, rng):
    """One system of a family; every family draws the same number of variates, so the seed fixes all three."""
    dom = (rng.uniform(-0.05, 0.05, N), rng.uniform(0.9, 1.1, N), rng.uniform(-0.05, 0.05, N))
    skw = (-0.5 * rng.uniform(0.95, 1.05, N), rng.uniform(0.08, 0.12, N), 0.5 * rng.uniform(0.95, 1.05, N))
    if kind == "dominant":
        lo, di, up = dom
    elif kind == "skew":
        lo, di, up = skw
    else:                                                      # skew on rows N/4 ... 3N/4, dominant elsewhere
        mid = np.zeros(N, dtype=bool)
        mid[N // 4:3 * N // 4] = True
        lo, di, up = (np.where(mid, s, d) for s, d in zip(skw, dom))
    lo = lo.copy(); up = up.copy()
    lo[0] = 0.0; up[-1] = 0.0
    return lo, di.copy(), up, rng.standard_normal(N)


@functools.lru_cache(maxsize=None)
def _batch(N):
    """Six systems that interleave the three families (samples 0-3 share a workgroup, so it holds waves on both exits)
    and their reference solutions.  Computed once per size; the arrays are read-only."""
    rng = np.random.default_rng(31000 + N)
    kinds = FAMILIES * 2
    sys_ = [_family(k, N, rng) for k in kinds]
    lo, di, up, rhs = (np.stack([s[i] for s in sys_]) for i in range(4))
    ref = np.stack([br.tridiag_solve(lo[b], di[b], up[b], rhs[b]) for b in range(len(kinds))])
    for a in (lo, di, up, rhs, ref):
        a.setflags(write=False)
    return kinds, lo, di, up, rhs, ref


def _shift(v, s):
    """v[j - s] at j, zero outside 0 ... 63 (s < 0: v[j + |s|])."""
    out = np.zeros_like(v)
    if s > 0:
        out[s:] = v[:-s]
    else:
        out[:s] = v[-s:]
    return out


def interface_m3(lo, di, up):
    """max(|A|, |C|) over the 64 interface equations after three PCR steps (strides 1, 2, 4): what pcr64 tests against tau.
    Restates wang_reduce / wang_interface / pcr_step of csrc/fom_device.hpp with exact divisions; lane p owns rows
    [pR, pR + R), rows >= N are identity rows."""
    N = len(di)
    R = next(r for r in ROWS_PER_LANE if N <= 64 * r)
    l = np.zeros(64 * R); d = np.ones(64 * R); u = np.zeros(64 * R)
    l[:N] = lo; d[:N] = di; u[:N] = up
    l, d, u = l.reshape(64, R), d.reshape(64, R), u.reshape(64, R)
    if R == 1:
        A, C = l[:, 0] / d[:, 0], u[:, 0] / d[:, 0]
    else:
        f = l.copy(); inv = np.empty_like(d); g = np.zeros_like(d)
        dp = d[:, 0]
        inv[:, 0] = 1.0 / dp
        for j in range(1, R):                                  # sub-diagonal downwards: left spike f, 1 / pivot
            m = l[:, j] * inv[:, j - 1]
            dp = d[:, j] - m * u[:, j - 1]
            inv[:, j] = 1.0 / dp
            f[:, j] = -m * f[:, j - 1]
        g[:, R - 2] = u[:, R - 2]
        for j in range(R - 3, -1, -1):                         # super-diagonal upwards from row R-3: right spike g
            t = u[:, j] * inv[:, j + 1]
            f[:, j] = f[:, j] - t * f[:, j + 1]
            g[:, j] = -t * g[:, j + 1]
        F0, G0 = _shift(f[:, 0] * inv[:, 0], -1), _shift(g[:, 0] * inv[:, 0], -1)
        ul = u[:, R - 1]
        B = dp - ul * F0
        A, C = f[:, R - 1] / B, -(ul * G0) / B
    for s in (1, 2, 4):
        Bn = 1.0 - _shift(C, s) * A - _shift(A, -s) * C
        A, C = -(_shift(A, s) * A) / Bn, -(_shift(C, -s) * C) / Bn
    return float(max(np.abs(A).max(), np.abs(C).max()))


def _assert_classes(N):
    kinds, lo, di, up, _, _ = _batch(N)
    for b, kind in enumerate(kinds):
        m3 = interface_m3(lo[b], di[b], up[b])
        if EXIT[kind] == "short":
            assert m3 <= 2.0 ** -33, f"N={N} {kind}: m3/tau = {m3 / TAU:.3g}, not safely on the short exit"
        else:
            assert m3 >= 2.0 ** -29, f"N={N} {kind}: m3/tau = {m3 / TAU:.3g}, not safely on the full exit"


@pytest.mark.parametrize("N", SIZES)
def test_families_sit_a_factor_of_four_from_the_threshold(N):
    """Needs no GPU: the CPU classification of every test system, and the conditioning the gate's margin rests on."""
    _assert_classes(N)
    kinds, lo, di, up, _, _ = _batch(N)
    for b in range(3):
        assert np.linalg.cond(br.tridiag_dense(lo[b], di[b], up[b])) <= 13.0, (N, kinds[b])


def _solve(lo, di, up, rhs):
    from burgers_hip import fom
    sol = fom.tridiag_solve(*[torch.tensor(np.asarray(a), device="cuda") for a in (lo, di, up, rhs)])
    torch.cuda.synchronize()
    return sol.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_both_exits_in_one_workgroup(hip, N):
    _assert_classes(N)
    kinds, lo, di, up, rhs, ref = _batch(N)
    sol = _solve(lo, di, up, rhs)
    for b, kind in enumerate(kinds):
        e = rel_l2(sol[b], ref[b])
        print(f"N={N} {kind}: rel-L2 {e:.2e}")
        assert e < SOLVE_TOL, f"N={N} sample {b} ({kind}, {EXIT[kind]} exit): {e:.2e}"


@pytest.mark.gpu
@pytest.mark.parametrize("N", WIDE_SIZES)
def test_workgroup_wide_solver_inherits_the_exit(hip, N):
    """wide_tridiag_solve closes with the same pcr64; accuracy only."""
    kinds, lo, di, up, rhs, ref = _batch(N)
    sol = _solve(lo, di, up, rhs)
    for b, kind in enumerate(kinds):
        e = rel_l2(sol[b], ref[b])
        print(f"N={N} {kind}: rel-L2 {e:.2e}")
        assert e < SOLVE_TOL, f"N={N} sample {b} ({kind}): {e:.2e}"


@pytest.mark.gpu
@pytest.mark.parametrize("bad,field", [(0, "rhs"), (1, "rhs"), (3, "lo")])
def test_nonfinite_sample_stays_alone(hip, bad, field):
    """A NaN in one sample (a short-exit one, a full-exit one; in the right-hand side, in a coefficient, where it makes
    the couplings NaN and must fail the test against tau): that sample comes back non-finite, the other waves of its
    workgroup and the rest of the batch still meet the gate."""
    N = 1024
    kinds, lo, di, up, rhs, ref = _batch(N)
    arrs = {"lo": lo.copy(), "di": di.copy(), "up": up.copy(), "rhs": rhs.copy()}
    arrs[field][bad, 517] = np.nan
    sol = _solve(arrs["lo"], arrs["di"], arrs["up"], arrs["rhs"])
    assert not np.isfinite(sol[bad]).all()
    for b, kind in enumerate(kinds):
        if b != bad:
            assert rel_l2(sol[b], ref[b]) < SOLVE_TOL, f"sample {b} ({kind}) next to a NaN in sample {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 1000])
def test_fom_run_end_to_end(hip, N):
    """The time loop at the bench's mesh and step (short exit; N = 1000 with padded rows) against the C oracle."""
    from burgers_hip import fom
    rng = np.random.default_rng(77 + N)
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


@pytest.mark.gpu
def test_fd_stepper_end_to_end(hip):
    from burgers_hip import fom
    rng = np.random.default_rng(78)
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
