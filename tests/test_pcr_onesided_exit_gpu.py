"""The one-sided exit of the interface PCR (csrc/fom_device.hpp, pcr64_onesided): after the stride-1 step a wave whose lower
couplings are all <= tau_A = 2^-28 and whose upper ones are all <= tau_J = 2^-9 closes A x[j-2] + x[j] + C x[j+2] = D from
y = D by three sweeps y <- D - C y[j+2], the fold D' = D - A y[j-2] of the second iterate, and three sweeps
y <- D' - C y[j+2] from the third ("onesided").  Every other wave restarts from the stride-1 step and takes the routes of
tests/test_pcr_jacobi_exit_gpu.py: six two-sided sweeps ("jacobi"), the exit against tau ("short"), all six steps ("full").
The route is compiled into the FEM stepper on a uniform mesh and into bg_tridiag_solve, where a lane owns at least 12 rows
(N = 1024: 16, N = 768: 12); at N = 128, in the workgroup solver (N = 2049), on a graded mesh and in the FD stepper the
earlier routes run, and the same checks pin that.

The restatement helpers, the reference solves and the gates are those of test_pcr_jacobi_exit_gpu.py.  Route against a
longdouble solve: 2^-50 max|X| (truncation < 2^-53 max|X|, see the header of pcr64_onesided, plus the roundings of the last
sweep).  Solver: rel-L2 < 1e-12 against the dense solve (condition numbers <= 13).  Time loops: rel-L2 <= 1e-10 and identical
iteration counts against the oracles, no flags."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from oracle import burgers_ref as br
from oracle import burgers_ref_c as bc
from test_pcr_jacobi_exit_gpu import (RUN_TOL, SOLVE_TOL, SWEEP_TOL, TAU, TAU_J, _assemble_uniform, _cond, _coupling_cases,
                                      _family, _fma, _graded, _partition, _shift, _solve, _solve_distance2, pcr_step,
                                      wang_finish, wang_interface)

TAU_A = 2.0 ** -28
FAMILIES = ("onesided", "twosided", "patch", "skew")           # four waves: one workgroup of the wave-per-system solver
ROUTE = {"onesided": "onesided", "twosided": "jacobi", "patch": "short", "skew": "full"}


def route(A, C, D, fma):
    """pcr64_onesided of csrc/fom_device.hpp; fma(a, b, c) = a * b + c, with one rounding or with two."""
    y = D
    for _ in range(2):
        y = fma(-_shift(y, -2), C, D)
    Df = fma(-_shift(y, 2), A, D)                              # the fold reads the second iterate, beside the third sweep
    y = fma(-_shift(y, -2), C, D)
    for _ in range(3):
        y = fma(-_shift(y, -2), C, Df)
    return y


def _route_errors(scale_a, scale_c):
    """max|x - ref| / max|ref| of the route with exact FMAs per coupling family, A on [-scale_a, scale_a] and C on
    [-scale_c, scale_c], end points and zeros included."""
    out = {}
    for name, (A, C, D) in _coupling_cases(1.0).items():
        A, C = A * scale_a, C * scale_c                        # powers of two: the end points stay end points
        ref = _solve_distance2(A, C, D)
        out[name] = float(np.abs(route(A, C, D, _fma).astype(np.longdouble) - ref).max() / np.abs(ref).max())
    return out


def test_route_against_longdouble_solve():
    for name, err in _route_errors(TAU_A, TAU_J).items():
        print(f"{name}: max|x - ref| / max|ref| = {err:.2e} ({err / SWEEP_TOL:.3f} of the gate)")
        assert err <= SWEEP_TOL, name


@pytest.mark.parametrize("fa,fc", [(64.0, 1.0), (1.0, 8.0)])
def test_thresholds_are_not_decorative(fa, fc):
    """At 64 tau_A the fold errs by a (c^3 + a) ~ 2^-44, at 8 tau_J the last three sweeps leave c^3 (c^4 + a) ~ 2^-42: the
    gate must see either."""
    worst = max(_route_errors(fa * TAU_A, fc * TAU_J).values())
    print(f"couplings at {fa:g} tau_A, {fc:g} tau_J: {worst:.2e} ({worst / SWEEP_TOL:.1f} of the gate)")
    assert worst > SWEEP_TOL


def test_flagship_sits_on_the_route():
    """bench.py's mesh and step at the two mu1 = 5.5 corners of its parameter box, every Picard iteration of all 500 steps
    (the largest |A| grows over the run: 1.3e-10 after 60 steps, 3.9e-10 after 500): assembly, Wang partition, stride-1 step
    and the route as the solve.  |A| stays a factor of four under tau_A, |C| a factor of two under tau_J, and the iteration
    counts are the C oracle's."""
    N, dt, nsteps, tol, max_it = 1024, 0.025, 500, 1e-6, 20
    X, _ = mesh(N)
    h = X[1] - X[0]
    mu1 = np.array([5.5, 5.5]); mu2 = np.array([0.03, 0.015])
    M3 = br.mass_tridiag(X)
    dtF = dt * br.forcing_vector(X, mu2)
    gp = (1.0 + np.array([-1.0, 1.0])[:, None] / np.sqrt(3.0)) / 2.0
    fsum = sum(0.02 * np.exp(mu2[:, None] * ((1.0 - w) * X[:-1] + w * X[1:])) for w in gp)
    Un = np.ones((2, N))
    iters = np.zeros((2, nsteps), dtype=np.int32)
    worst_a = worst_c = 0.0
    for n in range(nsteps):
        g = br.tridiag_matvec(*M3, Un) + dtF
        U0 = Un
        active = np.ones(2, dtype=bool)
        while active.any():
            lo, di, up, rhs = _assemble_uniform(h, dt, U0, g, fsum, mu1)
            A, C, D, ctx = wang_interface(lo, di, up, rhs)
            A, C, D = pcr_step(A, C, D, 1)
            worst_a = max(worst_a, float(np.abs(A[active]).max()))
            worst_c = max(worst_c, float(np.abs(C[active]).max()))
            dU = wang_finish(ctx, route(A, C, D, lambda a, b, c: a * b + c))
            U1 = U0 + dU
            err = np.linalg.norm(dU, axis=1) / np.linalg.norm(U1, axis=1)
            U0 = np.where(active[:, None], U1, U0)
            iters[active, n] += 1
            active = active & (err > tol) & (iters[:, n] < max_it)
        Un = U0
    print(f"after the stride-1 step: largest |A| {worst_a:.3e} = tau_A / {TAU_A / worst_a:.2f}, largest |C| {worst_c:.3e} = "
          f"tau_J / {TAU_J / worst_c:.2f}; iterations {iters.sum(axis=1).tolist()}")
    assert worst_a <= TAU_A / 4
    assert worst_c <= TAU_J / 2
    ho, ito = bc.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps)
    assert np.array_equal(iters, ito)
    assert rel_l2(Un, ho[:, -1]) <= RUN_TOL


# ---- solver entry: four routes side by side ------------------------------------------------------------------------------

def _system(kind, N, rng):
    """One system of a family; every family draws the same number of variates.  onesided: (-0.3, 0.45, 0.5), sub- and
    super-diagonal of opposite sign and unequal size as in the flagship's matrix: the left spike of a lane decays much
    faster than the right one.  twosided: (-1, 1, 1), both spikes decay by 0.62 per row, far enough for the sweeps and not
    for tau_A.  patch, skew: the families of test_pcr_jacobi_exit_gpu.py."""
    base = _family(kind if kind in ("patch", "skew") else "dominant", N, rng)
    shape = {"onesided": (-0.3, 0.45, 0.5), "twosided": (-1.0, 1.0, 1.0)}.get(kind)
    if shape is None:
        return base
    lo, di, up = (s * rng.uniform(0.95, 1.05, N) for s in shape)
    lo[0] = 0.0; up[-1] = 0.0
    return lo, di, up, base[3]


@functools.lru_cache(maxsize=None)
def _batch(N):
    """Four systems, one workgroup of the wave-per-system solver, and their dense solutions.  Computed once per size; the
    arrays are read-only."""
    rng = np.random.default_rng(9100 + N)
    sys_ = [_system(k, N, rng) for k in FAMILIES]
    lo, di, up, rhs = (np.stack([s[i] for s in sys_]) for i in range(4))
    ref = np.stack([np.linalg.solve(br.tridiag_dense(lo[b], di[b], up[b]), rhs[b]) for b in range(len(FAMILIES))])
    for a in (lo, di, up, rhs, ref):
        a.setflags(write=False)
    return lo, di, up, rhs, ref


def _couplings(lo, di, up):
    """(a, c, m_tau): largest |A| and |C| where pcr64 takes its ballots after the stride-1 step, and the largest coupling
    where it tests against tau, after the stride-4 step.  One wave per system."""
    assert _partition(len(di))[2] == 0
    A, C, D, _ = wang_interface(lo, di, up, np.zeros_like(di))
    A, C, D = pcr_step(A, C, D, 1)
    a, c = float(np.abs(A).max()), float(np.abs(C).max())
    for s in (2, 4):
        A, C, D = pcr_step(A, C, D, s)
    return a, c, float(max(np.abs(A).max(), np.abs(C).max()))


def _assert_classes(N):
    """Every system a factor of four from each threshold its route depends on."""
    lo, di, up, _, _ = _batch(N)
    for b, kind in enumerate(FAMILIES):
        a, c, mt = _couplings(lo[b], di[b], up[b])
        r = ROUTE[kind]
        where = f"N={N} {kind} ({r}): |A| / tau_A = {a / TAU_A:.3g}, |C| / tau_J = {c / TAU_J:.3g}, m_tau / tau = {mt / TAU:.3g}"
        print(where)
        if r == "onesided":
            assert a <= TAU_A / 4 and c <= TAU_J / 4, where
            assert c >= 4 * TAU_A, where                       # one-sided, not decoupled: the sweeps have work to do
        elif r == "jacobi":
            assert a >= 4 * TAU_A and max(a, c) <= TAU_J / 4, where
        else:
            assert max(a, c) >= 4 * TAU_J, where
            assert mt <= 2.0 ** -33 if r == "short" else mt >= 2.0 ** -29, where


def test_families_sit_a_factor_of_four_from_the_thresholds():
    """Needs no GPU: the CPU classification of every test system at N = 1024, and the conditioning the gate's margin rests
    on (at N = 128 the route is not compiled in and no class is claimed)."""
    _assert_classes(1024)
    for N in (1024, 128):
        lo, di, up, _, _ = _batch(N)
        for b, kind in enumerate(FAMILIES):
            assert _cond(lo[b], di[b], up[b]) <= 13.0, (N, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 128])
def test_four_routes_side_by_side(hip, N):
    if N == 1024:
        _assert_classes(N)
    lo, di, up, rhs, ref = _batch(N)
    sol = _solve(lo, di, up, rhs)
    for b, kind in enumerate(FAMILIES):
        e = rel_l2(sol[b], ref[b])
        print(f"N={N} {kind}: rel-L2 {e:.2e}")
        assert e < SOLVE_TOL, f"N={N} sample {b} ({kind}): {e:.2e}"


# ---- a non-finite sample next to finite ones ------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("what", ["u0", "mu1"])
def test_nonfinite_sample_stays_alone(hip, what):
    """A NaN in u0, or mu1 = inf, in one of the four samples of a workgroup at N = 1024: its couplings are non-finite and
    must fail the ballot.  That sample leaves each step after one iteration with the NONFINITE flag, as the reference and
    the earlier routes have it; its finite neighbours stay at the oracle with no flag."""
    from burgers_hip import fom, lib
    N, nsteps, dt, bad = 1024, 4, 0.025, 2
    X, _ = mesh(N)
    u0 = np.ones((4, N)); mu1 = np.array([5.0, 5.2, 4.5, 5.5]); mu2 = np.array([0.02, 0.02, 0.03, 0.015])
    if what == "u0":
        u0[bad, 517] = np.nan
    else:
        mu1[bad] = np.inf
    r = fom.fom_run(X, u0, mu1, mu2, dt, nsteps)
    torch.cuda.synchronize()
    ho, ito = bc.fom_run(X, u0, mu1, mu2, dt, nsteps)
    it, fl, hist = r.iters.cpu().numpy(), r.flags.cpu().numpy(), r.hist.cpu().numpy()
    assert np.array_equal(it, ito) and (it[bad] == 1).all()
    assert fl.tolist() == [lib.BG_FLAG_NONFINITE if b == bad else 0 for b in range(4)]
    assert not np.isfinite(hist[bad, -1]).all()
    good = [b for b in range(4) if b != bad]
    assert rel_l2(hist[good], ho[good]) <= RUN_TOL


# ---- end to end against the oracles ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("N,graded,B,nsteps", [(1024, False, 4, 6), (1000, False, 4, 6), (768, False, 4, 6),
                                               (2049, False, 2, 3), (300, True, 4, 6)])
def test_fom_run_end_to_end(hip, N, graded, B, nsteps):
    """The time loop against the C oracle: the bench's mesh and step (the route), N = 1000 with padded identity rows,
    N = 768 at the fewest rows per lane that have the route, the workgroup form and a graded mesh, which do not."""
    from burgers_hip import fom
    rng = np.random.default_rng(2100 + N)
    dt = 0.025 * min(1.0, 1024 / N)
    X = _graded(N, rng) if graded else mesh(N)[0]
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    res = fom.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps)
    torch.cuda.synchronize()
    ho, ito = bc.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps)
    e = rel_l2(res.hist.cpu().numpy(), ho)
    print(f"fom_run N={N}{' graded' if graded else ''}: rel-L2 {e:.2e}, iterations {int(ito.sum())}")
    assert e <= RUN_TOL
    assert np.array_equal(res.iters.cpu().numpy(), ito)
    assert not res.flags.cpu().numpy().any()


@pytest.mark.gpu
def test_fd_stepper_end_to_end(hip):
    from burgers_hip import fom
    rng = np.random.default_rng(2178)
    N, B, nsteps, dt = 1024, 4, 3, 0.025
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    res = fom.fd_run(0.0, 100.0, N, np.ones(N), mu1, mu2, dt, nsteps)
    torch.cuda.synchronize()
    assert not res.flags.cpu().numpy().any()
    for b in range(B):
        Uo, ito = br.fd_newton(0.0, 100.0, N, dt, nsteps, np.ones(N), mu1[b], mu2[b], return_iters=True)
        e = rel_l2(res.hist[b].cpu().numpy().T, Uo)
        print(f"fd_run sample {b}: rel-L2 {e:.2e}")
        assert e <= RUN_TOL
        assert np.array_equal(res.iters[b].cpu().numpy(), ito)
