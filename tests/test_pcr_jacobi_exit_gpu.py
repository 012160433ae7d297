"""The Jacobi exit of the interface PCR (csrc/fom_device.hpp, pcr64): after its stride-1 step a wave whose couplings are all
<= tau_J = 2^-9 closes the system A x[j-2] + x[j] + C x[j+2] = D by six sweeps x <- D - A x[j-2] - C x[j+2] from x = D
("jacobi"); every other wave goes on as before, to the exit against tau = 2^-31 after two more steps ("short") or through all
six steps ("full").  The exit is compiled in where a lane owns at least BG_PCR_JACOBI_MIN_ROWS = 12 rows (N = 1024: 16, the
workgroup solver at N = 2049: 12); at N = 128 (2 rows) every wave takes the earlier route, and the same systems pin that.

Which route a system takes is decided here on the CPU by a NumPy restatement of the Wang partition and the PCR steps, with a
factor of four to either side of each threshold, so that rounding differences between host and device cannot flip a case and
no case can silently stop covering its route.  The workgroup solver (N > 1536) runs two PCR steps over its 256 equations before
pcr64, so its thresholds are met two steps later.

Gates.  Six sweeps against a longdouble solve: 2^-50 max|X|, the 2^-56 truncation ((2 tau_J)^7 / (1 - 2 tau_J)) plus the two
FMA roundings of the last sweep (2 * 2^-53 max|X|, the earlier ones damped by 2^-8 per sweep), with a factor of four to spare.
Solver: rel-L2 < 1e-12 against the dense solve (condition numbers <= 13, so the reference is orders inside it).  Time loops:
rel-L2 <= 1e-10 and identical iteration counts against the oracles, no flags."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import torch

from conftest import mesh, rel_l2
from oracle import burgers_ref as br
from oracle import burgers_ref_c as bc

TAU_J = 2.0 ** -9
TAU = 2.0 ** -31
SWEEPS = 6
SWEEP_TOL = 2.0 ** -50
SOLVE_TOL = 1e-12
RUN_TOL = 1e-10
WAVE_ROWS = (1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 16, 24)           # dispatch_r of csrc/fom.hip, 64 lanes
WIDE_ROWS = (2, 4, 8, 12, 16, 24, 32)                          # dispatch_wide, 256 threads, N > 1536
SIZES = (1024, 128, 2049)
FAMILIES = ("dominant", "patch", "skew", "dominant")           # four waves: one workgroup of the wave-per-system solver
# The route each family is asserted to take.  One wave per system: one family per route.  The workgroup solver at N = 2049
# tests against tau_J three PCR steps behind 12 rows per thread, 96 rows apart, and against tau 384 rows apart; with a
# condition number <= 13 no coupling reaches that far (the skew family, 0.905 per row, arrives at tau_J / 16), so there
# every family is asserted on the jacobi route and the other two routes are covered by the wave sizes.
ROUTE = {1024: {"dominant": "jacobi", "patch": "short", "skew": "full"},
         128: {"dominant": "jacobi", "patch": "short", "skew": "full"},
         2049: {"dominant": "jacobi", "patch": "jacobi", "skew": "jacobi"}}


def _shift(v, s):
    """v[..., j - s] at j, zero outside (s < 0: v[..., j + |s|]): the zero fill of the DPP moves."""
    out = np.zeros_like(v)
    if s > 0:
        out[..., s:] = v[..., :-s]
    else:
        out[..., :s] = v[..., -s:]
    return out


def _fma(a, b, c):
    """Elementwise fma with one rounding: exact in rationals, then rounded to nearest even by float()."""
    return np.vectorize(lambda x, y, z: float(Fraction(x) * Fraction(y) + Fraction(z)), otypes=[np.float64])(a, b, c)


def sweeps_fma(A, C, D, sweeps=SWEEPS):
    """pcr_jacobi_sweep of csrc/fom_device.hpp, `sweeps` times from x = D: fma(-x[j+2], C, fma(-x[j-2], A, D))."""
    x = D
    for _ in range(sweeps):
        x = _fma(-_shift(x, -2), C, _fma(-_shift(x, 2), A, D))
    return x


def _solve_distance2(A, C, D):
    """x of A x[j-2] + x[j] + C x[j+2] = D in longdouble: elimination inside the band, without pivoting (the matrix is
    strictly diagonally dominant)."""
    n = len(D)
    M = np.eye(n, dtype=np.longdouble)
    for j in range(n):
        if j >= 2:
            M[j, j - 2] = A[j]
        if j + 2 < n:
            M[j, j + 2] = C[j]
    r = D.astype(np.longdouble)
    for k in range(n - 2):                                     # the only entry below the diagonal of column k: row k + 2
        f = M[k + 2, k] / M[k, k]
        M[k + 2] -= f * M[k]
        r[k + 2] -= f * r[k]
    x = np.zeros(n, dtype=np.longdouble)
    for k in range(n - 1, -1, -1):
        x[k] = (r[k] - M[k, k + 1:] @ x[k + 1:]) / M[k, k]
    return x


def _coupling_cases(scale):
    """64-equation systems with couplings on [-scale, scale]: random with the end points hit, zeros, all at +scale,
    alternating signs."""
    rng = np.random.default_rng(906)
    n = 64
    rnd = [rng.uniform(-scale, scale, n) for _ in range(4)]
    rnd[0][::7] = scale; rnd[1][3::5] = -scale; rnd[2][::4] = 0.0; rnd[3][1::3] = 0.0
    alt = scale * (-1.0) ** np.arange(n)
    cases = {"random": (rnd[0], rnd[1]), "zeros mixed in": (rnd[2], rnd[3]), "all zero": (np.zeros(n), np.zeros(n)),
             "all at +scale": (np.full(n, scale), np.full(n, scale)), "alternating": (alt, -alt),
             "alternating by pairs": (scale * (-1.0) ** (np.arange(n) // 2), scale * (-1.0) ** (np.arange(n) // 2 + 1))}
    return {k: (a, c, rng.standard_normal(n)) for k, (a, c) in cases.items()}


def test_six_sweeps_against_longdouble_solve():
    for name, (A, C, D) in _coupling_cases(TAU_J).items():
        x = sweeps_fma(A, C, D)
        ref = _solve_distance2(A, C, D)
        err = float(np.abs(x.astype(np.longdouble) - ref).max() / np.abs(ref).max())
        print(f"{name}: max|x - ref| / max|ref| = {err:.2e} ({err / SWEEP_TOL:.3f} of the gate)")
        assert err <= SWEEP_TOL, name


def test_threshold_is_not_decorative():
    """At 4 tau_J six sweeps leave (8 tau_J)^7 ~ 2^-42: the gate must see it."""
    A, C, D = _coupling_cases(4.0 * TAU_J)["all at +scale"]
    x = sweeps_fma(A, C, D)
    ref = _solve_distance2(A, C, D)
    err = float(np.abs(x.astype(np.longdouble) - ref).max() / np.abs(ref).max())
    print(f"couplings at 4 tau_J: {err:.2e} ({err / SWEEP_TOL:.1f} of the gate)")
    assert err > SWEEP_TOL


# ---- the Wang partition and the PCR steps, restated over a leading batch axis ------------------------------------------

def _partition(N):
    """(threads, rows per thread, PCR steps in front of pcr64) of bg_tridiag_solve / the time loops at N."""
    if N > 64 * WAVE_ROWS[-1]:
        return 256, next(r for r in WIDE_ROWS if N <= 256 * r), 2
    return 64, next(r for r in WAVE_ROWS if N <= 64 * r), 0


def wang_interface(lo, di, up, rhs):
    """wang_reduce / wang_interface of csrc/fom_device.hpp with exact divisions, over (..., N): thread p owns rows
    [pR, pR + R), rows >= N are identity rows.  Returns the normalised interface equations (A, C, D), each (..., threads),
    and what wang_finish needs.  Inside, the row of a thread is the leading axis."""
    N = di.shape[-1]
    T, R, _ = _partition(N)
    assert R > 1
    shp = di.shape[:-1]
    def lay(a, fill):
        out = np.full(shp + (T * R,), fill)
        out[..., :N] = a
        return np.ascontiguousarray(np.moveaxis(out.reshape(shp + (T, R)), -1, 0))
    l, d, u, r = lay(lo, 0.0), lay(di, 1.0), lay(up, 0.0), lay(rhs, 0.0)
    f = l.copy(); inv = np.empty_like(d); g = np.zeros_like(d)
    dp = d[0]
    inv[0] = 1.0 / dp
    for j in range(1, R):                                      # sub-diagonal downwards: left spike f, 1 / pivot
        m = l[j] * inv[j - 1]
        dp = d[j] - m * u[j - 1]
        inv[j] = 1.0 / dp
        r[j] -= m * r[j - 1]
        f[j] = -m * f[j - 1]
    g[R - 2] = u[R - 2]
    for j in range(R - 3, -1, -1):                             # super-diagonal upwards from row R-3: right spike g
        t = u[j] * inv[j + 1]
        r[j] -= t * r[j + 1]
        f[j] -= t * f[j + 1]
        g[j] = -t * g[j + 1]
    F0, G0, R0 = (_shift(a[0] * inv[0], -1) for a in (f, g, r))
    ul = u[R - 1]
    B = dp - ul * F0
    return f[R - 1] / B, -(ul * G0) / B, (r[R - 1] - ul * R0) / B, (f, inv, g, r, N)


def wang_finish(ctx, X):
    f, inv, g, r, N = ctx
    sol = (r - f * _shift(X, 1) - g * X) * inv
    sol[-1] = X
    sol = np.moveaxis(sol, 0, -1)
    return sol.reshape(sol.shape[:-2] + (-1,))[..., :N]


def pcr_step(A, C, D, s):
    Bn = 1.0 - _shift(C, s) * A - _shift(A, -s) * C
    Dn = (D - _shift(D, s) * A - _shift(D, -s) * C) / Bn
    return -(_shift(A, s) * A) / Bn, -(_shift(C, -s) * C) / Bn, Dn


def couplings(lo, di, up):
    """(m_J, m_tau): max(|A|, |C|) where pcr64 tests against tau_J (after its stride-1 step) and against tau (after its
    stride-4 step); the workgroup solver has two steps over its 256 equations in front of pcr64."""
    _, _, pre = _partition(len(di))
    A, C, D, _ = wang_interface(lo, di, up, np.zeros_like(di))
    out = []
    for k in range(pre + 3):
        A, C, D = pcr_step(A, C, D, 1 << k)
        out.append(float(max(np.abs(A).max(), np.abs(C).max())))
    return out[pre], out[pre + 2]


# ---- the flagship workload sits on the exit -----------------------------------------------------------------------------

def _assemble_uniform(h, dt, U0, g, fsum, mu1):
    """The Picard system of the reference on a uniform mesh in closed form (csrc/fom_device.hpp, header; E = 0):
    A = M + dt C(U0) with row 0 <- e0, b = g - dt S(U0) with b0 = mu1, g = M u^n + dt F; fsum = f(gp1) + f(gp2) per
    element.  Returns lo, di, up and the right-hand side b - A U0 of the increment, over (B, N)."""
    ul, ur = U0[:, :-1], U0[:, 1:]
    c1, c2 = (2.0 * ul + ur) / 6.0, (ul + 2.0 * ur) / 6.0      # convection: E_ll = -c1, E_lr = c1, E_rl = -c2, E_rr = c2
    ubar = 0.5 * (ul + ur)
    se = 0.5 * h / (2.0 * np.maximum(np.abs(ubar), 1.0e-10)) * (ubar * (ur - ul) / h - 0.5 * fsum)
    lo = np.zeros_like(U0); di = np.empty_like(U0); up = np.zeros_like(U0); b = g.copy()
    lo[:, 1:] = h / 6.0 - dt * c2
    up[:, :-1] = h / 6.0 + dt * c1
    di[:, 1:-1] = 2.0 * h / 3.0 + dt * (c2[:, :-1] - c1[:, 1:])
    di[:, -1] = h / 3.0 + dt * c2[:, -1]
    b[:, 1:] -= dt * se
    b[:, :-1] += dt * se
    lo[:, 0] = 0.0; di[:, 0] = 1.0; up[:, 0] = 0.0; b[:, 0] = mu1
    return lo, di, up, b - br.tridiag_matvec(lo, di, up, U0)


def test_flagship_sits_on_the_exit():
    """bench.py's mesh and step at two corners of its parameter box, every Picard iteration of 500 steps: assembly, Wang
    partition, stride-1 step and six sweeps as the solve.  The largest coupling after the stride-1 step stays a factor of
    two under tau_J (9.28e-4 measured), and the iteration counts are the C oracle's."""
    N, dt, nsteps, tol, max_it = 1024, 0.025, 500, 1e-6, 20
    X, _ = mesh(N)
    h = X[1] - X[0]
    mu1 = np.array([5.5, 4.25]); mu2 = np.array([0.03, 0.015])
    M3 = br.mass_tridiag(X)
    dtF = dt * br.forcing_vector(X, mu2)
    gp = (1.0 + np.array([-1.0, 1.0])[:, None] / np.sqrt(3.0)) / 2.0
    fsum = sum(0.02 * np.exp(mu2[:, None] * ((1.0 - w) * X[:-1] + w * X[1:])) for w in gp)
    Un = np.ones((2, N))
    iters = np.zeros((2, nsteps), dtype=np.int32)
    worst = 0.0
    for n in range(nsteps):
        g = br.tridiag_matvec(*M3, Un) + dtF
        U0 = Un
        active = np.ones(2, dtype=bool)
        while active.any():
            lo, di, up, rhs = _assemble_uniform(h, dt, U0, g, fsum, mu1)
            A, C, D, ctx = wang_interface(lo, di, up, rhs)
            A, C, D = pcr_step(A, C, D, 1)
            worst = max(worst, float(np.abs(A[active]).max()), float(np.abs(C[active]).max()))
            x = D
            for _ in range(SWEEPS):
                x = D - A * _shift(x, 2) - C * _shift(x, -2)
            dU = wang_finish(ctx, x)
            U1 = U0 + dU
            err = np.linalg.norm(dU, axis=1) / np.linalg.norm(U1, axis=1)
            U0 = np.where(active[:, None], U1, U0)
            iters[active, n] += 1
            active = active & (err > tol) & (iters[:, n] < max_it)
        Un = U0
    print(f"largest coupling after the stride-1 step: {worst:.3e} = tau_J / {TAU_J / worst:.2f}; "
          f"iterations {iters.sum(axis=1).tolist()}")
    assert worst <= TAU_J / 2
    ho, ito = bc.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps)
    assert np.array_equal(iters, ito)
    assert rel_l2(Un, ho[:, -1]) <= RUN_TOL


# ---- solver entry: three routes side by side ----------------------------------------------------------------------------

def _family(kind, N, rng):
    """One system of a family; every family draws the same number of variates, so the seed fixes all of them.
    dominant: diagonally dominant everywhere.  skew: (-1/2, 1/10, 1/2) everywhere, the slowest decay of the couplings that a
    condition number <= 13 allows (0.905 per row).  patch: skew on the rows of a few neighbouring threads, dominant
    elsewhere: the product of neighbouring couplings that a PCR step forms is large inside the patch where pcr64 tests
    against tau_J and has left it two steps later."""
    _, R, pre = _partition(N)
    dom =(rng.uniform(-0.02, 0.02, N), rng.uniform(0.9, 1.1, N), rng.uniform(-0.02, 0.02, N))
    skw = (-0.5 * rng.uniform(0.95, 1.05, N), rng.uniform(0.08, 0.12, N), 0.5 * rng.uniform(0.95, 1.05, N))
    if kind == "dominant":
        lo, di, up = dom
    elif kind == "skew":
        lo, di, up = skw
    else:
        span = 3 << pre                                        # threads in the patch: 1.5 times the reach of the step in
        t0 = -(-N // R) // 3                                   # front of the test against tau_J, under that of tau's
        patch = np.zeros(N, dtype=bool)
        patch[t0 * R:(t0 + span) * R] = True
        lo, di, up = (np.where(patch, s, d) for s, d in zip(skw, dom))
    lo = lo.copy(); up = up.copy()
    lo[0] = 0.0; up[-1] = 0.0
    return lo, di.copy(), up, rng.standard_normal(N)


@functools.lru_cache(maxsize=None)
def _batch(N):
    """Four systems, one workgroup of the wave-per-system solver, and their dense solutions.  Computed once per size;
    the arrays are read-only."""
    rng = np.random.default_rng(9000 + N)
    sys_ = [_family(k, N, rng) for k in FAMILIES]
    lo, di, up, rhs = (np.stack([s[i] for s in sys_]) for i in range(4))
    ref = np.stack([np.linalg.solve(br.tridiag_dense(lo[b], di[b], up[b]), rhs[b]) for b in range(len(FAMILIES))])
    for a in (lo, di, up, rhs, ref):
        a.setflags(write=False)
    return lo, di, up, rhs, ref


def _cond(lo, di, up):
    """2-norm condition number of the dense matrix, from the extreme eigenvalues of the pentadiagonal A^T A (squaring costs
    nothing at condition numbers of ten; an SVD of the 2049 x 2049 matrices would take seconds)."""
    S = sp.diags([lo[1:], di, up[:-1]], [-1, 0, 1], format="csr")
    G = (S.T @ S).todia()
    n = len(di)
    ab = np.zeros((3, n))
    for k in range(3):
        ab[2 - k, k:] = G.diagonal(k)
    ev = sla.eigvals_banded(ab, lower=False)
    return float(np.sqrt(ev[-1] / ev[0]))


def _assert_classes(N):
    lo, di, up, _, _ = _batch(N)
    for b, kind in enumerate(FAMILIES):
        mj, mt = couplings(lo[b], di[b], up[b])
        route = ROUTE[N][kind]
        where = f"N={N} {kind} ({route}): m_J / tau_J = {mj / TAU_J:.3g}, m_tau / tau = {mt / TAU:.3g}"
        if route == "jacobi":
            assert mj <= TAU_J / 4, where
        else:
            assert mj >= 4 * TAU_J, where
            assert mt <= 2.0 ** -33 if route == "short" else mt >= 2.0 ** -29, where


@pytest.mark.parametrize("N", SIZES)
def test_families_sit_a_factor_of_four_from_the_thresholds(N):
    """Needs no GPU: the CPU classification of every test system, and the conditioning the gate's margin rests on."""
    _assert_classes(N)
    lo, di, up, _, _ = _batch(N)
    for b in range(3):
        assert _cond(lo[b], di[b], up[b]) <= 13.0, (N, FAMILIES[b])


def _solve(lo, di, up, rhs):
    from burgers_hip import fom
    sol = fom.tridiag_solve(*[torch.tensor(np.asarray(a), device="cuda") for a in (lo, di, up, rhs)])
    torch.cuda.synchronize()
    return sol.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_three_routes_side_by_side(hip, N):
    _assert_classes(N)
    lo, di, up, rhs, ref = _batch(N)
    sol = _solve(lo, di, up, rhs)
    for b, kind in enumerate(FAMILIES):
        e = rel_l2(sol[b], ref[b])
        print(f"N={N} {kind} ({ROUTE[N][kind]}): rel-L2 {e:.2e}")
        assert e < SOLVE_TOL, f"N={N} sample {b} ({kind}, {ROUTE[N][kind]}): {e:.2e}"


@pytest.mark.gpu
@pytest.mark.parametrize("bad,field", [(0, "lo"), (0, "rhs"), (1, "di"), (2, "rhs"), (3, "di")])
def test_nonfinite_sample_stays_alone(hip, bad, field):
    """A NaN in one sample (in a coefficient, where it makes the couplings NaN and must fail the test against tau_J, or in
    the right-hand side, where the sweeps carry it): that sample comes back non-finite, its three neighbours in the
    workgroup still meet the gate."""
    N = 1024
    lo, di, up, rhs, ref = _batch(N)
    arrs = {"lo": lo.copy(), "di": di.copy(), "up": up.copy(), "rhs": rhs.copy()}
    arrs[field][bad, 517] = np.nan
    sol = _solve(arrs["lo"], arrs["di"], arrs["up"], arrs["rhs"])
    assert not np.isfinite(sol[bad]).all()
    for b, kind in enumerate(FAMILIES):
        if b != bad:
            assert rel_l2(sol[b], ref[b]) < SOLVE_TOL, f"sample {b} ({kind}) next to a NaN in sample {bad}"


# ---- end to end against the oracles -------------------------------------------------------------------------------------

def _graded(N, rng):
    w = rng.uniform(0.7, 1.3, N - 1)
    return np.concatenate([[0.0], np.cumsum(w)]) * (100.0 / w.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("N,graded", [(1024, False), (1000, False), (300, True), (2049, False)])
def test_fom_run_end_to_end(hip, N, graded):
    """The time loop against the C oracle: the bench's mesh and step (jacobi exit), N = 1000 with padded identity rows,
    a graded mesh at 5 rows per lane and the workgroup form."""
    from burgers_hip import fom
    rng = np.random.default_rng(1900 + N)
    B, nsteps, dt = 4, 12, 0.025 * min(1.0, 1024 / N)
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
    rng = np.random.default_rng(1978)
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
