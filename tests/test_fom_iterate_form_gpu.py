"""The iterate form of the Picard loop (csrc/fom.hip, fom_sample; csrc/fom_device.hpp, assemble_p2<.., ITER>): a time step
starts with lean iterations, which solve A(u) v = b for the new iterate v, not A(u) du = b - A(u) u for the increment
(du = v - u serves the stopping norm only), and goes over to the increment once the stopping test is missed by no more than
a factor of 16.  The two forms give the same v in exact arithmetic, and the matrix is the same bit for bit, but in a lean
iteration the solve's rounding and the truncation of the PCR exits are relative to |u| and not to |du|.  With
max_it = 1 every step is one lean iteration: that case pins the form on its own.

Gate, the project's own: iteration counts and flags identical to the C oracle (oracle.burgers_ref_c.fom_run, which keeps
the increment form), rel-L2 of the whole history <= 1e-10.  The cases are the small ones on which a CPU restatement of the
iterate form, each solve disturbed by 1e-13 relative, kept every count of the oracle: the mu pairs are the first samples of
the bench's draw, and one case per instantiation family the loop is compiled into."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from oracle import burgers_ref as br
from oracle import burgers_ref_c as bc

pytestmark = pytest.mark.gpu
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def _mu(B):
    import bench
    mu1, mu2 = bench.mu_shard(1024, 1, 0)
    mu1, mu2 = mu1[:B].copy(), mu2[:B].copy()
    mu1.setflags(write=False); mu2.setflags(write=False)
    return mu1, mu2


def _graded(N):
    w = np.random.default_rng(300).uniform(0.7, 1.3, N - 1)
    return np.concatenate([[0.0], np.cumsum(w)]) * (100.0 / w.sum())


# (id, N, graded, B, nsteps, E, dt)
CASES = [
    ("n1024_flagship_r16_full", 1024, False, 8, 12, 0.0, 0.025),
    ("n1000_masked", 1000, False, 8, 12, 0.0, 0.025),
    ("n128_fast_convergence", 128, False, 8, 20, 0.0, 0.05),
    ("n128_diffusive", 128, False, 8, 20, 1.0, 0.05),
    ("n65", 65, False, 8, 20, 0.2, 0.05),
    ("n2049_workgroup", 2049, False, 4, 6, 0.0, 0.0125),
    ("n300_graded", 300, True, 8, 12, 0.0, 0.05),
]


@pytest.mark.parametrize("name,N,graded,B,nsteps,E,dt", CASES, ids=[c[0] for c in CASES])
def test_time_loop_against_the_oracle(hip, name, N, graded, B, nsteps, E, dt):
    from burgers_hip import fom
    X = _graded(N) if graded else mesh(N)[0]
    mu1, mu2 = _mu(B)
    res = fom.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps, E=E)
    torch.cuda.synchronize()
    ho, ito = bc.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps, E=E)
    h, it, fl = res.hist.cpu().numpy(), res.iters.cpu().numpy(), res.flags.cpu().numpy()
    e = rel_l2(h, ho)
    worst = max(rel_l2(h[b], ho[b]) for b in range(B))
    print(f"{name}: rel-L2 {e:.2e}, worst sample {worst:.2e}, iterations {int(ito.sum())}, "
          f"steps that ran into the cap {int((ito >= 20).sum())}")
    assert np.array_equal(it, ito)
    assert np.array_equal(fl, np.where((ito >= 20).any(axis=1), hip.BG_FLAG_HIT_CAP, 0))
    assert e <= TOL and worst <= TOL


def test_traced_equals_untraced_and_the_reference_errors(hip):
    """The TRACE instantiation takes the same form: history, counts and flags equal to the untraced run bit for bit, and
    the error of every iteration, ||v - u|| / ||v||, is the reference's ||dU|| / ||U1||."""
    from burgers_hip import fom
    N, B, nsteps, dt = 1024, 4, 6, 0.025
    X, _ = mesh(N)
    mu1, mu2 = _mu(B)
    a = fom.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps)
    t = fom.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps, trace=True)
    torch.cuda.synchronize()
    assert torch.equal(a.hist, t.hist) and torch.equal(a.iters, t.iters) and torch.equal(a.flags, t.flags)
    errs = t.errs.cpu().numpy()
    for b in range(B):
        _, it, eo = br.fom_burgers(X, dt, nsteps, np.ones(N), mu1[b], 0.0, mu2[b], return_iters=True, return_errs=True)
        ran = ~np.isnan(eo)
        assert np.array_equal(a.iters[b].cpu().numpy(), it)
        assert np.array_equal(np.isnan(errs[b]), ~ran)
        print(f"sample {b}: worst relative deviation of a traced error {np.abs(errs[b][ran] / eo[ran] - 1.0).max():.2e}, "
              f"smallest error {eo[ran].min():.2e}")
        assert np.allclose(errs[b][ran], eo[ran], rtol=1e-6, atol=0.0)


def test_one_iteration_per_step(hip):
    """max_it = 1: one solve per step and no second look at it.  Every count is 1, every sample is flagged as capped and
    the history is the oracle's."""
    from burgers_hip import fom
    N, B, nsteps, dt = 1024, 8, 12, 0.025
    X, _ = mesh(N)
    mu1, mu2 = _mu(B)
    res = fom.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps, max_it=1)
    torch.cuda.synchronize()
    ho, ito = bc.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps, max_it=1)
    assert (ito == 1).all() and np.array_equal(res.iters.cpu().numpy(), ito)
    assert (res.flags.cpu().numpy() == hip.BG_FLAG_HIT_CAP).all()
    e = rel_l2(res.hist.cpu().numpy(), ho)
    print(f"max_it = 1: rel-L2 {e:.2e}")
    assert e <= TOL


def test_diagnostic_assembly_keeps_the_residual_form(hip):
    """bg_fom_assemble still returns rhs = b - A(u_k) u_k (the ABI's contract), at the tolerances of
    test_fom_gpu.py::test_assembly_matches_oracle; a right-hand side that were b alone would be off by O(|A u|)."""
    from burgers_hip import fom
    N, B, dt, E = 1024, 6, 0.03, 0.02
    rng = np.random.default_rng(N)
    X, _ = mesh(N)
    uk = 1.0 + 4.0 * rng.random((B, N)); un = 1.0 + 4.0 * rng.random((B, N))
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    lo, di, up, rhs = [t.cpu().numpy() for t in fom.fom_assemble(X, uk, un, mu1, mu2, dt, E=E)]
    M3, K3 = br.mass_tridiag(X), br.diffusion_tridiag(X)
    for b in range(B):
        l, d, u = br.system_tridiag(M3, K3, br.convection_tridiag(X, uk[b]), dt, E)
        bb = br.tridiag_matvec(*M3, un[b]) + dt * br.forcing_vector(X, mu2[b]) - dt * br.supg_term(X, uk[b], mu2[b])
        bb[0] = mu1[b]
        r = bb - br.tridiag_matvec(l, d, u, uk[b])
        scale = np.abs(d).max()
        assert np.abs(lo[b] - l).max() < 1e-13 * scale
        assert np.abs(di[b] - d).max() < 1e-13 * scale
        assert np.abs(up[b] - u).max() < 1e-13 * scale
        assert np.abs(rhs[b] - r).max() < 1e-12 * max(1.0, np.abs(r).max())
        assert np.abs(rhs[b] - bb).max() > 1e-3 * np.abs(bb).max()       # and it is not b
