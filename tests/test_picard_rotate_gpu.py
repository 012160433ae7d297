"""The rotated Picard loop of the wave-per-sample FOM kernels (BG_PICARD_ROTATE, csrc/fom.hip): the off-diagonals and
SUPG terms of an iterate are formed right after the update that makes it, ahead of the stopping test, and consumed by
whatever comes next: the next iteration, or the first iteration of the next time step with its new g.  Every case below is
the smallest shape at which that hand-over can go wrong, against the C oracle with the suite's gate: rel-L2 < 1e-10 on the
history and identical iteration counts."""
import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from oracle import burgers_ref_c as bc

pytestmark = pytest.mark.gpu
TOL = 1e-10

MU1 = np.array([4.3, 4.7, 5.0, 5.3, 5.5])
MU2 = np.array([0.016, 0.02, 0.024, 0.027, 0.03])


def _both(X, u0, mu1, mu2, dt, nsteps, **kw):
    """The library's run and the oracle's on the same inputs: (hist, iters, flags), (hist, iters)."""
    from burgers_hip import fom
    r = fom.fom_run(X, u0, mu1, mu2, dt, nsteps, **kw)
    torch.cuda.synchronize()
    kw.pop("form", None)
    return (r.hist.cpu().numpy(), r.iters.cpu().numpy(), r.flags.cpu().numpy()), bc.fom_run(X, u0, mu1, mu2, dt, nsteps, **kw)


def _gate(got, ref):
    (h, it, _), (ho, ito) = got, ref
    assert np.isfinite(ho).all()
    assert np.array_equal(it, ito)
    assert rel_l2(h, ho) < TOL
    for b in range(len(h)):
        assert rel_l2(h[b], ho[b]) < TOL, b


def test_cap_exit_hands_over_the_right_head(hip):
    """N = 128 (two rows per lane, every row real): at dt = 0.2 the first steps end at max_it and the later ones converge,
    so heads formed in front of a cap exit and in front of a converged exit both start a time step."""
    from burgers_hip import lib
    X, _ = mesh(128)
    got, ref = _both(X, np.ones(128), MU1, MU2, 0.2, 12)
    assert (ref[1] == 20).any() and (ref[1] < 20).any()
    _gate(got, ref)
    assert np.array_equal((got[2] & lib.BG_FLAG_HIT_CAP) != 0, (ref[1] >= 20).any(axis=1))


def test_one_iteration_steps(hip):
    """Steps of a single iteration: the head formed at the end of step n is consumed by step n + 1 with a new g, and no
    iteration of step n ever consumed one of its own.  With max_it = 1 every step is such a step; with a small dt and a
    loose tolerance the later steps of some samples converge in one iteration and those of others in two."""
    X, _ = mesh(128)
    got, ref = _both(X, np.ones(128), MU1, MU2, 0.2, 6, max_it=1)
    assert (ref[1] == 1).all()
    _gate(got, ref)
    got, ref = _both(X, np.ones(128), MU1, MU2, 1e-3, 12, tol=1e-3)
    assert (ref[1][:, 1:] == 1).any() and (ref[1][:, 1:] == 2).any()
    _gate(got, ref)


@pytest.mark.parametrize("N,graded", [(65, False), (300, True), (64, False)])
def test_padded_rows_graded_mesh_and_one_row_per_lane(hip, N, graded):
    """N = 65: two rows per lane with 63 padded rows; N = 300 on a graded mesh: the general assembly in its two halves,
    five rows per lane, padded; N = 64: one row per lane, where the head has no interior lo[j + 1]."""
    rng = np.random.default_rng(7700 + N)
    X, _ = mesh(N)
    E = 0.0
    if graded:
        w = rng.uniform(0.7, 1.3, N - 1)
        X = np.concatenate([[0.0], np.cumsum(w)]) * (100.0 / w.sum())
        E = 0.004
    u0 = 1.0 + 0.3 * np.sin(np.outer(rng.uniform(0.5, 2.0, 5), X / 100 * np.pi))
    dt = min(0.5, 0.05 * 512 / N)
    from burgers_hip import lib
    got, ref = _both(X, u0, MU1, MU2, dt, 8, E=E)
    _gate(got, ref)
    assert np.array_equal(got[2], np.where((ref[1] >= 20).any(axis=1), lib.BG_FLAG_HIT_CAP, 0))


@pytest.mark.parametrize("nsteps", [0, 1])
def test_no_step_and_one_step(hip, nsteps):
    """The head formed ahead of the time loop exists even when no step (or one step) follows: nothing consumes it
    wrongly and nothing is written past the sample's history (the row behind the result keeps its fill)."""
    from burgers_hip import fom
    N, B = 128, 5
    X, _ = mesh(N)
    fill = -777.0
    hist = torch.full((B + 1, nsteps + 1, N), fill, dtype=torch.float64, device="cuda")
    iters = torch.full((B + 1, nsteps), -7, dtype=torch.int32, device="cuda")
    flags = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    fom.fom_run(X, np.ones(N), MU1, MU2, 0.05, nsteps, out=fom.FomResult(hist[:B], iters[:B], flags[:B]))
    torch.cuda.synchronize()
    ho, ito = bc.fom_run(X, np.ones(N), MU1, MU2, 0.05, nsteps)
    assert (hist[B] == fill).all() and (iters[B] == -7).all() and int(flags[B]) == -7
    assert np.array_equal(iters[:B].cpu().numpy(), ito) and (flags[:B] == 0).all()
    assert np.array_equal(hist[:B, 0].cpu().numpy(), np.ones((B, N)))
    assert rel_l2(hist[:B].cpu().numpy(), ho) < TOL


def test_head_of_a_nonfinite_state_changes_no_flag_and_no_count(hip):
    """The inputs of test_nonfinite_state_exits_like_the_reference: the head of a NaN state is formed like any other,
    ahead of the test that ends the loop; counts stay the oracle's, the flag stays on the NaN sample alone."""
    from burgers_hip import lib
    X, _ = mesh(256)
    u0 = np.ones((2, 256)); u0[1, 40] = np.nan
    from burgers_hip import fom
    r = fom.fom_run(X, u0, [5.0, 5.0], [0.02, 0.02], 0.05, 6)
    torch.cuda.synchronize()
    ho, ito = bc.fom_run(X, u0, [5.0, 5.0], [0.02, 0.02], 0.05, 6)
    it, fl = r.iters.cpu().numpy(), r.flags.cpu().numpy()
    assert np.array_equal(it, ito) and (it[1] == 1).all()
    assert fl[1] == lib.BG_FLAG_NONFINITE and fl[0] == 0
    assert rel_l2(r.hist[0].cpu().numpy(), ho[0]) < TOL


def test_workgroup_form_keeps_its_order(hip):
    """N = 2049: one workgroup per sample, whose loop is not rotated."""
    rng = np.random.default_rng(2049)
    X, _ = mesh(2049)
    mu1 = rng.uniform(4.25, 5.5, 2); mu2 = rng.uniform(0.015, 0.03, 2)
    got, ref = _both(X, np.ones(2049), mu1, mu2, 0.05 * 512 / 2049, 6)
    _gate(got, ref)
    assert (got[2] == 0).all()


def test_flagship_instantiation(hip):
    """fom_fused_kernel<16, true, true, false>: N = 1024 exactly, the bench's dt."""
    rng = np.random.default_rng(20251121)
    X, _ = mesh(1024)
    mu1 = rng.uniform(4.25, 5.5, 8); mu2 = rng.uniform(0.015, 0.03, 8)
    got, ref = _both(X, np.ones(1024), mu1, mu2, 0.025, 20, form="wave")
    _gate(got, ref)
    assert (got[2] == 0).all()
