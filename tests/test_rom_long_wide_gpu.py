"""bg_rom_run_long_wide: the device-side POD-PROM time loop for meshes of 513 .. 1024 nodes and bases of 41 .. 96 modes
(csrc/rom_long_wide.hip), against the oracle and the library path (the default route for N > 512).
reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785.

Bases: the leading r left singular vectors of the FOM snapshots (oracle, C) of the 3 x 3 training grid, 200 steps."""
import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from loop_cases import (check_order_entries_skipped, check_plan_reuse_restart_and_refusals, check_pod_vs_oracle, draw,
                        max_multiplier, pod_basis, same)
from oracle import burgers_ref as br

pytestmark = pytest.mark.gpu
TOL = 1e-10
ENTRY = "bg_rom_run_long_wide"


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("N,dt,r", [(1024, 0.025, 96), (1024, 0.025, 41), (600, 0.04, 64), (513, 0.05, 77)])
def test_parity_with_the_oracle(hip, N, dt, r, proj):
    """N = 513: a last slab of one mesh row; N = 600: a ragged last slab; r = 41: one live column in its block; r = 77: no
    multiple of 4; r = 96 at N = 1024: the full kernel."""
    from burgers_hip import rom
    X, Phi = pod_basis(N, dt, r)
    mu1, mu2 = draw(6)
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, 8, Phi, projection=proj, long_wide=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.redone == 0
    check_pod_vs_oracle(res, X, dt, 8, mu1, mu2, Phi, proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", ["diffusion", "nonuniform"])
def test_diffusion_and_nonuniform_mesh(hip, case, proj):
    """The guard decides who did the work: a sample whose unpivoted elimination meets a multiplier above 1 comes back
    marked and is redone through the library path.  The oracle's own multiplier says which it must be; an input whose
    multiplier lies within 1 % of the guard's threshold decides nothing and fails the test."""
    from burgers_hip import lib, rom
    N, dt, nT = 1024, 0.025, 8
    E, seed = (0.01, None) if case == "diffusion" else (0.0, 21)
    X, Phi = pod_basis(N, dt, 96, E=E, seed=seed)
    assert lib.mesh_is_uniform(X) == (seed is None)
    mu1, mu2 = draw(3, seed=5)
    worst = max_multiplier(X, dt, nT, mu1[0], mu2[0], Phi, proj, E)
    print(f"{case} {proj}: largest unpivoted multiplier of sample 0: {worst:.3f}")
    assert worst >= 1.01 or worst <= 0.99, f"unsuitable input: multiplier {worst} too close to the guard's threshold"
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, projection=proj, E=E, long_wide=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    print(f"{case} {proj}: redone {res.redone} of {len(mu1)}")
    assert res.redone == (len(mu1) if worst >= 1.01 else 0)
    check_pod_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, proj, E=E)


def test_batch_behaviour(hip):
    """B = 300 (more samples than workgroups) on N = 1024, r = 96, LSPG: a sample alone, the sample order of the persistent
    loop and the hand-back of every sample must not change what the batch computes."""
    from burgers_hip import lib, rom
    N, dt, nT, B = 1024, 0.025, 3, 300
    X, Phi = pod_basis(N, dt, 96)
    mu1, mu2 = draw(B)
    p = rom.PROJ["lspg"]
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, projection="LSPG", long_wide=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.redone == 0
    assert not bool(res.flags.any()) and bool((res.info == 0).all())
    alone = rom.pod_prom_run_long_wide(X, np.ones(N), mu1[299:], mu2[299:], dt, nT, res.plan, p)
    plain = rom.pod_prom_run_long_wide(X, np.ones(N), mu1, mu2, dt, nT, res.plan, p, balance=False)
    torch.cuda.synchronize()
    assert alone.path == ENTRY and plain.path == ENTRY
    assert torch.equal(alone.hist[0], res.hist[299]) and torch.equal(alone.iters[0], res.iters[299])
    same(plain, res)
    pick = list(range(0, B, B // 8))[:8]
    ref = rom.pod_prom_run(X, np.ones(N), mu1[pick], mu2[pick], dt, nT, Phi, projection="LSPG")
    assert ref.path == "library"
    fh, lh = res.hist[pick].cpu().numpy(), ref.hist.cpu().numpy()
    worst = max(rel_l2(fh[s], lh[s]) for s in range(len(pick)))
    print(f"worst rel-L2 against the library path over {len(pick)} samples {worst:.2e}")
    assert worst <= TOL
    forced = rom.pod_prom_run_long_wide(X, np.ones(N), mu1[:5], mu2[:5], dt, nT, res.plan, p, options=lib.BG_OPT_FORCE_PIVOTED)
    torch.cuda.synchronize()
    assert forced.path == ENTRY and forced.redone == 5 and bool((forced.info == 0).all())
    assert torch.equal(forced.iters, res.iters[:5])
    fo, ba = forced.hist.cpu().numpy(), res.hist[:5].cpu().numpy()
    worst = max(rel_l2(fo[s], ba[s]) for s in range(5))
    print(f"worst rel-L2 of the handed-back samples against the batch {worst:.2e}")
    assert worst <= 1e-11


def test_plan_reuse_and_refusals(hip, monkeypatch):
    from burgers_hip import rom
    X, Phi = pod_basis(1024, 0.025, 96)
    check_plan_reuse_restart_and_refusals(monkeypatch, rom.pod_prom_run_long_wide, rom.LongWidePodPlan, ENTRY, X, 0.025, Phi, other_r=64,
                                          too_long=(1025, 48))


def test_order_entries_outside_the_batch_are_skipped(hip):
    from burgers_hip import rom
    N, dt, B = 600, 0.04, 6
    X, Phi = pod_basis(N, dt, 64)
    mu1, mu2 = draw(B, seed=3)
    p = rom.PROJ["galerkin"]
    ref = rom.pod_prom_run_long_wide(X, np.ones(N), mu1, mu2, dt, 3, Phi, p)
    assert ref.redone == 0
    check_order_entries_skipped(ENTRY, ref, X, dt, mu1, mu2, p)


def test_facade_opt_in_and_unchanged_default(hip):
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    N, dt = 1024, 0.025
    X, Phi = pod_basis(N, dt, 96)
    _, T = mesh(N)
    U = FEMBurgers(X, T).pod_prom_burgers(dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG", long_wide=True)
    Uo = br.pod_prom_burgers(X, dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG")
    assert np.asarray(U).shape == (N, 7) and rel_l2(np.asarray(U), Uo) <= TOL
    default = rom.pod_prom_run(X, np.ones(N), [4.8], [0.021], dt, 2, Phi, projection="Galerkin")
    assert default.path == "library"
    long_only = rom.pod_prom_run(X, np.ones(N), [4.8], [0.021], dt, 2, Phi, projection="Galerkin", long_mesh=True)
    assert long_only.path == "library"
