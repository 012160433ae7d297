"""bg_rom_run_long: the device-side POD-PROM time loop for meshes of 513 .. 1024 nodes and bases of up to 40 modes
(csrc/rom_long.hip), against the oracle and the library path (the default route for N > 512).
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
ENTRY = "bg_rom_run_long"


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("N,dt,r", [(1024, 0.025, 40), (1024, 0.025, 25), (600, 0.04, 40), (513, 0.05, 17)])
def test_parity_with_the_oracle(hip, N, dt, r, proj):
    from burgers_hip import rom
    X, Phi = pod_basis(N, dt, r)
    mu1, mu2 = draw(6)
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, 12, Phi, projection=proj, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    check_pod_vs_oracle(res, X, dt, 12, mu1, mu2, Phi, proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", ["diffusion", "nonuniform"])
def test_diffusion_and_nonuniform_mesh(hip, case, proj):
    from burgers_hip import lib, rom
    N, dt, nT = 1024, 0.025, 12
    E, seed = (0.01, None) if case == "diffusion" else (0.0, 21)
    X, Phi = pod_basis(N, dt, 40, E=E, seed=seed)
    assert lib.mesh_is_uniform(X) == (seed is None)
    mu1, mu2 = draw(3, seed=5)
    # info stays 0 either way (the pivoting repair runs inside the call); the multipliers say which kernel did the work
    print(f"{case} {proj}: largest unpivoted multiplier of sample 0: {max_multiplier(X, dt, nT, mu1[0], mu2[0], Phi, proj, E):.3f}")
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, projection=proj, E=E, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    check_pod_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, proj, E=E)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_at_batch_size(hip, proj):
    """B = 1024 on N = 1024, r = 40: 16 samples against the oracle, all of them against the library path (the default
    route; its counts are not compared: the library GEMM's summation order depends on the batch size), and the sample
    order of the persistent loop must not change a bit."""
    from burgers_hip import rom
    N, dt, nT, B = 1024, 0.025, 4, 1024
    X, Phi = pod_basis(N, dt, 40)
    mu1, mu2 = draw(B)
    p = rom.PROJ[proj.lower()]
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, projection=proj, long_mesh=True)
    ref = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, projection=proj)
    plain = rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, nT, res.plan, p, balance=False)
    torch.cuda.synchronize()
    assert res.path == ENTRY and ref.path == "library" and plain.path == ENTRY
    check_pod_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, proj, samples=range(0, B, B // 16))
    fh, lh = res.hist.cpu().numpy(), ref.hist.cpu().numpy()
    worst = max(rel_l2(fh[s], lh[s]) for s in range(B))
    print(f"{proj}: worst rel-L2 against the library path over {B} samples {worst:.2e}")
    assert worst <= TOL
    same(plain, res)


def test_plan_reuse_and_refusals(hip, monkeypatch):
    from burgers_hip import rom
    X, Phi = pod_basis(1024, 0.025, 40)
    check_plan_reuse_restart_and_refusals(monkeypatch, rom.pod_prom_run_long, rom.LongPodPlan, ENTRY, X, 0.025, Phi, other_r=17,
                                          too_long=(1025, 8))


def test_forced_pivoting_route(hip):
    from burgers_hip import lib, rom
    N, dt = 1024, 0.025
    X, Phi = pod_basis(N, dt, 40)
    mu1, mu2 = draw(4, seed=13)
    res = rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, 12, Phi, rom.PROJ["lspg"], options=lib.BG_OPT_FORCE_PIVOTED)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    check_pod_vs_oracle(res, X, dt, 12, mu1, mu2, Phi, "LSPG")


def test_order_entries_outside_the_batch_are_skipped(hip):
    from burgers_hip import rom
    N, dt, B = 600, 0.04, 6
    X, Phi = pod_basis(N, dt, 40)
    mu1, mu2 = draw(B, seed=3)
    p = rom.PROJ["galerkin"]
    ref = rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, 3, Phi, p)
    check_order_entries_skipped(ENTRY, ref, X, dt, mu1, mu2, p)


def test_facade_opt_in_and_unchanged_default(hip):
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    N, dt = 1024, 0.025
    X, Phi = pod_basis(N, dt, 40)
    _, T = mesh(N)
    U = FEMBurgers(X, T).pod_prom_burgers(dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG", long_mesh=True)
    Uo = br.pod_prom_burgers(X, dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG")
    assert np.asarray(U).shape == (N, 7) and rel_l2(np.asarray(U), Uo) <= TOL
    default = rom.pod_prom_run(X, np.ones(N), [4.8], [0.021], dt, 2, Phi, projection="Galerkin")
    assert default.path == "library"
