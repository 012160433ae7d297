"""bg_rom_run_long_wide: the device-side POD-PROM time loop for meshes of 513 .. 1024 nodes and bases of 41 .. 96 modes
(csrc/rom_long_wide.hip), against the oracle and the library path (the default route for N > 512).
reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785.

Bases: the leading r left singular vectors of the FOM snapshots (oracle, C) of the 3 x 3 training grid, 200 steps."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from oracle import burgers_ref as br
from oracle import burgers_ref_c as brc

pytestmark = pytest.mark.gpu
TOL = 1e-10
ENTRY = "bg_rom_run_long_wide"


@functools.lru_cache(maxsize=None)
def _modes(N, dt, E=0.0, seed=None):
    """(X, U): the mesh (``seed``: interior nodes moved by at most 0.2 h) and the 96 leading left singular vectors."""
    X, _ = mesh(N)
    if seed is not None:
        X = X.copy()
        X[1:-1] += np.random.default_rng(seed).uniform(-0.2, 0.2, N - 2) * (100.0 / (N - 1))
    mu1 = np.repeat([4.25, 4.875, 5.5], 3); mu2 = np.tile([0.015, 0.0225, 0.03], 3)
    hist, _ = brc.fom_run(X, np.ones(N), mu1, mu2, dt, 200, E=E)
    U = np.linalg.svd(hist.reshape(-1, N).T, full_matrices=False)[0]
    return X, np.ascontiguousarray(U[:, :96])


def _basis(N, dt, r, E=0.0, seed=None):
    X, U = _modes(N, dt, E, seed)
    return X, np.ascontiguousarray(U[:, :r])


def _draw(B, seed=20251121):
    rng = np.random.default_rng(seed)
    return rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B)


def _check_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, proj, E=0.0, samples=None):
    hist, iters = res.hist.cpu().numpy(), res.iters.cpu().numpy()
    for s in (range(len(mu1)) if samples is None else samples):
        U, ito = br.pod_prom_burgers(X, dt, nT, np.ones(len(X)), mu1[s], E, mu2[s], Phi, projection=proj, return_iters=True)
        err = rel_l2(hist[s].T, U)
        print(f"N={len(X)} r={Phi.shape[1]} {proj} sample {s}: rel-L2 {err:.2e}, iterations {iters[s].tolist()} / {ito.tolist()}")
        assert err <= TOL, (proj, s, err)
        assert np.array_equal(iters[s], ito), (proj, s)
    assert not bool(res.flags.any()) and bool((res.info == 0).all())


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("N,dt,r", [(1024, 0.025, 96), (1024, 0.025, 41), (600, 0.04, 64), (513, 0.05, 77)])
def test_parity_with_the_oracle(hip, N, dt, r, proj):
    """N = 513: a last slab of one mesh row; N = 600: a ragged last slab; r = 41: one live column in its block; r = 77: no
    multiple of 4; r = 96 at N = 1024: the full kernel."""
    from burgers_hip import rom
    X, Phi = _basis(N, dt, r)
    mu1, mu2 = _draw(6)
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, 8, Phi, projection=proj, long_wide=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.redone == 0
    _check_vs_oracle(res, X, dt, 8, mu1, mu2, Phi, proj)


def _max_multiplier(X, dt, nT, mu1, mu2, Phi, proj, E):
    """Largest sub-diagonal multiplier of the unpivoted elimination over the systems of the reference's own run."""
    worst = 0.0
    real = np.linalg.solve

    def wrapped(A, b):
        nonlocal worst
        W = np.array(A, dtype=np.float64)
        for k in range(len(W) - 1):
            m = W[k + 1:, k] / W[k, k]
            worst = max(worst, float(np.abs(m).max()))
            W[k + 1:] -= np.outer(m, W[k])
        return real(A, b)
    np.linalg.solve = wrapped
    try:
        br.pod_prom_burgers(X, dt, nT, np.ones(len(X)), mu1, E, mu2, Phi, projection=proj)
    finally:
        np.linalg.solve = real
    return worst


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", ["diffusion", "nonuniform"])
def test_diffusion_and_nonuniform_mesh(hip, case, proj):
    """The guard decides who did the work: a sample whose unpivoted elimination meets a multiplier above 1 comes back
    marked and is redone through the library path.  The oracle's own multiplier says which it must be; an input whose
    multiplier lies within 1 % of the guard's threshold decides nothing and fails the test."""
    from burgers_hip import lib, rom
    N, dt, nT = 1024, 0.025, 8
    E, seed = (0.01, None) if case == "diffusion" else (0.0, 21)
    X, Phi = _basis(N, dt, 96, E=E, seed=seed)
    assert lib.mesh_is_uniform(X) == (seed is None)
    mu1, mu2 = _draw(3, seed=5)
    worst = _max_multiplier(X, dt, nT, mu1[0], mu2[0], Phi, proj, E)
    print(f"{case} {proj}: largest unpivoted multiplier of sample 0: {worst:.3f}")
    assert worst >= 1.01 or worst <= 0.99, f"unsuitable input: multiplier {worst} too close to the guard's threshold"
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, projection=proj, E=E, long_wide=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    print(f"{case} {proj}: redone {res.redone} of {len(mu1)}")
    assert res.redone == (len(mu1) if worst >= 1.01 else 0)
    _check_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, proj, E=E)


def _same(a, b):
    for k in ("hist", "iters", "flags", "info"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_batch_behaviour(hip):
    """B = 300 (more samples than workgroups) on N = 1024, r = 96, LSPG: a sample alone, the sample order of the persistent
    loop and the hand-back of every sample must not change what the batch computes."""
    from burgers_hip import lib, rom
    N, dt, nT, B = 1024, 0.025, 3, 300
    X, Phi = _basis(N, dt, 96)
    mu1, mu2 = _draw(B)
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
    _same(plain, res)
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
    N, dt = 1024, 0.025
    X, Phi = _basis(N, dt, 96)
    mu1, mu2 = _draw(5, seed=9)
    dev = torch.device("cuda", torch.cuda.current_device())
    p = rom.PROJ["lspg"]
    first = rom.pod_prom_run_long_wide(X, np.ones(N), mu1, mu2, dt, 5, Phi, p)
    again = rom.pod_prom_run_long_wide(X, np.ones(N), mu1, mu2, dt, 5, first.plan, p)
    torch.cuda.synchronize()
    assert again.plan is first.plan and again.path == ENTRY and first.redone == 0
    _same(again, first)
    # restart: the second half of a run from the state the first half ended in
    head = rom.pod_prom_run_long_wide(X, np.ones(N), mu1, mu2, dt, 2, first.plan, p)
    tail = rom.pod_prom_run_long_wide(X, head.hist[:, -1].cpu().numpy(), mu1, mu2, dt, 3, first.plan, p)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([head.hist, tail.hist[:, 1:]], 1), first.hist)
    assert torch.equal(torch.cat([head.iters, tail.iters], 1), first.iters)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    X6, _ = mesh(600)
    with pytest.raises(ValueError):
        rom.pod_prom_run_long_wide(X6, np.ones(600), mu1, mu2, dt, 2, first.plan, p)     # a plan for another N
    other_r = rom.LongWidePodPlan(Phi[:600, :64], dev)                               # another N and r
    with pytest.raises(ValueError):
        rom.pod_prom_run_long_wide(X, np.ones(N), mu1, mu2, dt, 2, other_r, p)
    with pytest.raises(ValueError):
        rom.LongWidePodPlan(np.concatenate([Phi, Phi[:, :1]], axis=1), dev)              # 97 columns
    with pytest.raises(ValueError):
        rom.LongWidePodPlan(np.zeros((1025, 48)), dev)


def test_order_entries_outside_the_batch_are_skipped(hip):
    from burgers_hip import lib, rom
    N, dt, B, r = 600, 0.04, 6, 64
    X, Phi = _basis(N, dt, r)
    mu1, mu2 = _draw(B, seed=3)
    p = rom.PROJ["galerkin"]
    ref = rom.pod_prom_run_long_wide(X, np.ones(N), mu1, mu2, dt, 3, Phi, p)
    assert ref.redone == 0
    dev = ref.hist.device
    L = lib.load()
    u0d = torch.ones((B, N), dtype=torch.float64, device=dev)
    mu1d, mu2d, Xd = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev), torch.as_tensor(X, device=dev)
    hist = torch.full((B, 4, N), -7.0, dtype=torch.float64, device=dev)
    iters = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    order = torch.arange(B, dtype=torch.int32, device=dev)
    order[1], order[4] = -1, B + 5
    rc = L.bg_rom_run_long_wide(N, B, r, 3, p, lib.ptr(Xd), lib.ptr(ref.plan.PhiP), lib.ptr(u0d), lib.ptr(mu1d), lib.ptr(mu2d),
                                dt, 0.0, 1e-6, 20, lib.mesh_options(X, supg=True), lib.ptr(hist), lib.ptr(iters),
                                lib.ptr(flags), lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    keep = [0, 2, 3, 5]
    assert torch.equal(hist[keep], ref.hist[keep]) and torch.equal(iters[keep], ref.iters[keep])
    assert bool((hist[[1, 4]] == -7.0).all()) and bool((info == 0).all())


def test_facade_opt_in_and_unchanged_default(hip):
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    N, dt = 1024, 0.025
    X, Phi = _basis(N, dt, 96)
    _, T = mesh(N)
    U = FEMBurgers(X, T).pod_prom_burgers(dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG", long_wide=True)
    Uo = br.pod_prom_burgers(X, dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG")
    assert np.asarray(U).shape == (N, 7) and rel_l2(np.asarray(U), Uo) <= TOL
    default = rom.pod_prom_run(X, np.ones(N), [4.8], [0.021], dt, 2, Phi, projection="Galerkin")
    assert default.path == "library"
    long_only = rom.pod_prom_run(X, np.ones(N), [4.8], [0.021], dt, 2, Phi, projection="Galerkin", long_mesh=True)
    assert long_only.path == "library"
