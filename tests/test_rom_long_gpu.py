"""bg_rom_run_long: the device-side POD-PROM time loop for meshes of 513 .. 1024 nodes and bases of up to 40 modes
(csrc/rom_long.hip), against the oracle and the library path (the default route for N > 512).
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
ENTRY = "bg_rom_run_long"


@functools.lru_cache(maxsize=None)
def _modes(N, dt, E=0.0, seed=None):
    """(X, U): the mesh (``seed``: interior nodes moved by at most 0.2 h) and the 40 leading left singular vectors."""
    X, _ = mesh(N)
    if seed is not None:
        X = X.copy()
        X[1:-1] += np.random.default_rng(seed).uniform(-0.2, 0.2, N - 2) * (100.0 / (N - 1))
    mu1 = np.repeat([4.25, 4.875, 5.5], 3); mu2 = np.tile([0.015, 0.0225, 0.03], 3)
    hist, _ = brc.fom_run(X, np.ones(N), mu1, mu2, dt, 200, E=E)
    U = np.linalg.svd(hist.reshape(-1, N).T, full_matrices=False)[0]
    return X, np.ascontiguousarray(U[:, :40])


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
@pytest.mark.parametrize("N,dt,r", [(1024, 0.025, 40), (1024, 0.025, 25), (600, 0.04, 40), (513, 0.05, 17)])
def test_parity_with_the_oracle(hip, N, dt, r, proj):
    from burgers_hip import rom
    X, Phi = _basis(N, dt, r)
    mu1, mu2 = _draw(6)
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, 12, Phi, projection=proj, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    _check_vs_oracle(res, X, dt, 12, mu1, mu2, Phi, proj)


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
    from burgers_hip import lib, rom
    N, dt, nT = 1024, 0.025, 12
    E, seed = (0.01, None) if case == "diffusion" else (0.0, 21)
    X, Phi = _basis(N, dt, 40, E=E, seed=seed)
    assert lib.mesh_is_uniform(X) == (seed is None)
    mu1, mu2 = _draw(3, seed=5)
    # info stays 0 either way (the pivoting repair runs inside the call); the multipliers say which kernel did the work
    print(f"{case} {proj}: largest unpivoted multiplier of sample 0: {_max_multiplier(X, dt, nT, mu1[0], mu2[0], Phi, proj, E):.3f}")
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, projection=proj, E=E, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    _check_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, proj, E=E)


def _same(a, b):
    for k in ("hist", "iters", "flags", "info"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_at_batch_size(hip, proj):
    """B = 1024 on N = 1024, r = 40: 16 samples against the oracle, all of them against the library path (the default
    route; its counts are not compared: the library GEMM's summation order depends on the batch size), and the sample
    order of the persistent loop must not change a bit."""
    from burgers_hip import rom
    N, dt, nT, B = 1024, 0.025, 4, 1024
    X, Phi = _basis(N, dt, 40)
    mu1, mu2 = _draw(B)
    p = rom.PROJ[proj.lower()]
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, projection=proj, long_mesh=True)
    ref = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, projection=proj)
    plain = rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, nT, res.plan, p, balance=False)
    torch.cuda.synchronize()
    assert res.path == ENTRY and ref.path == "library" and plain.path == ENTRY
    _check_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, proj, samples=range(0, B, B // 16))
    fh, lh = res.hist.cpu().numpy(), ref.hist.cpu().numpy()
    worst = max(rel_l2(fh[s], lh[s]) for s in range(B))
    print(f"{proj}: worst rel-L2 against the library path over {B} samples {worst:.2e}")
    assert worst <= TOL
    _same(plain, res)


def test_plan_reuse_and_refusals(hip, monkeypatch):
    from burgers_hip import rom
    N, dt = 1024, 0.025
    X, Phi = _basis(N, dt, 40)
    mu1, mu2 = _draw(5, seed=9)
    dev = torch.device("cuda", torch.cuda.current_device())
    p = rom.PROJ["lspg"]
    first = rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, 5, Phi, p)
    again = rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, 5, first.plan, p)
    torch.cuda.synchronize()
    assert again.plan is first.plan and again.path == ENTRY
    _same(again, first)
    # restart: the second half of a run from the state the first half ended in
    head = rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, 2, first.plan, p)
    tail = rom.pod_prom_run_long(X, head.hist[:, -1].cpu().numpy(), mu1, mu2, dt, 3, first.plan, p)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([head.hist, tail.hist[:, 1:]], 1), first.hist)
    assert torch.equal(torch.cat([head.iters, tail.iters], 1), first.iters)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    X6, _ = mesh(600)
    with pytest.raises(ValueError):
        rom.pod_prom_run_long(X6, np.ones(600), mu1, mu2, dt, 2, first.plan, p)          # a plan for another N
    other_r = rom.LongPodPlan(Phi[:600, :17], dev)                                   # another N and r
    with pytest.raises(ValueError):
        rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, 2, other_r, p)
    with pytest.raises(ValueError):
        rom.LongPodPlan(np.concatenate([Phi, Phi[:, :1]], axis=1), dev)                  # 41 columns
    with pytest.raises(ValueError):
        rom.LongPodPlan(np.zeros((1025, 8)), dev)


def test_forced_pivoting_route(hip):
    from burgers_hip import lib, rom
    N, dt = 1024, 0.025
    X, Phi = _basis(N, dt, 40)
    mu1, mu2 = _draw(4, seed=13)
    res = rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, 12, Phi, rom.PROJ["lspg"], options=lib.BG_OPT_FORCE_PIVOTED)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    _check_vs_oracle(res, X, dt, 12, mu1, mu2, Phi, "LSPG")


def test_order_entries_outside_the_batch_are_skipped(hip):
    from burgers_hip import lib, rom
    N, dt, B = 600, 0.04, 6
    X, Phi = _basis(N, dt, 40)
    mu1, mu2 = _draw(B, seed=3)
    p = rom.PROJ["galerkin"]
    ref = rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, 3, Phi, p)
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
    rc = L.bg_rom_run_long(N, B, 40, 3, p, lib.ptr(Xd), lib.ptr(ref.plan.PhiP), lib.ptr(u0d), lib.ptr(mu1d), lib.ptr(mu2d),
                           dt, 0.0, 1e-6, 20, lib.mesh_options(X, supg=True), lib.ptr(hist), lib.ptr(iters), lib.ptr(flags),
                           lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    keep = [0, 2, 3, 5]
    assert torch.equal(hist[keep], ref.hist[keep]) and torch.equal(iters[keep], ref.iters[keep])
    assert bool((hist[[1, 4]] == -7.0).all())


def test_facade_opt_in_and_unchanged_default(hip):
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    N, dt = 1024, 0.025
    X, Phi = _basis(N, dt, 40)
    _, T = mesh(N)
    U = FEMBurgers(X, T).pod_prom_burgers(dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG", long_mesh=True)
    Uo = br.pod_prom_burgers(X, dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG")
    assert np.asarray(U).shape == (N, 7) and rel_l2(np.asarray(U), Uo) <= TOL
    default = rom.pod_prom_run(X, np.ones(N), [4.8], [0.021], dt, 2, Phi, projection="Galerkin")
    assert default.path == "library"
