"""The device-side local POD time loop (bg_local_rom_run, rom.local_prom_run_fused) against the reference's live fixture,
the oracle and the host-driven batched iteration it replaces.  Tolerance 1e-10 against the oracle (as the host path),
1e-11 per sample against the host path; iteration counts, flags and cluster sequences must be equal."""
import numpy as np
import pytest
import torch

from conftest import load_golden, mesh, rel_l2
from loop_cases import DENSE_WIDTHS, _margins, _worst, to_np
from oracle import burgers_ref as br

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _fixture():
    g = load_golden("local_pod.npz")
    return g, {c: g[f"basis{c}"] for c in range(4)}


def _dense():
    """11 centres at U_g^T u of the fixture's LSPG trajectory at steps 0, 15, ..., 150 and bases of 8 .. 40 leading
    modes of the committed 40-mode basis: 10 switches in 150 steps through all 11 clusters."""
    g = load_golden("local_pod.npz")
    Phi = load_golden("committed_pod_r40.npz")["Phi"]
    centres = (g["U_global"][:, :12].T @ g["U_LSPG"][:, ::3]).T.copy()
    bases = {c: np.ascontiguousarray(Phi[:, :w]) for c, w in enumerate(DENSE_WIDTHS)}
    return centres, bases, g["U_global"]


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_live_fixture(hip, proj):
    from burgers_hip import rom
    g, bases = _fixture()
    X, _ = mesh(512)
    nT, stride = int(g["nT"]), int(g["stride"])
    res = rom.local_prom_run(X, np.ones(512), [float(g["mu1"]), 5.4], [float(g["mu2"]), 0.029], float(g["At"]), nT,
                             g["centers"], bases, g["U_global"], 12, projection=proj, fused=True)
    torch.cuda.synchronize()
    assert res.path == "bg_local_rom_run"
    assert int(res.info.abs().sum()) == 0
    assert rel_l2(to_np(res.hist[0]).T[:, ::stride], g["U_" + proj]) < TOL
    assert np.array_equal(to_np(res.iters[0]), g["iters_" + proj])
    for b, (m1, m2) in enumerate([(float(g["mu1"]), float(g["mu2"])), (5.4, 0.029)]):
        U, it, cl = br.local_prom_burgers(X, float(g["At"]), nT, np.ones(512), m1, 0.0, m2, g["centers"], bases,
                                          g["U_global"], 12, projection=proj, return_iters=True)
        assert rel_l2(to_np(res.hist[b]).T, U) < TOL
        assert np.array_equal(to_np(res.iters[b]), it)
        assert np.array_equal(to_np(res.clusters[b]), cl)
        assert len(np.unique(cl)) >= 2                         # the run really switches
    if proj == "LSPG":
        cl0 = to_np(res.clusters[0])
        assert cl0[120] == 0 and cl0[121] == 3                 # the switch 0 -> 3 at step 121


@pytest.mark.parametrize("proj,mus", [("LSPG", [(4.9, 0.022)]), ("Galerkin", [(4.6, 0.02), (5.3, 0.028)])])
def test_dense_switching_vs_oracle(hip, proj, mus):
    from burgers_hip import rom
    centres, bases, Ug = _dense()
    X, _ = mesh(512)
    res = rom.local_prom_run_fused(X, np.ones(512), [m[0] for m in mus], [m[1] for m in mus], 0.05, 150, centres, bases,
                                   Ug, 12, projection=proj)
    torch.cuda.synchronize()
    for b, (m1, m2) in enumerate(mus):
        U, it, cl = br.local_prom_burgers(X, 0.05, 150, np.ones(512), m1, 0.0, m2, centres, bases, Ug, 12,
                                          projection=proj, return_iters=True)
        assert (np.diff(cl) != 0).sum() >= 10 and len(np.unique(cl)) == 11
        assert np.array_equal(to_np(res.clusters[b]), cl)
        assert np.array_equal(to_np(res.iters[b]), it)
        assert rel_l2(to_np(res.hist[b]).T, U) < TOL


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_matches_the_host_path_at_batch_size(hip, proj):
    """The bench's (mu1, mu2) draw, B = 1024, the dense clustering.  Samples whose Picard iteration hits the 20-iteration
    cap in some step (BG_FLAG_HIT_CAP, equal on both paths) are excluded from the bitwise comparison: there the iteration
    does not contract, rounding decides the later steps, and neither path follows the oracle (measured on the LSPG sweep:
    113 capped samples, 9 of which differ from the host path; both paths differ from the oracle there by 1e-7 .. 0.4)."""
    import bench
    from burgers_hip import lib, rom
    centres, bases, Ug = _dense()
    X, _ = mesh(512)
    mu1, mu2 = bench.mu_shard(1024, 1, 0)
    dev = rom.local_prom_run(X, np.ones(512), mu1, mu2, 0.05, 150, centres, bases, Ug, 12, projection=proj, fused=True)
    host = rom.local_prom_run(X, np.ones(512), mu1, mu2, 0.05, 150, centres, bases, Ug, 12, projection=proj)
    torch.cuda.synchronize()
    assert dev.path == "bg_local_rom_run" and host.path == "host"
    assert torch.equal(dev.flags, host.flags)
    ok = (dev.flags & lib.BG_FLAG_HIT_CAP) == 0
    assert int(ok.sum()) >= 0.8 * 1024, int(ok.sum())                   # LSPG: 911 of 1024 never hit it
    near_tie = _margins(host, centres, Ug)[ok] < 1e-10
    assert int(near_tie.sum()) == 0                                # no step of this sweep needs the near-tie excuse
    assert torch.equal(dev.clusters[ok], host.clusters[ok])
    assert torch.equal(dev.iters[ok], host.iters[ok])
    switches = int((dev.clusters[ok, 1:] != dev.clusters[ok, :-1]).sum())
    assert switches > 0                                            # the reload is exercised
    d, h = dev.hist[ok].flatten(1), host.hist[ok].flatten(1)
    worst = float(((d - h).norm(dim=1) / h.norm(dim=1)).max())
    print(f"local POD {proj}: {int((~ok).sum())} capped samples excluded, {switches} switches, "
          f"worst per-sample rel-L2 device vs host {worst:.2e}")
    assert worst < 1e-11, worst


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_pivoted_branch_switches_too(hip, proj):
    from burgers_hip import lib, rom
    centres, bases, Ug = _dense()
    X, _ = mesh(512)
    mu1, mu2 = [4.6, 5.3, 4.9], [0.02, 0.028, 0.022]
    fast = rom.local_prom_run_fused(X, np.ones(512), mu1, mu2, 0.05, 150, centres, bases, Ug, 12, projection=proj)
    piv = rom.local_prom_run_fused(X, np.ones(512), mu1, mu2, 0.05, 150, centres, bases, Ug, 12, projection=proj,
                                   options=lib.BG_OPT_FORCE_PIVOTED)
    torch.cuda.synchronize()
    assert int(piv.info.abs().sum()) == 0
    assert torch.equal(fast.iters, piv.iters) and torch.equal(fast.clusters, piv.clusters)
    assert int((piv.clusters[:, 1:] != piv.clusters[:, :-1]).sum()) >= 10
    assert _worst(piv, fast) < 1e-12


def test_coarse_nonuniform_mesh_with_diffusion(hip):
    """N = 256 (4 rows per lane) on a perturbed mesh with E != 0: every other node of the fixture's mesh, the dense
    clustering's bases and U_global re-orthonormalised there (4 - 5 switches in 60 steps)."""
    from burgers_hip import rom
    g = load_golden("local_pod.npz")
    Phi = load_golden("committed_pod_r40.npz")["Phi"]
    X, _ = mesh(512)
    X = X[::2].copy()
    h = X[1] - X[0]
    rng = np.random.default_rng(5)
    X[1:-1] += rng.uniform(-0.2, 0.2, 254) * h
    Q = np.linalg.qr(Phi[::2])[0]
    bases = {c: np.ascontiguousarray(Q[:, :w]) for c, w in enumerate(DENSE_WIDTHS)}
    Ug = np.linalg.qr(g["U_global"][::2])[0]
    cen = (Ug.T @ g["U_LSPG"][::2, ::3]).T.copy()
    mus = [(4.7, 0.021), (5.2, 0.027)]
    for proj in ("Galerkin", "LSPG"):
        res = rom.local_prom_run_fused(X, np.ones(256), [m[0] for m in mus], [m[1] for m in mus], 0.05, 60, cen, bases,
                                       Ug, 12, projection=proj, E=0.02)
        torch.cuda.synchronize()
        for b, (m1, m2) in enumerate(mus):
            U, it, cl = br.local_prom_burgers(X, 0.05, 60, np.ones(256), m1, 0.02, m2, cen, bases, Ug, 12,
                                              projection=proj, return_iters=True)
            assert (np.diff(cl) != 0).sum() >= 4
            assert np.array_equal(to_np(res.clusters[b]), cl)
            assert np.array_equal(to_np(res.iters[b]), it)
            assert rel_l2(to_np(res.hist[b]).T, U) < TOL


def test_extreme_widths_and_global_modes(hip):
    """Widths 1 and 40 in one plan; m = 1 and m = 64."""
    from burgers_hip import rom
    g = load_golden("local_pod.npz")
    Phi = load_golden("committed_pod_r40.npz")["Phi"]
    X, _ = mesh(512)
    rng = np.random.default_rng(11)
    Ug64 = np.linalg.qr(np.concatenate([g["U_global"], rng.standard_normal((512, 52))], 1))[0]
    Ug64[:, :12] = g["U_global"]
    traj = g["U_LSPG"][:, ::6]                                     # steps 0, 30, ..., 150
    for m, widths in ((1, [1, 40, 12]), (64, [40, 1, 25, 8, 33, 17])):
        centres = (Ug64[:, :m].T @ traj[:, :len(widths)]).T.copy()
        bases = {c: np.ascontiguousarray(Phi[:, :w]) for c, w in enumerate(widths)}
        res = rom.local_prom_run_fused(X, np.ones(512), [4.9, 5.3], [0.022, 0.027], 0.05, 40, centres, bases, Ug64, m,
                                       projection="LSPG")
        torch.cuda.synchronize()
        assert res.plan.rmax == 40
        for b, (m1, m2) in enumerate([(4.9, 0.022), (5.3, 0.027)]):
            U, it, cl = br.local_prom_burgers(X, 0.05, 40, np.ones(512), m1, 0.0, m2, centres, bases, Ug64, m,
                                              projection="LSPG", return_iters=True)
            assert np.array_equal(to_np(res.clusters[b]), cl)
            assert np.array_equal(to_np(res.iters[b]), it)
            assert rel_l2(to_np(res.hist[b]).T, U) < TOL


def test_persistent_loop_and_empty_runs(hip):
    """B = 1200 > grid: a workgroup carries its loaded cluster from one sample to the next; B = 0 and nsteps = 0."""
    from burgers_hip import rom
    centres, bases, Ug = _dense()
    X, _ = mesh(512)
    rng = np.random.default_rng(3)
    mu1, mu2 = rng.uniform(4.25, 5.5, 1200), rng.uniform(0.015, 0.03, 1200)
    dev = rom.local_prom_run_fused(X, np.ones(512), mu1, mu2, 0.05, 40, centres, bases, Ug, 12, projection="Galerkin",
                                   balance=False)
    host = rom.local_prom_run(X, np.ones(512), mu1, mu2, 0.05, 40, centres, bases, Ug, 12, projection="Galerkin")
    torch.cuda.synchronize()
    assert torch.equal(dev.clusters, host.clusters) and torch.equal(dev.iters, host.iters)
    assert _worst(dev, host) < 1e-11
    for b in (0, 777, 1199):
        U, it, cl = br.local_prom_burgers(X, 0.05, 40, np.ones(512), mu1[b], 0.0, mu2[b], centres, bases, Ug, 12,
                                          projection="Galerkin", return_iters=True)
        assert np.array_equal(to_np(dev.clusters[b]), cl) and rel_l2(to_np(dev.hist[b]).T, U) < TOL
    empty = rom.local_prom_run_fused(X, np.ones(512), np.zeros(0), np.zeros(0), 0.05, 10, centres, bases, Ug, 12)
    assert tuple(empty.hist.shape) == (0, 11, 512) and tuple(empty.clusters.shape) == (0, 10)
    none = rom.local_prom_run_fused(X, np.ones(512), [4.9, 5.1], [0.022, 0.02], 0.05, 0, centres, bases, Ug, 12)
    torch.cuda.synchronize()
    assert tuple(none.clusters.shape) == (2, 0) and torch.equal(none.hist[:, 0].cpu(), torch.ones(2, 512, dtype=torch.float64))


def test_plans_and_fallbacks(hip):
    from burgers_hip import rom
    centres, bases, Ug = _dense()
    X, _ = mesh(512)
    mu1, mu2 = [4.6, 5.3, 4.9, 5.0], [0.02, 0.028, 0.022, 0.025]
    fresh = rom.local_prom_run_fused(X, np.ones(512), mu1, mu2, 0.05, 60, centres, bases, Ug, 12, projection="LSPG")
    again = rom.local_prom_run_fused(X, np.ones(512), mu1, mu2, 0.05, 60, None, None, None, 12, projection="LSPG",
                                     plan=fresh.plan)
    unbal = rom.local_prom_run_fused(X, np.ones(512), mu1, mu2, 0.05, 60, centres, bases, Ug, 12, projection="LSPG",
                                     balance=False)
    torch.cuda.synchronize()
    for r in (again, unbal):
        assert torch.equal(r.hist, fresh.hist) and torch.equal(r.iters, fresh.iters)
        assert torch.equal(r.clusters, fresh.clusters)
    X2, _ = mesh(256)
    with pytest.raises(ValueError):                                # a plan for another N
        rom.local_prom_run_fused(X2, np.ones(256), mu1, mu2, 0.05, 5, None, None, None, 12, plan=fresh.plan)
    with pytest.raises(ValueError):                                # a basis with the wrong row count
        rom.local_prom_run_fused(X, np.ones(512), mu1, mu2, 0.05, 5, centres, {**bases, 3: bases[3][:300]}, Ug, 12)
    with pytest.raises(ValueError):                                # centres not (C, m)
        rom.local_prom_run_fused(X, np.ones(512), mu1, mu2, 0.05, 5, centres[:, :10], bases, Ug, 12)
    with pytest.raises(ValueError):                                # U_global narrower than m
        rom.local_prom_run_fused(X, np.ones(512), mu1, mu2, 0.05, 5, centres, bases, Ug[:, :8], 12)
    # 80-mode bases: beyond the kernel, fused=True still runs (host path)
    g96 = load_golden("committed_pod_r96.npz")
    lp = load_golden("local_pod.npz")
    wide = {c0: np.ascontiguousarray(g96["Phi"][:, :w0]) for c0, w0 in zip(range(4), (80, 72, 66, 80))}
    assert rom.local_prom_run_fused(X, np.ones(512), 4.9, 0.022, 0.05, 12, lp["centers"], wide, lp["U_global"], 12) is None
    res = rom.local_prom_run(X, np.ones(512), 4.9, 0.022, 0.05, 12, lp["centers"], wide, lp["U_global"], 12, fused=True)
    torch.cuda.synchronize()
    assert res.path != "bg_local_rom_run"
    U, ito, cl = br.local_prom_burgers(X, 0.05, 12, np.ones(512), 4.9, 0.0, 0.022, lp["centers"], wide, lp["U_global"],
                                       12, projection="Galerkin", return_iters=True)
    assert rel_l2(to_np(res.hist[0]).T, U) < 1e-9 and np.array_equal(to_np(res.iters[0]), ito)
    assert np.array_equal(to_np(res.clusters[0]), cl)
    # a centre without a basis: the plan declines, the host path raises when that centre is predicted
    partial = {c: b for c, b in bases.items() if c != 0}
    plan = rom.LocalPodPlan(centres, partial, Ug, 12, 512, torch.device("cuda", 0))
    assert not plan.ok and "no local basis" in plan.reason
    with pytest.raises(KeyError):
        rom.local_prom_run(X, np.ones(512), 4.9, 0.022, 0.05, 5, centres, partial, Ug, 12, fused=True)


def test_facade(hip):
    from fem_burgers import FEMBurgers
    g, bases = _fixture()
    X, T = mesh(512)

    class KM:                                             # what the reference's drivers pass (joblib-loaded KMeans)
        cluster_centers_ = g["centers"]
    fb = FEMBurgers(X, T)
    nT = 130
    for mu1, mu2 in ((4.9, 0.022), ([4.9, 5.4], [0.022, 0.029])):
        a = fb.local_prom_burgers(0.05, nT, np.ones(512), mu1, 0.0, mu2, KM(), bases, g["U_global"], 12, projection="LSPG",
                                  fused=True)
        b = fb.local_prom_burgers(0.05, nT, np.ones(512), mu1, 0.0, mu2, KM(), bases, g["U_global"], 12, projection="LSPG")
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.shape[-2:] == (512, nT + 1)
        assert rel_l2(a, b) < 1e-11
