"""bg_local_rom_run_long: the device-side local POD time loop for meshes of 513 .. 1024 nodes (csrc/rom_local_long.hip),
against the oracle and the host-driven iteration (the default route for N > 512).
reference: FEMBurgers.local_prom_burgers, FEM/fem_burgers.py:979-1079.

Clustering (as test_local_rom_fused_gpu._dense, on loop_cases.training_snapshots): Phi = U_global = the 40 leading left
singular vectors of the FOM snapshots (oracle, C) of the 3 x 3 training grid, 200 steps; m = 12; 11 centres at U_g^T u of
the oracle's LSPG r = 40 POD run at mu = (4.9, 0.022), steps 0, 4, ..., 40; bases Phi[:, :w], w in DENSE_WIDTHS.
Tolerances: 1e-10 against the oracle (every ROM parity test here), 1e-11 per sample against the host path and 1e-12 between
the fast and the pivoted route (test_local_rom_fused_gpu); iteration counts, flags and cluster sequences must be equal."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from loop_cases import DENSE_WIDTHS, _margins, _worst, draw, to_np, training_snapshots
from oracle import burgers_ref as br

pytestmark = pytest.mark.gpu
TOL = 1e-10
ENTRY = "bg_local_rom_run_long"
NT = 40
MUS = {"LSPG": [(4.9, 0.022), (5.4, 0.029)], "Galerkin": [(4.6, 0.02), (5.3, 0.028)]}


@functools.lru_cache(maxsize=None)
def _clustering(N, dt, E=0.0, seed=None, widths=tuple(DENSE_WIDTHS)):
    """(X, centres, bases, U_global) of the module docstring for one mesh."""
    X, _, U = training_snapshots(N, dt, E, seed)
    U = np.ascontiguousarray(U[:, :40])
    traj = br.pod_prom_burgers(X, dt, NT, np.ones(N), 4.9, E, 0.022, U, projection="LSPG")
    centres = (U[:, :12].T @ traj[:, ::4]).T.copy()
    assert centres.shape == (11, 12)
    bases = {c: np.ascontiguousarray(U[:, :w]) for c, w in enumerate(widths)}
    return X, centres, bases, U


def _check_vs_oracle(res, X, dt, mus, centres, bases, Ug, proj, E=0.0, samples=None, min_switches=8):
    """Clusters, iteration counts and rel-L2 of ``samples`` against the oracle; returns the oracle's cluster paths."""
    paths = []
    for b in (range(len(mus)) if samples is None else samples):
        U, it, cl = br.local_prom_burgers(X, dt, NT, np.ones(len(X)), mus[b][0], E, mus[b][1], centres, bases, Ug, 12,
                                          projection=proj, return_iters=True)
        sw = int((np.diff(cl) != 0).sum())
        err = rel_l2(to_np(res.hist[b]).T, U)
        print(f"N={len(X)} {proj} sample {b} mu={mus[b]}: rel-L2 {err:.2e}, {sw} switches through {len(np.unique(cl))} "
              f"clusters, iterations up to {int(it.max())}")
        if min_switches is not None:
            assert sw >= min_switches, (proj, b, sw)                 # from the oracle's own output
        assert np.array_equal(to_np(res.clusters[b]), cl), (proj, b)
        assert np.array_equal(to_np(res.iters[b]), it), (proj, b)
        assert err <= TOL, (proj, b, err)
        paths.append(cl)
    return paths


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("N,dt", [(1024, 0.025), (600, 0.04), (513, 0.05)])
def test_parity_with_the_oracle(hip, N, dt, proj):
    """The default clustering starts in the narrowest cluster (8 modes, centre 0 = U_g^T u0): the first step after u0 runs
    with 32 padded unknowns."""
    from burgers_hip import rom
    X, centres, bases, Ug = _clustering(N, dt)
    mus = MUS[proj]
    res = rom.local_prom_run(X, np.ones(N), [m[0] for m in mus], [m[1] for m in mus], dt, NT, centres, bases, Ug, 12,
                             projection=proj, fused=True, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    assert bool((res.info == 0).all())
    paths = _check_vs_oracle(res, X, dt, mus, centres, bases, Ug, proj)
    for cl in paths:
        assert cl[0] == 0 and bases[int(cl[0])].shape[1] == 8 == min(DENSE_WIDTHS)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_all_widths_forty(hip, proj):
    from burgers_hip import rom
    N, dt = 1024, 0.025
    X, centres, bases, Ug = _clustering(N, dt, widths=(40,) * 11)
    mus = MUS[proj]
    res = rom.local_prom_run(X, np.ones(N), [m[0] for m in mus], [m[1] for m in mus], dt, NT, centres, bases, Ug, 12,
                             projection=proj, fused=True, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.plan.rmax == 40 and bool((res.info == 0).all())
    _check_vs_oracle(res, X, dt, mus, centres, bases, Ug, proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_pivoted_branch_switches_too(hip, proj):
    """BG_OPT_FORCE_PIVOTED against the fast route on the four (mu1, mu2) pairs of MUS, each taken only if the ORACLE's run
    of it under this projection stays below the 20-iteration cap.  A step that reaches the cap does not contract, and there
    rounding decides what follows on any route: on the CPU reference, LSPG at (5.3, 0.028) reaches the cap (the other
    seven runs stay at or below 12 iterations), and multiplying every np.linalg.solve result of that run by
    1 + 1.1e-16 cond(Ar) N(0, 1) (cond(Ar) <= 59) moves its history by 2.5e-11 in rel-L2, while the same perturbation moves
    the runs below the cap by 1e-15 .. 1.7e-15.  With that pair included the device gave 6.5e-11 between its two routes,
    identical iteration counts and clusters.  So 1e-12 is asked of the runs that contract; at least three must remain."""
    from burgers_hip import lib, rom
    N, dt = 1024, 0.025
    X, centres, bases, Ug = _clustering(N, dt)
    mus = []
    for m1, m2 in MUS["Galerkin"] + MUS["LSPG"]:
        it = br.local_prom_burgers(X, dt, NT, np.ones(N), m1, 0.0, m2, centres, bases, Ug, 12, projection=proj,
                                   return_iters=True)[1]
        print(f"{proj} mu=({m1}, {m2}): the oracle's iterations go up to {int(it.max())}")
        if int(it.max()) < 20:
            mus.append((m1, m2))
    assert len(mus) >= 3, mus
    mu1, mu2 = [m[0] for m in mus], [m[1] for m in mus]
    fast = rom.local_prom_run_long(X, np.ones(N), mu1, mu2, dt, NT, centres, bases, Ug, 12, projection=proj)
    piv = rom.local_prom_run_long(X, np.ones(N), mu1, mu2, dt, NT, None, None, None, 12, projection=proj, plan=fast.plan,
                                  options=lib.BG_OPT_FORCE_PIVOTED)
    torch.cuda.synchronize()
    assert fast.path == ENTRY and piv.path == ENTRY
    assert int(piv.info.abs().sum()) == 0 and int(fast.info.abs().sum()) == 0
    assert not bool(fast.flags.any()) and not bool(piv.flags.any())
    assert torch.equal(fast.iters, piv.iters) and torch.equal(fast.clusters, piv.clusters)
    assert int((piv.clusters[:, 1:] != piv.clusters[:, :-1]).sum()) >= 8
    worst = _worst(piv, fast)
    print(f"{proj}: worst per-sample rel-L2 pivoted vs fast over {len(mus)} samples {worst:.2e}")
    assert worst < 1e-12


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_nonuniform_mesh_with_diffusion(hip, proj):
    from burgers_hip import lib, rom
    N, dt, E = 1024, 0.025, 0.01
    X, centres, bases, Ug = _clustering(N, dt, E=E, seed=21)
    assert not lib.mesh_is_uniform(X)
    # LSPG at (5.4, 0.029) is left out on this mesh: the oracle's own run reaches the 20-iteration cap there, and a step
    # that does not contract is decided by rounding (test_matches_the_host_path_at_batch_size)
    mus = MUS[proj] if proj == "Galerkin" else MUS[proj][:1]
    res = rom.local_prom_run(X, np.ones(N), [m[0] for m in mus], [m[1] for m in mus], dt, NT, centres, bases, Ug, 12,
                             projection=proj, E=E, fused=True, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY and bool((res.info == 0).all()) and not bool(res.flags.any())
    _check_vs_oracle(res, X, dt, mus, centres, bases, Ug, proj, E=E)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_matches_the_host_path_at_batch_size(hip, proj):
    """N = 1024, B = 1024, the draw of loop_cases.draw.  The host-driven iteration is the reference.  Samples whose
    Picard iteration hits the 20-iteration cap in some step (BG_FLAG_HIT_CAP, equal on both paths) are left out of the
    comparison: there the iteration does not contract and rounding decides the later steps (see
    test_local_rom_fused_gpu.test_matches_the_host_path_at_batch_size).  At least 75 % of the batch must remain."""
    from burgers_hip import lib, rom
    N, dt, B = 1024, 0.025, 1024
    X, centres, bases, Ug = _clustering(N, dt)
    mu1, mu2 = draw(B)
    dev = rom.local_prom_run(X, np.ones(N), mu1, mu2, dt, NT, centres, bases, Ug, 12, projection=proj, fused=True,
                             long_mesh=True)
    host = rom.local_prom_run(X, np.ones(N), mu1, mu2, dt, NT, centres, bases, Ug, 12, projection=proj)
    torch.cuda.synchronize()
    assert dev.path == ENTRY and host.path == "host"
    ok = (host.flags & lib.BG_FLAG_HIT_CAP) == 0
    kept = int(ok.sum())
    print(f"local POD long {proj}: {B - kept} of {B} samples hit the cap on the host route, {kept} ({kept / B:.1%}) remain")
    assert torch.equal(dev.flags, host.flags)
    assert kept >= 0.75 * B, kept
    margins = _margins(host, centres, Ug)[ok]
    print(f"  smallest tie margin over the retained steps {float(margins.min()):.2e}")
    assert int((margins < 1e-10).sum()) == 0
    assert torch.equal(dev.clusters[ok], host.clusters[ok])
    assert torch.equal(dev.iters[ok], host.iters[ok])
    switches = int((dev.clusters[ok, 1:] != dev.clusters[ok, :-1]).sum())
    assert switches > 0
    d, h = dev.hist[ok].flatten(1), host.hist[ok].flatten(1)
    worst = float(((d - h).norm(dim=1) / h.norm(dim=1)).max())
    print(f"  {switches} switches, worst per-sample rel-L2 device vs host {worst:.2e}")
    assert worst < 1e-11, worst
    assert bool((dev.info == 0).all())
    picks = [int(s) for s in ok.nonzero().squeeze(1)[:: max(1, kept // 16)][:16].tolist()]
    assert len(picks) == 16
    _check_vs_oracle(dev, X, dt, list(zip(mu1, mu2)), centres, bases, Ug, proj, samples=picks, min_switches=None)
    # the sample order of the persistent loop must not change a bit
    order = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=dev.hist.device)
    L = lib.load()
    plan = dev.plan
    Xd, u0d, mu1d, mu2d = dev._keep[:4]
    hist = torch.empty_like(dev.hist)
    iters, flags, info, clusters = (torch.zeros_like(t) for t in (dev.iters, dev.flags, dev.info, dev.clusters))
    rc = L.bg_local_rom_run_long(N, B, plan.C, plan.rmax, plan.m, NT, rom.PROJ[proj.lower()], lib.ptr(Xd),
                                 lib.ptr(plan.stack), lib.ptr(plan.widths), lib.ptr(plan.UgT), lib.ptr(plan.centres),
                                 lib.ptr(u0d), lib.ptr(mu1d), lib.ptr(mu2d), dt, 0.0, 1e-6, 20, lib.mesh_options(X, supg=True),
                                 lib.ptr(hist), lib.ptr(iters), lib.ptr(flags), lib.ptr(info), lib.ptr(clusters),
                                 lib.ptr(order), lib.stream_ptr(hist.device))
    assert rc == 0
    torch.cuda.synchronize()
    for a, b, k in ((hist, dev.hist, "hist"), (iters, dev.iters, "iters"), (flags, dev.flags, "flags"), (info, dev.info, "info"),
                    (clusters, dev.clusters, "clusters")):
        assert torch.equal(a, b), k


def test_plan_reuse(hip):
    from burgers_hip import rom
    N, dt = 1024, 0.025
    X, centres, bases, Ug = _clustering(N, dt)
    mu1, mu2 = draw(5, seed=9)
    first = rom.local_prom_run_long(X, np.ones(N), mu1, mu2, dt, NT, centres, bases, Ug, 12, projection="LSPG")
    again = rom.local_prom_run_long(X, np.ones(N), mu1, mu2, dt, NT, None, None, None, 12, projection="LSPG", plan=first.plan)
    torch.cuda.synchronize()
    assert again.plan is first.plan and again.path == ENTRY and first.plan.long_mesh
    for k in ("hist", "iters", "flags", "info", "clusters"):
        assert torch.equal(getattr(again, k), getattr(first, k)), k
    assert int((first.clusters[:, 1:] != first.clusters[:, :-1]).sum()) > 0


def test_routing(hip):
    from burgers_hip import rom
    mu1, mu2 = [4.9], [0.022]
    X5, centres5, bases5, Ug5 = _clustering(512, 0.05)
    at512 = rom.local_prom_run(X5, np.ones(512), mu1, mu2, 0.05, 3, centres5, bases5, Ug5, 12, fused=True, long_mesh=True)
    assert at512.path == "bg_local_rom_run"
    N, dt = 1024, 0.025
    X, centres, bases, Ug = _clustering(N, dt)
    unfused = rom.local_prom_run(X, np.ones(N), mu1, mu2, dt, 3, centres, bases, Ug, 12, long_mesh=True)
    assert unfused.path == "host"
    default = rom.local_prom_run(X, np.ones(N), mu1, mu2, dt, 3, centres, bases, Ug, 12, fused=True)
    assert default.path == "host"                                     # no default changed
    wide = dict(bases)
    wide[3] = np.concatenate([Ug, Ug[:, :1]], axis=1)                   # 41 columns
    too_wide = rom.local_prom_run(X, np.ones(N), mu1, mu2, dt, 3, centres, wide, Ug, 12, fused=True, long_mesh=True)
    assert too_wide.path == "host"
    with pytest.raises(ValueError):
        rom.local_prom_run_long(X, np.ones(N), mu1, mu2, dt, 3, centres, wide, Ug, 12)
    X1025, _ = mesh(1025)
    pad = lambda a: np.concatenate([a, a[-1:]], axis=0)
    with pytest.raises(ValueError):
        rom.local_prom_run_long(X1025, np.ones(1025), mu1, mu2, dt, 3, centres, {c: pad(b) for c, b in bases.items()},
                                pad(Ug), 12)
    torch.cuda.synchronize()


def test_facade(hip):
    from fem_burgers import FEMBurgers
    N, dt = 1024, 0.025
    X, centres, bases, Ug = _clustering(N, dt)
    _, T = mesh(N)

    class KM:                                             # what the reference's drivers pass (joblib-loaded KMeans)
        cluster_centers_ = centres
    U = FEMBurgers(X, T).local_prom_burgers(dt, NT, np.ones(N), 4.9, 0.0, 0.022, KM(), bases, Ug, 12, projection="LSPG",
                                            fused=True, long_mesh=True)
    Uo = br.local_prom_burgers(X, dt, NT, np.ones(N), 4.9, 0.0, 0.022, centres, bases, Ug, 12, projection="LSPG")
    Uo = Uo[0] if isinstance(Uo, tuple) else Uo
    assert np.asarray(U).shape == (N, NT + 1) and rel_l2(np.asarray(U), Uo) <= TOL
