"""bg_rom_run_blocked: the device-side POD-PROM time loop for bases of up to 256 modes (the thesis' r = 160 and r = 227),
against the oracle, the library path, the committed PROM outputs and the other device-side loops.
reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785; bases POD/modes/U_modes_tol_1e-05 / 1e-06.npy."""
import numpy as np
import pytest
import torch

from conftest import load_golden, mesh, rel_l2
from loop_cases import check_pod_vs_oracle, same
from oracle import burgers_ref as br

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope="module")
def thesis_bases(hip):
    """The 9 training runs regenerated on the device (pinned to the committed snapshots) and the thesis' two finest
    bases built from them: eps^2 = 1e-5 -> K = 160, eps^2 = 1e-6 -> K = 227."""
    from burgers_hip import fom, pod
    N = 512
    X, _ = mesh(N)
    mu1 = np.repeat(np.linspace(4.25, 5.5, 3), 3); mu2 = np.tile(np.linspace(0.015, 0.03, 3), 3)
    res = fom.fom_run(X, np.ones(N), mu1, mu2, 0.05, 500)
    h = res.hist.cpu().numpy()
    gf = load_golden("committed_fom_n512.npz")
    for b, key in ((0, "4.250_0.0150"), (8, "5.500_0.0300")):
        assert np.linalg.norm(h[b].T[:, gf["cols"]] - gf["U_" + key]) < 1e-10 * np.linalg.norm(gf["U_" + key])
    S = pod.snapshot_matrix(res.hist).contiguous()
    out = {}
    for eps2, K in ((1e-5, 160), (1e-6, 227)):
        U, _, s_all = pod.pod_basis(S, eps2)
        assert U.shape == (N, K)
        out[K] = U.cpu().numpy()
    out["S"] = S
    return out


def _oracle(X, nT, mu1, mu2, Phi, proj, E=0.0):
    return br.pod_prom_burgers(X, 0.05, nT, np.ones(len(X)), mu1, E, mu2, Phi, projection=proj, return_iters=True)


@pytest.mark.parametrize("K", [160, 227])
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_thesis_bases_vs_oracle(thesis_bases, K, proj):
    from burgers_hip import rom
    X, _ = mesh(512)
    Phi = thesis_bases[K]
    mu1, mu2 = [4.75, 5.3], [0.02, 0.018]
    res = rom.pod_prom_run_blocked(X, np.ones(512), mu1, mu2, 0.05, 8, Phi, rom.PROJ[proj.lower()])
    torch.cuda.synchronize()
    assert res.path == "bg_rom_run_blocked" and res.redone == 0
    check_pod_vs_oracle(res, X, 0.05, 8, mu1, mu2, Phi, proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_r227_vs_library_path_at_batch_size(thesis_bases, proj):
    """B = 257 (one more than a round number of workgroups), 20 steps, the bench's mu draw."""
    from burgers_hip import rom
    X, _ = mesh(512)
    Phi = thesis_bases[227]
    B, nT = 257, 20
    rng = np.random.default_rng(20251121)
    mu1, mu2 = rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B)
    f = rom.pod_prom_run_blocked(X, np.ones(512), mu1, mu2, 0.05, nT, Phi, rom.PROJ[proj.lower()])
    lib = rom.pod_prom_run(X, np.ones(512), mu1, mu2, 0.05, nT, Phi, projection=proj, fused=False)
    torch.cuda.synchronize()
    assert lib.path == "library" and f.path == "bg_rom_run_blocked"
    ff, lf = f.flags.cpu().numpy(), lib.flags.cpu().numpy()
    assert np.array_equal(ff, lf)
    fh, lh = f.hist.cpu().numpy(), lib.hist.cpu().numpy()
    fi, li = f.iters.cpu().numpy(), lib.iters.cpu().numpy()
    capped = (ff & 1) != 0
    assert (~capped).sum() > B // 2
    for s in np.nonzero(~capped)[0]:
        assert rel_l2(fh[s], lh[s]) < TOL, s
        assert np.array_equal(fi[s], li[s]), s


def test_committed_outputs_and_the_other_loops(hip):
    from burgers_hip import rom
    X, _ = mesh(512)
    g96 = load_golden("committed_pod_r96.npz")
    g40 = load_golden("committed_pod_r40.npz")
    for tag, proj in (("galerkin", "Galerkin"), ("lspg", "LSPG")):
        p = rom.PROJ[tag]
        res = rom.pod_prom_run_blocked(X, np.ones(512), [4.75, 5.3], [0.02, 0.018], 0.05, 8, g96["Phi"], p)
        wide = rom.pod_prom_run_wide(X, np.ones(512), [4.75, 5.3], [0.02, 0.018], 0.05, 8, g96["Phi"], p)
        torch.cuda.synchronize()
        assert res.path == "bg_rom_run_blocked" and wide.path == "bg_rom_run_wide"
        assert rel_l2(res.hist[0].cpu().numpy().T, g96["first9_" + tag]) < TOL
        for s in range(2):
            assert rel_l2(res.hist[s].cpu().numpy(), wide.hist[s].cpu().numpy()) < TOL
            assert torch.equal(res.iters[s], wide.iters[s])
        cols = g40["cols"]
        res = rom.pod_prom_run_blocked(X, np.ones(512), [4.75], [0.02], 0.05, int(cols.max()), g40["Phi"], p)
        torch.cuda.synchronize()
        assert rel_l2(res.hist[0].cpu().numpy().T[:, cols], g40["U_" + tag]) < TOL, proj


@pytest.mark.parametrize("K", [131, 256])
def test_padding_and_full_width(thesis_bases, K):
    """The leading K modes of the same snapshots (K = 256 is the kernel's full width; 131 pads to 144)."""
    from burgers_hip import pod, rom
    X, _ = mesh(512)
    if K <= 227:
        Phi = thesis_bases[227][:, :K]
    else:                                          # beyond eps^2 = 1e-6: the same SVD truncated at 256
        Phi = pod.pod_basis(thesis_bases["S"], n_modes=K)[0].cpu().numpy()
    for proj in ("Galerkin", "LSPG"):
        res = rom.pod_prom_run_blocked(X, np.ones(512), [4.6, 5.2], [0.017, 0.026], 0.05, 4, Phi, rom.PROJ[proj.lower()])
        torch.cuda.synchronize()
        assert res.path == "bg_rom_run_blocked"
        check_pod_vs_oracle(res, X, 0.05, 4, [4.6, 5.2], [0.017, 0.026], Phi, proj)


def _fom_basis(X, E, K, nT=200):
    """An orthonormal basis built on mesh X from a short FOM run there (LAPACK's SVD: its trailing singular vectors stay
    orthonormal where the snapshots have next to no energy left)."""
    from burgers_hip import fom, pod
    mu1 = np.repeat(np.linspace(4.25, 5.5, 3), 3); mu2 = np.tile(np.linspace(0.015, 0.03, 3), 3)
    r = fom.fom_run(X, np.ones(len(X)), mu1, mu2, 0.05, nT, E=E)
    S = pod.snapshot_matrix(r.hist).cpu().numpy()
    return np.ascontiguousarray(np.linalg.svd(S, full_matrices=False)[0][:, :K])


def test_nonuniform_mesh_with_diffusion_and_small_mesh(hip):
    from burgers_hip import rom
    rng = np.random.default_rng(7)
    Xn = np.sort(np.concatenate([[0.0, 100.0], rng.uniform(0.0, 100.0, 298)]))
    assert len(Xn) == 300 and np.all(np.diff(Xn) > 0)
    Phi = _fom_basis(Xn, 0.5, 150)
    assert np.allclose(Phi.T @ Phi, np.eye(150), atol=1e-10)
    for proj in ("Galerkin", "LSPG"):
        res = rom.pod_prom_run_blocked(Xn, np.ones(300), [4.6, 5.2], [0.017, 0.026], 0.05, 4, Phi, rom.PROJ[proj.lower()],
                                       E=0.5)
        torch.cuda.synchronize()
        check_pod_vs_oracle(res, Xn, 0.05, 4, [4.6, 5.2], [0.017, 0.026], Phi, proj, E=0.5)
    X2, _ = mesh(200)
    Phi2 = _fom_basis(X2, 0.0, 120)
    assert np.allclose(Phi2.T @ Phi2, np.eye(120), atol=1e-10)
    for proj in ("Galerkin", "LSPG"):
        res = rom.pod_prom_run_blocked(X2, np.ones(200), [4.9], [0.022], 0.05, 4, Phi2, rom.PROJ[proj.lower()])
        torch.cuda.synchronize()
        check_pod_vs_oracle(res, X2, 0.05, 4, [4.9], [0.022], Phi2, proj)


def test_scheduling_and_workspace_reuse(thesis_bases):
    from burgers_hip import lib, rom
    X, _ = mesh(512)
    Phi = thesis_bases[160]
    dev = torch.device("cuda", torch.cuda.current_device())
    B = 20
    rng = np.random.default_rng(11)
    mu1, mu2 = rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B)
    p = rom.PROJ["lspg"]
    ref = rom.pod_prom_run_blocked(X, np.ones(512), mu1, mu2, 0.05, 3, Phi, p)
    same(rom.pod_prom_run_blocked(X, np.ones(512), mu1, mu2, 0.05, 3, Phi, p, balance=False), ref)
    small = rom.BlockedPodPlan(Phi, dev, slots=3)                   # 20 samples through 3 workspace slots
    first = rom.pod_prom_run_blocked(X, np.ones(512), mu1, mu2, 0.05, 3, small, p)
    again = rom.pod_prom_run_blocked(X, np.ones(512), mu1, mu2, 0.05, 3, first.plan, p)
    assert first.plan is small and again.plan is small
    same(first, ref)
    same(again, ref)
    # an order with entries outside the batch: those slots are skipped, the others are computed as ever
    L = lib.load()
    u0d = torch.ones((B, 512), dtype=torch.float64, device=dev)
    mu1d, mu2d = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev)
    Xd = torch.as_tensor(X, device=dev)
    hist = torch.full((B, 4, 512), -7.0, dtype=torch.float64, device=dev)
    iters = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    order = torch.arange(B, dtype=torch.int32, device=dev)
    order[3], order[11] = -1, B + 5
    rc = L.bg_rom_run_blocked(512, B, small.r, 3, p, lib.ptr(Xd), lib.ptr(small.PhiP), lib.ptr(u0d), lib.ptr(mu1d),
                              lib.ptr(mu2d), 0.05, 0.0, 1e-6, 20, lib.mesh_options(X, supg=True), lib.ptr(small.work),
                              small.slots, lib.ptr(hist), lib.ptr(iters), lib.ptr(flags), lib.ptr(info), lib.ptr(order),
                              lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    keep = [s for s in range(B) if s not in (3, 11)]
    assert torch.equal(hist[keep], ref.hist[keep]) and torch.equal(iters[keep], ref.iters[keep])
    assert torch.equal(flags[keep], ref.flags[keep]) and torch.equal(info[keep], ref.info[keep])
    assert bool((hist[[3, 11]] == -7.0).all())


def test_forced_handback_equals_library(thesis_bases):
    from burgers_hip import lib, rom
    X, _ = mesh(512)
    Phi = thesis_bases[160]
    mu1, mu2 = [4.5, 5.1, 5.45], [0.016, 0.024, 0.029]
    for proj in ("Galerkin", "LSPG"):
        f = rom.pod_prom_run_blocked(X, np.ones(512), mu1, mu2, 0.05, 3, Phi, rom.PROJ[proj.lower()],
                                     options=lib.BG_OPT_FORCE_PIVOTED)
        b = rom.pod_prom_run(X, np.ones(512), mu1, mu2, 0.05, 3, Phi, projection=proj, fused=False)
        torch.cuda.synchronize()
        assert f.redone == 3
        for k in ("hist", "iters", "flags"):
            assert torch.equal(getattr(f, k), getattr(b, k)), k


def test_refusals_before_launch(thesis_bases, monkeypatch):
    from burgers_hip import rom
    X, _ = mesh(512)
    dev = torch.device("cuda", torch.cuda.current_device())
    plan = rom.BlockedPodPlan(thesis_bases[160], dev)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    X4, _ = mesh(448)
    with pytest.raises(ValueError):
        rom.pod_prom_run_blocked(X4, np.ones(448), [5.0], [0.02], 0.05, 2, plan, rom.PROJ["lspg"])
    wide = np.concatenate([thesis_bases[227], thesis_bases[160][:, :30]], axis=1)
    assert wide.shape[1] == 257
    with pytest.raises(ValueError):
        rom.BlockedPodPlan(wide, dev)
    with pytest.raises(ValueError):
        rom.pod_prom_run_blocked(X, np.ones(512), [5.0], [0.02], 0.05, 2, wide, rom.PROJ["galerkin"])


def test_interface_opt_in_and_unchanged_default(thesis_bases):
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    X, T = mesh(512)
    Phi = thesis_bases[160]
    res = rom.pod_prom_run(X, np.ones(512), [4.8], [0.021], 0.05, 4, Phi, projection="LSPG", blocked=True)
    torch.cuda.synchronize()
    assert res.path == "bg_rom_run_blocked"
    check_pod_vs_oracle(res, X, 0.05, 4, [4.8], [0.021], Phi, "LSPG")
    U = FEMBurgers(X, T).pod_prom_burgers(0.05, 4, np.ones(512), 4.8, 0.0, 0.021, Phi, projection="Galerkin", blocked=True)
    Uo, _ = _oracle(X, 4, 4.8, 0.021, Phi, "Galerkin")
    assert rel_l2(np.asarray(U), Uo) < TOL
    default = rom.pod_prom_run(X, np.ones(512), [4.8], [0.021], 0.05, 2, Phi, projection="Galerkin")
    assert default.path == "library"
