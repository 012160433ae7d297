"""GPU parity of bg_quad_rom_run, the device-side quadratic-manifold PROM time loop (csrc/quad_fused.hip): four samples
per workgroup, tangent on fp64 MFMA with H3 streamed once per four sample-iterations, decode u = 1/2 (Phi q + T q).

Pinned against (i) the reference's committed PROM output and live reference runs (fixtures of tests/golden/make_golden.py),
(ii) the oracle (oracle/burgers_ref.py), (iii) the host-driven batched path (fused=False: bg_quad_tangent ->
bg_rom_reduce_frag -> bg_lu_solve_update -> decode GEMM), with identical Newton iteration counts, and (iv) itself:
every sample's result is bit-for-bit independent of which other samples share its workgroup or its launch.
reference: FEM/fem_burgers.py:1081-1175 (pod_quadratic_manifold), :263-312 (get_sym, get_dQ_dq).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, mesh, rel_l2
from oracle import burgers_ref as br

pytestmark = pytest.mark.gpu
TOL = 1e-10        # BASELINE north_star: <= 1e-10 relative L2 vs the reference


def _synthetic_manifold(N, n, seed, scale=2e-3):
    """A smooth orthonormal basis and a small quadratic tensor on an N-node mesh (sizes the committed fixtures lack)."""
    rng = np.random.default_rng(seed)
    xi = np.linspace(0, 1, N)
    cols = [np.ones(N), xi] + [np.tanh((xi - c0) * 10) for c0 in np.linspace(0.1, 0.9, n - 2)]
    Phi = np.linalg.qr(np.stack(cols, 1))[0]
    H = scale * rng.standard_normal((N, n * (n + 1) // 2))
    H -= Phi @ (Phi.T @ H)
    return Phi, H


def test_quad_fused_golden_and_live(hip):
    """The reference's committed n = 21 PROM output and live reference runs, both projections, iteration counts."""
    from burgers_hip import rom
    c = load_golden("committed_quadratic_n21.npz")
    live = load_golden("quadratic_live_n21.npz")
    X, _ = mesh(512)
    res = rom.quadratic_run(X, np.ones(512), float(c["mu1"]), float(c["mu2"]), 0.05, 6, c["Phi"], c["H"])
    torch.cuda.synchronize()
    assert res.path == "bg_quad_rom_run"                                 # the device-side loop ran
    assert rel_l2(res.hist[0].cpu().numpy().T, c["first7"]) < TOL
    for proj in ("Galerkin", "LSPG"):
        res = rom.quadratic_run(X, np.ones(512), float(live["mu1"]), float(live["mu2"]), float(live["At"]), int(live["nT"]),
                                c["Phi"], c["H"], projection=proj)
        torch.cuda.synchronize()
        assert res.path == "bg_quad_rom_run" and rel_l2(res.hist[0].cpu().numpy().T, live["U_" + proj]) < TOL
        assert np.array_equal(res.iters[0].cpu().numpy(), live["iters_" + proj])


@pytest.mark.parametrize("N,n,B,nT", [(512, 21, 9, 8), (512, 21, 4, 3), (200, 7, 5, 6), (257, 12, 2, 5), (64, 3, 1, 4), (330, 40, 6, 3)])
def test_quad_fused_vs_batched_path_and_oracle(hip, N, n, B, nT):
    """Ragged sizes (N not a multiple of 64 or 4, n < 40, batches that do not fill a workgroup), E != 0: the fused
    loop against the host-driven batched path (identical counts) and the oracle."""
    from burgers_hip import rom
    if (N, n) == (512, 21):
        c = load_golden("committed_quadratic_n21.npz")
        Phi, H = c["Phi"], c["H"]
    else:
        Phi, H = _synthetic_manifold(N, n, seed=N + n)
    X, _ = mesh(N)
    rng = np.random.default_rng(N + B)
    mu1 = rng.uniform(4.4, 5.3, B); mu2 = rng.uniform(0.017, 0.028, B)
    for proj in ("LSPG", "Galerkin"):
        f = rom.quadratic_run(X, np.ones(N), mu1, mu2, 0.04, nT, Phi, H, projection=proj, E=0.002)
        b = rom.quadratic_run(X, np.ones(N), mu1, mu2, 0.04, nT, Phi, H, projection=proj, E=0.002, fused=False)
        torch.cuda.synchronize()
        assert f.path == "bg_quad_rom_run" and b.path == "host"
        assert torch.equal(f.iters, b.iters) and torch.equal(f.flags, b.flags), proj
        assert rel_l2(f.hist.cpu().numpy(), b.hist.cpu().numpy()) < 1e-12, proj
        for s in range(min(B, 3)):
            U, ito = br.pod_quadratic_manifold(X, 0.04, nT, np.ones(N), mu1[s], 0.002, mu2[s], Phi, H, projection=proj,
                                               return_iters=True)
            assert rel_l2(f.hist[s].cpu().numpy().T, U) < TOL, (proj, s)
            assert np.array_equal(f.iters[s].cpu().numpy(), ito), (proj, s)


def test_quad_fused_sample_results_do_not_depend_on_the_batch(hip):
    """Bit for bit: a sample's trajectory is the same whether it runs alone, in another slot of a workgroup, or in a
    launch with more groups than compute units (the persistent loop over groups)."""
    from burgers_hip import rom
    c = load_golden("committed_quadratic_n21.npz")
    X, _ = mesh(512)
    rng = np.random.default_rng(8)
    B, nT = 1100, 3                                           # 275 groups > 256 CUs
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    plan = rom.QuadFusedPlan(c["Phi"], c["H"], torch.device("cuda", torch.cuda.current_device()))
    full = rom.quadratic_run(X, np.ones(512), mu1, mu2, 0.05, nT, c["Phi"], c["H"], plan=plan)
    perm = rng.permutation(B)
    shuf = rom.quadratic_run(X, np.ones(512), mu1[perm], mu2[perm], 0.05, nT, c["Phi"], c["H"], plan=plan)
    one = rom.quadratic_run(X, np.ones(512), mu1[777], mu2[777], 0.05, nT, c["Phi"], c["H"], plan=plan)
    torch.cuda.synchronize()
    assert bool((full.flags == 0).all())
    permd = torch.as_tensor(perm, device="cuda")
    assert torch.equal(full.hist[permd], shuf.hist) and torch.equal(full.iters[permd], shuf.iters)
    assert torch.equal(full.hist[777], one.hist[0]) and torch.equal(full.iters[777], one.iters[0])
    for s in (0, 555, 1099):
        U, ito = br.pod_quadratic_manifold(X, 0.05, nT, np.ones(512), mu1[s], 0.0, mu2[s], c["Phi"], c["H"], return_iters=True)
        assert rel_l2(full.hist[s].cpu().numpy().T, U) < TOL and np.array_equal(full.iters[s].cpu().numpy(), ito)


def test_quad_fused_cap_nonuniform_mesh_and_edge_cases(hip):
    from burgers_hip import lib, rom
    c = load_golden("committed_quadratic_n21.npz")
    X, _ = mesh(512)
    # the iteration cap: "Newton did not converge" (:1171) is a flag, not an error; counts equal the cap
    r = rom.quadratic_run(X, np.ones(512), [4.6, 5.1], [0.02, 0.024], 0.05, 3, c["Phi"], c["H"], newton_itmax=2)
    U, ito = br.pod_quadratic_manifold(X, 0.05, 3, np.ones(512), 4.6, 0.0, 0.02, c["Phi"], c["H"], newton_itmax=2, return_iters=True)
    torch.cuda.synchronize()
    assert bool((r.flags & lib.BG_FLAG_HIT_CAP).ne(0).all()) and np.array_equal(r.iters[0].cpu().numpy(), ito)
    # two Newton iterations from u0 = 1 leave the state far from the manifold's fixed point (values up to 19 against 5 on the
    # converged path): the unconverged iteration amplifies rounding differences -- measured 2.6e-10 -- hence 1e-8 here only
    assert rel_l2(r.hist[0].cpu().numpy().T, U) < 1e-8
    # graded mesh (per-element lengths in the assembly)
    N, n = 192, 6
    Phi, H = _synthetic_manifold(N, n, seed=3)
    Xg = 100.0 * np.linspace(0, 1, N) ** 1.3
    r = rom.quadratic_run(Xg, np.ones(N), [4.8, 5.0, 5.2], 0.021, 0.03, 5, Phi, H, E=0.01)
    torch.cuda.synchronize()
    for s, m1 in enumerate((4.8, 5.0, 5.2)):
        U, ito = br.pod_quadratic_manifold(Xg, 0.03, 5, np.ones(N), m1, 0.01, 0.021, Phi, H, return_iters=True)
        assert rel_l2(r.hist[s].cpu().numpy().T, U) < TOL and np.array_equal(r.iters[s].cpu().numpy(), ito)
    # empty batch, zero steps
    r = rom.quadratic_run(X, np.ones(512), np.zeros(0), np.zeros(0), 0.05, 2, c["Phi"], c["H"])
    assert r.hist.shape == (0, 3, 512)
    r = rom.quadratic_run(X, np.ones(512), 4.7, 0.02, 0.05, 0, c["Phi"], c["H"])
    torch.cuda.synchronize()
    assert r.hist.shape == (1, 1, 512) and torch.equal(r.hist[0, 0].cpu(), torch.ones(512, dtype=torch.float64))
    with pytest.raises(ValueError):
        rom.quadratic_run(X, np.ones(512), 4.7, 0.02, 0.05, 1, c["Phi"], c["H"][:, :-1])
    L = lib.load()
    assert L.bg_quad_rom_run(600, 1, 5, 1, 1, None, None, None, None, None, None, None, 0.05, 0.0, 1e-6, 25, 0, None, None, None, None,
                             None, None) == lib.BG_ERR_UNSUPPORTED_N
    assert L.bg_quad_rom_run(512, 1, 41, 1, 1, None, None, None, None, None, None, None, 0.05, 0.0, 1e-6, 25, 0, None, None, None, None,
                             None, None) == lib.BG_ERR_UNSUPPORTED_R
    assert L.bg_quad_rom_run(512, 1, 5, 1, 7, None, None, None, None, None, None, None, 0.05, 0.0, 1e-6, 25, 0, None, None, None, None,
                             None, None) == lib.BG_ERR_PROJECTION


def test_quad_fused_reduced_solve_pivots_like_numpy(hip):
    """A tangent basis whose reduced system needs row exchanges (columns far from orthogonal, growing downwards): the
    in-kernel Gauss-Jordan picks np.linalg.solve's pivots, the result equals the oracle's; and an exactly singular
    system (a repeated basis column) raises LinAlgError like numpy (:1161)."""
    from burgers_hip import rom
    N, n = 128, 5
    Phi, H = _synthetic_manifold(N, n, seed=11)
    rng = np.random.default_rng(2)
    Mix = np.eye(n) + 3.0 * np.triu(rng.standard_normal((n, n)), 1)
    Phi2 = np.ascontiguousarray((Phi @ Mix)[:, ::-1])
    X, _ = mesh(N)
    Ar = Phi2.T @ Phi2                                          # LSPG at A ~ M: the diagonal is NOT the column maximum
    assert np.abs(Ar[1:, 0]).max() > abs(Ar[0, 0])
    r = rom.quadratic_run(X, np.ones(N), [4.7, 5.1, 5.3], 0.02, 0.04, 3, Phi2, 0.0 * H, projection="LSPG")
    torch.cuda.synchronize()
    assert r.path == "bg_quad_rom_run"
    for s, m1 in enumerate((4.7, 5.1, 5.3)):
        U, ito = br.pod_quadratic_manifold(X, 0.04, 3, np.ones(N), m1, 0.0, 0.02, Phi2, 0.0 * H, return_iters=True)
        assert rel_l2(r.hist[s].cpu().numpy().T, U) < 1e-9 and np.array_equal(r.iters[s].cpu().numpy(), ito)
    Phi3 = Phi.copy(); Phi3[:, 3] = Phi3[:, 1]
    with pytest.raises(np.linalg.LinAlgError):
        rom.quadratic_run(X, np.ones(N), 4.7, 0.02, 0.04, 2, Phi3, 0.0 * H, projection="Galerkin")
