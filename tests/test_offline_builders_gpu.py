"""The offline basis builders on the device against host fp64 references of the same operation: the reference's
committed POD / quadratic-manifold artefacts, LAPACK, and oracle.burgers_ref.compute_H.

pod.thin_svd hands CPU tensors to LAPACK, so only device tensors reach the HIP kernel bg_jacobi_sweep.  The cases
cover the sizes the project builds at (m = 512 training core, 1024 x 808 bench gather), the kernel's strided loops
on two to four trips, a leading dimension above m, the single entry point as the batch of one, rank-deficient cores and
the refusals.
reference: POD/pod.py:8-14, :68-90; Quadratic_manifold/build_quadratic_manifold.py:25-48, quad_utils.py:63-81."""
import numpy as np
import pytest
import torch

from conftest import load_golden, mesh
from oracle import burgers_ref as br

pytestmark = pytest.mark.gpu
MAX_SWEEPS = 80                                   # pod.jacobi_svd's default limit
EPS = np.finfo(np.float64).eps


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _graded(m, rng, decades=10.0):
    U0, _ = np.linalg.qr(rng.standard_normal((m, m)))
    V0, _ = np.linalg.qr(rng.standard_normal((m, m)))
    s0 = np.logspace(0, -decades, m)
    return (U0 * s0) @ V0.T, s0


def _align(U, U_ref):
    """Flip columns of U (numpy) to match U_ref; singular vectors are defined up to sign."""
    sg = np.sign((U * U_ref).sum(0))
    sg[sg == 0] = 1
    return U * sg, sg


@pytest.fixture(scope="module")
def training_snapshots(hip):
    """The 9 training samples (3 x 3 mu grid of FEM/paper_training_stage.py:8-10, N = 512, dt 0.05, 500 steps) on the
    device, in the order the committed artefacts were built from; first pinned to the committed snapshot columns."""
    from burgers_hip import fom, pod
    N = 512
    X, _ = mesh(N)
    mu1 = np.repeat(np.linspace(4.25, 5.5, 3), 3); mu2 = np.tile(np.linspace(0.015, 0.03, 3), 3)
    res = fom.fom_run(X, np.ones(N), mu1, mu2, 0.05, 500)
    h = res.hist.cpu().numpy()
    gf = load_golden("committed_fom_n512.npz")
    for b, key in ((0, "4.250_0.0150"), (8, "5.500_0.0300")):
        assert np.linalg.norm(h[b].T[:, gf["cols"]] - gf["U_" + key]) < 1e-10 * np.linalg.norm(gf["U_" + key])
    return pod.snapshot_matrix(res.hist).contiguous()


def test_pod_basis_reproduces_committed_modes_on_device(training_snapshots):
    """Device QR + one-sided Jacobi on the m = 512 training core -> the committed s_all and 40-mode basis."""
    from burgers_hip import pod
    S = training_snapshots
    assert S.is_cuda and S.shape == (512, 9 * 501)
    info = {}
    pod.thin_svd(S, info=info)
    assert 0 < info["sweeps"] < MAX_SWEEPS                       # converged (non-convergence raises)
    g = load_golden("committed_pod_r40.npz")
    U, s, s_all = pod.pod_basis(S, epsilon_squared=1e-3)
    assert U.is_cuda and U.shape == (512, 40) and s.shape == (40,)
    s_all = s_all.cpu().numpy()
    ref = g["s_all"]
    assert np.all(np.diff(s_all) <= 0)
    assert np.abs(s_all[:len(ref)] - ref).max() < 1e-12 * ref[0]
    Ua, _ = _align(U.cpu().numpy(), g["Phi"])
    assert np.abs(Ua - g["Phi"]).max() < 1e-10


def test_quadratic_manifold_reproduces_committed_fit_on_device(training_snapshots):
    """Device build_quadratic_manifold(S, 21, 1e-2) -> the committed Phi and H, and H against the reference's own SVD
    filter-factor formula (oracle compute_H) evaluated on the host from the same Phi and snapshots."""
    from burgers_hip import pod
    S = training_snapshots
    q = load_golden("committed_quadratic_n21.npz")
    Phi, H, qd = pod.build_quadratic_manifold(S, 21, alpha=1e-2)
    assert Phi.is_cuda and H.is_cuda and Phi.shape == (512, 21) and H.shape == (512, 231)
    Phi, H = Phi.cpu().numpy(), H.cpu().numpy()
    Pa, sg = _align(Phi, q["Phi"])
    assert np.abs(Pa - q["Phi"]).max() < 1e-9
    I, J = np.triu_indices(21)
    H_ref = np.ascontiguousarray(q["H"])
    # 1e-8 holds on the host (test_dist_gloo); the device ridge solve (QR of [Q^T; alpha I]) lands H at 1.9e-8 of both
    # the committed H and the SVD formula on the same Phi (an eps-level perturbation of S moves LAPACK's H by 1.2e-10)
    assert np.linalg.norm(H * (sg[I] * sg[J]) - H_ref) < 5e-8 * np.linalg.norm(H_ref)
    Sh = S.cpu().numpy()
    qh = Phi.T @ Sh
    assert np.abs(qd.cpu().numpy() - qh).max() < 1e-12 * np.abs(qh).max()
    H_svd = br.compute_H(br.build_Q(qh), Sh - Phi @ qh, 1e-2)
    assert np.linalg.norm(H - H_svd) < 5e-8 * np.linalg.norm(H_svd)             # measured 1.9e-8 (compute_H docstring)


@pytest.mark.parametrize("m", [257, 512, 640, 777])
def test_jacobi_svd_core_real_sizes(hip, m):
    """test_jacobi_svd_core at sizes where every strided loop of the kernel takes two to four trips; 777 is odd, so
    every step holds one bye.  These cores need 40-46 sweeps.  Right factor and reconstruction keep the 1e-13 gates;
    the singular values and the accumulated left factor carry the rounding of ~m rotations per row and sweep, so
    their gates scale as 10 m eps (measured 2.5e-13 at m = 257 to 8e-13 at m = 777 on U^T U; LAPACK: 4e-15)."""
    from burgers_hip import pod
    A, s0 = _graded(m, np.random.default_rng(1000 + m))
    info = {}
    U, s, Vh = pod.jacobi_svd(_dev(A), info=info)
    assert 0 < info["sweeps"] < MAX_SWEEPS
    U, s, Vh = U.cpu().numpy(), s.cpu().numpy(), Vh.cpu().numpy()
    assert np.all(np.diff(s) <= 0)
    assert np.abs(s - s0).max() / s0[0] < 10 * m * EPS and np.abs(s / s0 - 1).max() < 1e-5
    assert np.abs(U.T @ U - np.eye(m)).max() < 10 * m * EPS and np.abs(Vh @ Vh.T - np.eye(m)).max() < 1e-13
    assert np.abs((U * s) @ Vh - A).max() < 1e-13


def test_jacobi_sweep_leading_dimension(hip):
    """bg_jacobi_sweep with ld = m + 37: the padding columns of G and J stay bitwise as they were, and one sweep gives
    bitwise the ld = m result (same rotations, same count)."""
    from burgers_hip import lib, pod
    L = lib.load()
    m, ld = 300, 337
    rng = np.random.default_rng(7)
    A, _ = _graded(m, rng)
    pairs = pod._round_robin(m).cuda()
    pad = _dev(rng.standard_normal((m, ld - m)))

    def sweep(ld_):
        G = torch.empty((m, ld_), dtype=torch.float64, device="cuda")
        J = torch.empty_like(G)
        G[:, m:] = pad[:, :ld_ - m]
        J[:, m:] = -pad[:, :ld_ - m]
        G[:, :m] = _dev(A)
        J[:, :m] = torch.eye(m, dtype=torch.float64, device="cuda")
        pad_G, pad_J = G[:, m:].clone(), J[:, m:].clone()
        rot = torch.zeros((1,), dtype=torch.int32, device="cuda")
        lib.check(L.bg_jacobi_sweep(m, ld_, lib.ptr(G), lib.ptr(J), lib.ptr(pairs), pairs.shape[0], pairs.shape[1],
                                    1e-15, lib.ptr(rot), lib.stream_ptr(torch.device("cuda"))), "bg_jacobi_sweep")
        torch.cuda.synchronize()
        return G, J, pad_G, pad_J, int(rot.item())

    G1, J1, _, _, r1 = sweep(m)
    G2, J2, pad_G, pad_J, r2 = sweep(ld)
    assert r1 == r2 and r1 > 0
    assert torch.equal(G2[:, m:], pad_G) and torch.equal(J2[:, m:], pad_J)
    assert torch.equal(G2[:, :m], G1) and torch.equal(J2[:, :m], J1)


def test_jacobi_sweep_is_the_batch_of_one(hip):
    """bg_jacobi_sweep forwards to the batched sweep: at m = 65 (odd: a bye in every step; more columns than one wave) and
    ld = 68, one sweep through bg_jacobi_sweep and through bg_jacobi_sweep_batched(count = 1, stride = m ld) leaves G, J,
    the padding columns (at their sentinel) and the rotation count bit for bit equal.  With count = 2 and stride = m ld + 11
    either matrix equals its count = 1 result, and the 11 doubles between the two stay at the sentinel."""
    from burgers_hip import lib, pod
    L = lib.load()
    m, ld, gap, sentinel = 65, 68, 11, -7.25
    rng = np.random.default_rng(65)
    cores = [_dev(_graded(m, rng)[0]) for _ in range(2)]
    pairs = pod._round_robin(m).cuda()
    stream = lib.stream_ptr(torch.device("cuda"))

    def sweep(mats, stride, batched):
        count = len(mats)
        G = torch.full(((count - 1) * stride + m * ld,), sentinel, dtype=torch.float64, device="cuda")
        J = G.clone()
        for k, A in enumerate(mats):
            G[k * stride:k * stride + m * ld].view(m, ld)[:, :m] = A
            J[k * stride:k * stride + m * ld].view(m, ld)[:, :m] = torch.eye(m, dtype=torch.float64, device="cuda")
        rot = torch.zeros((count,), dtype=torch.int32, device="cuda")
        if batched:
            lib.check(L.bg_jacobi_sweep_batched(m, ld, count, stride, lib.ptr(G), lib.ptr(J), lib.ptr(pairs), pairs.shape[0],
                                                pairs.shape[1], 1e-15, lib.ptr(rot), stream), "bg_jacobi_sweep_batched")
        else:
            lib.check(L.bg_jacobi_sweep(m, ld, lib.ptr(G), lib.ptr(J), lib.ptr(pairs), pairs.shape[0], pairs.shape[1], 1e-15,
                                        lib.ptr(rot), stream), "bg_jacobi_sweep")
        torch.cuda.synchronize()
        return G, J, rot.tolist()

    alone = []
    for A in cores:
        G1, J1, r1 = sweep([A], m * ld, batched=False)
        Gb, Jb, rb = sweep([A], m * ld, batched=True)
        assert r1 == rb and r1[0] > 0
        assert torch.equal(G1, Gb) and torch.equal(J1, Jb)                      # padding columns included
        for X in (G1, J1):
            assert bool((X.view(m, ld)[:, m:] == sentinel).all())
        assert not torch.equal(G1.view(m, ld)[:, :m], A)                        # the sweep did rotate
        alone.append((G1, J1, r1[0]))
    stride = m * ld + gap
    G2, J2, r2 = sweep(cores, stride, batched=True)
    for k, (G1, J1, r1) in enumerate(alone):
        assert r2[k] == r1, k
        assert torch.equal(G2[k * stride:k * stride + m * ld], G1) and torch.equal(J2[k * stride:k * stride + m * ld], J1), k
    assert bool((G2[m * ld:stride] == sentinel).all()) and bool((J2[m * ld:stride] == sentinel).all())


def test_jacobi_svd_rank_deficient(hip):
    """m = 300, rank 40 plus noise at 1e-17 relative: the 260 rows at the rounding level are left alone instead of
    rotated forever; converges, the 40 nonzero triplets match LAPACK and the left factor stays orthogonal."""
    from burgers_hip import pod
    m, k = 300, 40
    rng = np.random.default_rng(300)
    U0, _ = np.linalg.qr(rng.standard_normal((m, k)))
    V0, _ = np.linalg.qr(rng.standard_normal((m, k)))
    s0 = np.logspace(0, -3, k)
    A = (U0 * s0) @ V0.T
    A += 1e-17 * np.linalg.norm(A) * rng.standard_normal((m, m)) / m
    info = {}
    U, s, Vh = pod.jacobi_svd(_dev(A), info=info)
    assert 0 < info["sweeps"] < MAX_SWEEPS
    U, s, Vh = U.cpu().numpy(), s.cpu().numpy(), Vh.cpu().numpy()
    Ur, sr, Vhr = np.linalg.svd(A)
    assert np.all(np.diff(s) <= 0)
    assert np.abs(s - sr).max() < 1e-13 * sr[0]
    assert np.abs(s[:k] / sr[:k] - 1).max() < 1e-10
    assert np.abs(U.T @ U - np.eye(m)).max() < 1e-13
    Ua, sg = _align(U[:, :k], Ur[:, :k])
    assert np.abs(Ua - Ur[:, :k]).max() < 1e-10
    assert np.abs(Vh[:k] * sg[:, None] - Vhr[:k]).max() < 1e-10
    assert np.abs(Vh[:k] @ Vh[:k].T - np.eye(k)).max() < 1e-13
    assert np.abs((U * s) @ Vh - A).max() < 1e-13 * sr[0]


def test_jacobi_svd_exact_zero_rows(hip):
    """Rows that are exactly zero: no rotation touches them, the rest converges to LAPACK's triplets."""
    from burgers_hip import pod
    m = 200
    A, _ = _graded(m, np.random.default_rng(200), decades=6.0)
    zero = [0, 77, 150, 199]
    A[zero] = 0.0
    info = {}
    U, s, Vh = pod.jacobi_svd(_dev(A), info=info)
    assert 0 < info["sweeps"] < MAX_SWEEPS
    U, s, Vh = U.cpu().numpy(), s.cpu().numpy(), Vh.cpu().numpy()
    Ur, sr, Vhr = np.linalg.svd(A)
    k = m - len(zero)
    assert np.all(s[k:] == 0.0)
    assert np.abs(s - sr).max() < 1e-13 * sr[0] and np.abs(s[:k] / sr[:k] - 1).max() < 1e-7
    assert np.abs(U.T @ U - np.eye(m)).max() < 1e-13
    assert np.abs(U[zero][:, :k]).max() < 1e-13                   # the zero rows of A stay out of the range
    assert np.abs((U * s) @ Vh - A).max() < 1e-13 * sr[0]


def test_thin_svd_bench_gather_shape(hip):
    """The bench's allgather_svd block at world 1: 8 samples, every 5th level of a 500-step N = 1024 run (dt 0.025,
    bench.py's mu draw), N x 808, so thin_svd takes its tall branch and Jacobi runs an m = 808 rank-deficient core.
    Against host LAPACK: singular values to 1e-12 sigma_1, modes down to sigma/sigma_1 = 1e-8, the 1e-6 truncation."""
    from burgers_hip import fom, pod
    N = 1024
    X, _ = mesh(N)
    rng = np.random.default_rng(20251121)                         # bench.py SEED and mu_shard draw
    mu1 = rng.uniform(4.25, 5.5, 1024)[:8]; mu2 = rng.uniform(0.015, 0.03, 1024)[:8]
    res = fom.fom_run(X, np.ones(N), mu1, mu2, 0.025, 500)
    S = pod.snapshot_matrix(res.hist[:, ::5].contiguous()).contiguous()
    assert S.shape == (1024, 808)
    info = {}
    U, s, Vh = pod.thin_svd(S, info=info)
    assert 0 < info["sweeps"] < MAX_SWEEPS
    assert U.shape == (1024, 808) and s.shape == (808,) and Vh.shape == (808, 808)
    Sc = S.cpu().numpy()
    Uc, sc, _ = np.linalg.svd(Sc, full_matrices=False)
    s = s.cpu().numpy()
    assert np.all(np.diff(s) <= 0)
    assert np.abs(s - sc).max() < 1e-12 * sc[0]
    keep = int((sc / sc[0] > 1e-8).sum())
    assert keep > 50
    Ua, _ = _align(U[:, :keep].cpu().numpy(), Uc[:, :keep])
    assert np.abs(Ua - Uc[:, :keep]).max() < 1e-8
    Up, sp, _ = pod.pod_basis(S, epsilon_squared=1e-6)
    assert Up.shape[1] == br.n_modes_for_tolerance(sc, 1e-6)


def test_thin_svd_small_tall_factors(hip):
    """Tall branch on a small random case: U has orthonormal columns, Vh is orthogonal, U s Vh = A."""
    from burgers_hip import pod
    rng = np.random.default_rng(90)
    A = rng.standard_normal((90, 40))
    U, s, Vh = pod.thin_svd(_dev(A))
    U, s, Vh = U.cpu().numpy(), s.cpu().numpy(), Vh.cpu().numpy()
    assert U.shape == (90, 40) and Vh.shape == (40, 40)
    sr = np.linalg.svd(A, compute_uv=False)
    assert np.abs(s - sr).max() < 1e-13 * sr[0]
    assert np.abs(U.T @ U - np.eye(40)).max() < 1e-13 and np.abs(Vh @ Vh.T - np.eye(40)).max() < 1e-13
    assert np.abs((U * s) @ Vh - A).max() < 1e-13 * sr[0]


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_snapshots_refused(hip, bad):
    """np.linalg.svd raises LinAlgError on NaN / Inf; so do the device builders (a NaN row used to come back as a NaN
    mode)."""
    from burgers_hip import pod
    S = np.random.default_rng(3).standard_normal((64, 300))
    S[17, 123] = bad
    with pytest.raises(np.linalg.LinAlgError):
        pod.pod_basis(_dev(S), epsilon_squared=1e-6)
    with pytest.raises(np.linalg.LinAlgError):
        pod.thin_svd(_dev(S.T))                                  # the tall branch too
    with pytest.raises(np.linalg.LinAlgError):
        pod.jacobi_svd(_dev(S[:, 64:128]))                      # holds column 123


def test_jacobi_svd_reports_non_convergence(hip):
    """A graded m = 64 core cannot converge in one sweep: jacobi_svd must raise, naming the sweeps and rotations."""
    from burgers_hip import pod
    A, _ = _graded(64, np.random.default_rng(64))
    with pytest.raises(RuntimeError, match=r"not converged after 1 sweeps .* rotations in the last"):
        pod.jacobi_svd(_dev(A), max_sweeps=1)
