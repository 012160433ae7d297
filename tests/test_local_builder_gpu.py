"""The device-side local POD builder against the NumPy references of local_builder_ref: bg_kmeans_assign, bg_kmeans_update,
pod.kmeans, pod.jacobi_svd_batched (bitwise against jacobi_svd) and pod.build_local_bases end to end, into both device
loops of the local POD PROM.  Every reference input is checked here, on the host, to decide its labels and memberships
beyond rounding (margins above 1e-9), so no point is ever excluded from a comparison."""
import functools

import numpy as np
import pytest

import local_builder_ref as ref
from conftest import mesh, rel_l2

pytestmark = pytest.mark.gpu

MARGIN = 1e-9


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _assign(hip, Q, centres, overlap=None, labels=None):
    """The raw entry point: (labels, d2min, member words as uint64, changed)."""
    import torch
    L = hip.load()
    Ns, m = Q.shape
    lab = torch.full((Ns,), -1, dtype=torch.int32, device="cuda") if labels is None else _dev(labels, torch.int32)
    d2 = torch.empty((Ns,), dtype=torch.float64, device="cuda")
    bits = torch.zeros((Ns,), dtype=torch.int64, device="cuda") if overlap is not None else None
    changed = torch.zeros((1,), dtype=torch.int32, device="cuda")
    Qd, Cd = _dev(Q), _dev(centres)
    hip.check(L.bg_kmeans_assign(Ns, m, len(centres), hip.ptr(Qd), hip.ptr(Cd), overlap or 0.0, hip.ptr(lab), hip.ptr(d2),
                                 hip.ptr(bits), hip.ptr(changed), hip.stream_ptr(Qd.device)), "bg_kmeans_assign")
    torch.cuda.synchronize()
    return (lab.cpu().numpy(), d2.cpu().numpy(), None if bits is None else bits.cpu().numpy().view(np.uint64), int(changed.item()))


def _update(hip, Q, labels, centres):
    import torch
    L = hip.load()
    Qd, lab, cen = _dev(Q), _dev(labels, torch.int32), _dev(centres).clone()
    counts = torch.full((len(centres),), -1, dtype=torch.int32, device="cuda")
    hip.check(L.bg_kmeans_update(Q.shape[0], Q.shape[1], len(centres), hip.ptr(Qd), hip.ptr(lab), hip.ptr(cen), hip.ptr(counts),
                                 hip.stream_ptr(Qd.device)), "bg_kmeans_update")
    torch.cuda.synchronize()
    return cen.cpu().numpy(), counts.cpu().numpy()


def _points(Ns, m, C, seed=0):
    rng = np.random.default_rng([seed, Ns, m, C])
    return rng.normal(size=(Ns, m)), rng.normal(size=(C, m))


# (Ns, m, C): one point; a partial wave's worth of workgroups; a partial workgroup; the limits of both; more points than
# the largest grid holds waves (2048 workgroups of 4), so that every wave takes more than one trip
ASSIGN_SHAPES = [(1, 1, 1), (63, 5, 3), (257, 12, 4), (1000, 64, 64), (70000, 3, 7)]


@pytest.mark.parametrize("Ns,m,C", ASSIGN_SHAPES)
def test_assign_labels_distances_membership_and_changed(hip, Ns, m, C):
    Q, centres = _points(Ns, m, C)
    assert min(ref.margins(Q, centres, 1.5)) > MARGIN
    want_lab, want_mask = ref.members(Q, centres, 1.5)
    want_d2 = ref.d2_matrix(Q, centres).min(1)
    lab, d2, bits, changed = _assign(hip, Q, centres, overlap=1.5)
    assert np.array_equal(lab, want_lab)
    assert np.all(np.abs(d2 - want_d2) <= 1e-13 * want_d2)
    assert np.array_equal(bits, ref.member_words(want_mask))
    if C == 64:
        assert want_mask[:, 63].any() and not want_mask[:, 63].all()           # bit 63 is exercised both ways
    assert changed == Ns                                                        # every label differed from -1
    again = _assign(hip, Q, centres, labels=lab)
    assert again[3] == 0 and np.array_equal(again[0], lab) and again[2] is None
    assert np.array_equal(again[1], d2)
    other = lab.copy()
    flip = np.arange(0, Ns, 3)
    other[flip] = (other[flip] + 1) % (C + 1)                                   # C is no label at all: always a change
    assert _assign(hip, Q, centres, labels=other)[3] == len(flip)


def test_assign_takes_the_lower_of_two_identical_centres(hip):
    Q, centres = _points(300, 6, 5, seed=1)
    centres[3] = centres[1]
    assert ref.margins(Q, centres, ignore=(3,))[0] > MARGIN and ref.margins(Q, centres, 1.5)[1] > MARGIN
    want, want_mask = ref.members(Q, centres, 1.5)                              # np.argmin: the first index
    assert (want == 1).any() and not (want == 3).any()
    lab, _, bits, _ = _assign(hip, Q, centres, overlap=1.5)
    assert np.array_equal(lab, want)
    assert np.array_equal(bits, ref.member_words(want_mask))                    # the twin is a member wherever 1 is the label


# (Ns, m, C, empty cluster): a cluster of more than 1024 points (one full chunk and a remainder), of more than ten chunks,
# the limits of m and C, a single point
UPDATE_SHAPES = [(1, 1, 1, None), (63, 5, 3, 1), (5000, 12, 5, 2), (1000, 64, 64, 63), (70000, 3, 7, 0)]


@pytest.mark.parametrize("Ns,m,C,empty", UPDATE_SHAPES)
def test_update_means_counts_empty_cluster_and_reproducibility(hip, Ns, m, C, empty):
    Q, centres = _points(Ns, m, C, seed=2)
    used = [c for c in range(C) if c != empty]
    labels = np.asarray(used)[np.random.default_rng(5).integers(0, len(used), Ns)]
    want, want_counts = ref.means(Q, labels, centres)
    got, counts = _update(hip, Q, labels, centres)
    assert np.array_equal(counts, want_counts)
    for c in range(C):
        if want_counts[c] == 0:
            assert np.array_equal(got[c], centres[c])                           # kept, bitwise
        else:
            assert np.linalg.norm(got[c] - want[c]) <= 1e-13 * np.linalg.norm(want[c]), c
    assert np.array_equal(_update(hip, Q, labels, centres)[0], got)             # run to run
    # a cluster's sum depends on its own points and their order alone: take everybody else's points away
    for c in used[:2]:
        alone, n = _update(hip, Q[labels == c], labels[labels == c], centres)
        assert n[c] == want_counts[c] and np.array_equal(alone[c], got[c]), c


@functools.lru_cache(maxsize=None)
def _lloyd_case(data):
    Q = ref.blobs() if data == "blobs" else ref.smooth_trajectory()
    rows = np.random.default_rng(3).choice(len(Q), 4, replace=False)
    want = ref.lloyd(Q, Q[rows])
    assert want["converged"] and want["margin"] > MARGIN
    return Q, Q[rows].copy(), want


@pytest.mark.parametrize("data", ["blobs", "trajectory"])
def test_kmeans_follows_the_reference_lloyd(hip, data):
    import torch
    from burgers_hip import pod
    Q, init, want = _lloyd_case(data)
    Qd = _dev(Q)
    got = pod.kmeans(Qd, 4, init=init)
    assert got.labels.is_cuda and got.centres.is_cuda
    assert got.converged and got.n_iter == want["n_iter"] and got.changed == want["changed"]
    assert np.array_equal(got.labels.cpu().numpy(), want["labels"])
    assert np.linalg.norm(got.cluster_centers_ - want["centres"]) <= 1e-13 * np.linalg.norm(want["centres"])
    assert abs(got.inertia - want["inertia"]) <= 1e-12 * want["inertia"]
    # the labels of every pass: k passes and the closing assignment give the reference's pass k + 1
    for k in range(1, min(want["n_iter"], 6)):
        part = pod.kmeans(Qd, 4, init=init, max_iter=k)
        assert not part.converged and part.n_iter == k
        assert np.array_equal(part.labels.cpu().numpy(), want["seq"][k]), k
    assert torch.equal(got.predict(Qd), got.labels)
    assert np.array_equal(got.predict(Q), want["labels"])
    assert torch.equal(pod.kmeans(Qd, 4, seed=3).labels, got.labels)            # init=None: the same rows from the seed


def test_kmeans_refuses_nan_and_too_many_centres(hip):
    from burgers_hip import pod
    Q, init, _ = _lloyd_case("blobs")
    bad = Q.copy(); bad[11, 3] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        pod.kmeans(_dev(bad), 4, init=init)
    with pytest.raises(np.linalg.LinAlgError):
        pod.kmeans(_dev(Q), 4, init=bad[10:14])
    with pytest.raises(ValueError):
        pod.kmeans(_dev(Q), 65, seed=0)


def _cores(m):
    """A graded core of condition 1e10, one that is diagonal already, one of rank m / 2."""
    rng = np.random.default_rng(m)
    U = np.linalg.qr(rng.normal(size=(m, m)))[0]
    V = np.linalg.qr(rng.normal(size=(m, m)))[0]
    graded = (U * np.logspace(0, -10, m)) @ V.T
    diagonal = np.diag(np.linspace(2.0, 1.0, m))
    deficient = rng.normal(size=(m, m // 2)) @ rng.normal(size=(m // 2, m))
    return [graded, diagonal, deficient]


@pytest.mark.parametrize("m,count", [(96, 1), (96, 3), (65, 3)])
def test_batched_jacobi_is_bitwise_the_single_one(hip, m, count):
    """jacobi_svd is the batch of one matrix through the same driver and kernel, so this shows that a matrix of a batch does
    not depend on its batch-mates: floor, rotations, sweep count and every bit of the factors."""
    import torch
    from burgers_hip import pod
    Rs = _dev(np.stack(_cores(m)[:count]))
    info = {}
    U, s, Vh = pod.jacobi_svd_batched(Rs, info=info)
    for k in range(count):
        one = {}
        U1, s1, Vh1 = pod.jacobi_svd(Rs[k].clone(), info=one)
        assert torch.equal(U[k], U1) and torch.equal(s[k], s1) and torch.equal(Vh[k], Vh1), k
        assert info["sweeps"][k] == one["sweeps"], k
    assert info["rotations"][0][0] > 0
    if count == 3:
        assert all(r[1] == 0 for r in info["rotations"])                        # the diagonal one never rotates
        assert info["sweeps"][1] == 1 and len(info["rotations"]) == max(info["sweeps"]) > 1


# ---- end to end ---------------------------------------------------------------------------------------------------
E2E = dict(N=96, samples=6, steps=80, C=4, m=8, dt=0.05, seed=0)
LONG = dict(N=600, samples=3, steps=40, C=3, m=8, dt=0.05, seed=0)


@functools.lru_cache(maxsize=None)
def _snapshots(N, samples, steps, dt):
    """(X, mu1, mu2, S): FOM snapshots of the device solver, (N, samples * (steps + 1)), left as they are by every test."""
    from burgers_hip import fom, pod
    X, _ = mesh(N)
    mu1, mu2 = np.linspace(4.25, 5.5, samples), np.linspace(0.015, 0.03, samples)
    S = pod.snapshot_matrix(fom.fom_run(X, np.ones(N), mu1, mu2, dt, steps).hist).contiguous()
    return X, mu1, mu2, S


@functools.lru_cache(maxsize=None)
def _built(name):
    from burgers_hip import pod
    p = dict(E2E if name == "e2e" else LONG)
    X, mu1, mu2, S = _snapshots(p["N"], p["samples"], p["steps"], p["dt"])
    info = {}
    got = pod.build_local_bases(S, p["C"], p["m"], epsilon_squared=1e-4, max_modes=40, seed=p["seed"], info=info)
    rows = np.random.default_rng(p["seed"]).choice(S.shape[1], p["C"], replace=False)
    want = ref.builder(S.cpu().numpy(), p["C"], p["m"], rows, 1.5, 1e-4, 40)
    return p, X, mu1, mu2, S, got, want, info


def _gaps(want):
    """Smallest gap between consecutive retained singular values (and the first one dropped), relative to the largest."""
    worst = np.inf
    for c, B in want["bases"].items():
        s = want["svals"][c]
        K = B.shape[1]
        worst = min(worst, float(np.min(-np.diff(s[:K + 1])) / s[0]))
    return worst


def test_builder_matches_the_reference_builder(hip):
    import torch
    from burgers_hip import pod
    p, X, mu1, mu2, S, got, want, info = _built("e2e")
    assert min(want["margins"]) > MARGIN, want["margins"]
    # a singular vector moves by about (rounding of the matrix) / gap: 1e-15 / 1e-4 leaves a decade below the 1e-10 asked
    assert _gaps(want) > 1e-4, _gaps(want)
    assert want["kmeans"]["converged"] and got.kmeans.converged and got.kmeans.n_iter == want["kmeans"]["n_iter"]
    assert np.array_equal(got.labels.cpu().numpy(), want["labels"])
    assert np.array_equal(got.member_bits.cpu().numpy().view(np.uint64), ref.member_words(want["mask"]))
    assert got.member_counts == want["mask"].sum(0).tolist()
    assert info["batched"], "no cluster of at least N snapshots: the batched sweep was not exercised"
    for c in range(p["C"]):
        sw, sg = want["svals"][c], got.singular_values[c].cpu().numpy()
        n = min(len(sw), len(sg))
        assert np.abs(sg[:n] - sw[:n]).max() <= 1e-12 * sw[0], c
        Bw = torch.from_numpy(want["bases"][c])
        Bg = got.local_bases[c].cpu()
        assert Bg.shape == Bw.shape and got.local_bases[c].is_contiguous(), c
        err = float((pod.align_signs(Bg, Bw) - Bw).abs().max())
        print(f"cluster {c}: {got.member_counts[c]} snapshots, {Bg.shape[1]} modes, basis error {err:.2e}, sweeps {info['sweeps'][c]}")
        assert err <= 1e-10, (c, err)
    plain = pod.build_local_bases(S, p["C"], p["m"], epsilon_squared=1e-4, max_modes=40, seed=p["seed"], batched=False)
    for c in range(p["C"]):
        assert torch.equal(plain.local_bases[c], got.local_bases[c]), c
        assert torch.equal(plain.singular_values[c], got.singular_values[c]), c
    assert torch.equal(plain.member_bits, got.member_bits)


# Relative L2 difference between the local PROM on the builder's bases and on the reference-built ones (same loop, same
# mu), as measured on the MI355X; the gate is ten times that.
MEASURED = {"Galerkin": 2.085e-14, "LSPG": 2.200e-14}
BOUND = {k: 10.0 * v for k, v in MEASURED.items()}


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_built_bases_run_the_local_prom_like_the_reference_built_ones(hip, proj):
    """One training mu through bg_local_rom_run on the builder's clustering and on the NumPy-built one: the same clusters
    and iteration counts at every step, and trajectories within ten times the measured difference (2.085e-14 Galerkin,
    2.200e-14 LSPG relative L2 on the MI355X; column signs of a basis do not change its projection, so what is left is
    rounding).  The facade, given the k-means result object as ``kmeans``, returns the same bits."""
    import torch
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    p, X, mu1, mu2, S, got, want, _ = _built("e2e")
    N, nT, b = p["N"], p["steps"], 2                                           # one training mu
    res = rom.local_prom_run(X, np.ones(N), [mu1[b]], [mu2[b]], p["dt"], nT, got.centres, got.local_bases, got.U_global,
                             p["m"], projection=proj, fused=True)
    rf = rom.local_prom_run(X, np.ones(N), [mu1[b]], [mu2[b]], p["dt"], nT, want["centres"], want["bases"], want["U_global"],
                            p["m"], projection=proj, fused=True)
    torch.cuda.synchronize()
    assert res.path == "bg_local_rom_run" and rf.path == "bg_local_rom_run"
    assert not bool(res.flags.any()) and not bool(rf.flags.any())
    first = b * (nT + 1)                                                        # the initial condition's snapshot
    assert int(res.clusters[0, 0]) == int(got.labels[first]) == int(want["labels"][first])
    assert torch.equal(res.clusters, rf.clusters)
    assert torch.equal(res.iters, rf.iters)
    diff = rel_l2(res.hist[0].cpu().numpy(), rf.hist[0].cpu().numpy())
    fom_err = rel_l2(res.hist[0].cpu().numpy().T, S[:, first:first + nT + 1].cpu().numpy())
    print(f"{proj}: rel-L2 between builder-built and reference-built bases {diff:.3e}; against the FOM {fom_err:.3e}; "
          f"{len(torch.unique(res.clusters))} clusters visited")
    X_, T = mesh(N)
    U = FEMBurgers(X_, T).local_prom_burgers(p["dt"], nT, np.ones(N), mu1[b], 0.0, mu2[b], got.kmeans, got.local_bases,
                                             got.U_global, p["m"], projection=proj, fused=True)
    assert np.array_equal(np.asarray(U), res.hist[0].cpu().numpy().T)
    assert diff <= BOUND[proj], diff


def test_builder_refuses_more_than_64_centres_before_any_launch(hip, monkeypatch):
    from burgers_hip import pod
    _, _, _, _, S, _, _, _ = _built("e2e")

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(pod, "_assign", no_launch)
    monkeypatch.setattr(pod, "thin_svd", no_launch)
    with pytest.raises(ValueError):
        pod.build_local_bases(S, 65, 8, epsilon_squared=1e-4)


def test_builder_serves_the_long_mesh_loop(hip):
    import torch
    from burgers_hip import rom
    p, X, mu1, mu2, S, got, want, info = _built("long")
    assert min(want["margins"]) > MARGIN
    assert np.array_equal(got.labels.cpu().numpy(), want["labels"])
    assert max(b.shape[1] for b in got.local_bases.values()) <= 40
    N, nT, b = p["N"], p["steps"], 1
    res = rom.local_prom_run(X, np.ones(N), [mu1[b]], [mu2[b]], p["dt"], nT, got.centres, got.local_bases, got.U_global,
                             p["m"], projection="LSPG", fused=True, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == "bg_local_rom_run_long" and not bool(res.flags.any())
    first = b * (nT + 1)
    assert int(res.clusters[0, 0]) == int(got.labels[first])
    err = rel_l2(res.hist[0].cpu().numpy().T, S[:, first:first + nT + 1].cpu().numpy())
    print(f"N = {N}: local PROM on the built bases against its FOM run: rel-L2 {err:.3e}")
    assert np.isfinite(err)
