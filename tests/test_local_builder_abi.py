"""CPU-side checks of the local POD builder: the new entry points (bg_kmeans_limits / _assign / _update,
bg_jacobi_sweep_batched) are exported, declared and validate their arguments before anything is launched, and
pod.kmeans / pod.build_local_bases / save_local_bases on CPU tensors reproduce the NumPy reference of local_builder_ref."""
import ctypes
import os
import re

import numpy as np
import pytest

import local_builder_ref as ref
from conftest import REPO
from loop_cases import built_library

NEW = ("bg_kmeans_limits", "bg_kmeans_assign", "bg_kmeans_update", "bg_jacobi_sweep_batched")


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_new_symbols_are_exported_declared_and_bound(L):
    from burgers_hip import lib
    header = open(os.path.join(REPO, "include", "burgers_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.bg_abi_version() == 1


def test_limits_are_those_of_the_device_loops(L):
    from burgers_hip import lib
    assert lib.limits("bg_kmeans_limits", 2) == (64, 64)
    assert lib.limits("bg_kmeans_limits", 2) == lib.limits("bg_local_rom_limits", 3)[1:]
    assert L.bg_kmeans_limits(None, None) == 0


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    null = None

    def assign(Ns=10, m=3, C=2, overlap=1.5):
        return L.bg_kmeans_assign(Ns, m, C, null, null, overlap, null, null, null, null, null)

    def update(Ns=10, m=3, C=2):
        return L.bg_kmeans_update(Ns, m, C, null, null, null, null, null)

    for f in (assign, update):
        assert f(Ns=0) == lib.BG_OK
        assert f(C=65) == lib.BG_ERR_UNSUPPORTED_R
        assert f(m=65) == lib.BG_ERR_UNSUPPORTED_R
        assert f(C=0) == lib.BG_ERR_BAD_ARG
        assert f(m=0) == lib.BG_ERR_BAD_ARG
        assert f(Ns=-1) == lib.BG_ERR_BAD_ARG
        assert f() == lib.BG_ERR_BAD_ARG                  # null pointers with points to work on
    assert assign(overlap=-0.5) == lib.BG_ERR_BAD_ARG
    assert assign(overlap=float("nan")) == lib.BG_ERR_BAD_ARG
    assert update(Ns=2 ** 31 - 1) == lib.BG_ERR_BAD_ARG

    def sweep(m=8, ld=8, count=2, stride=64, n_steps=7, n_pairs=4, tol=1e-15):
        return L.bg_jacobi_sweep_batched(m, ld, count, stride, null, null, null, n_steps, n_pairs, tol, null, null)

    assert sweep(count=0) == lib.BG_OK
    assert sweep(n_steps=0) == lib.BG_OK
    assert sweep(count=-1) == lib.BG_ERR_BAD_ARG
    assert sweep(m=0) == lib.BG_ERR_BAD_ARG
    assert sweep(ld=7) == lib.BG_ERR_BAD_ARG
    assert sweep(stride=63) == lib.BG_ERR_BAD_ARG         # consecutive matrices would overlap
    assert sweep(count=65536) == lib.BG_ERR_BAD_ARG
    assert sweep() == lib.BG_ERR_BAD_ARG                  # null pointers with work to do


@pytest.mark.parametrize("data", ["blobs", "trajectory"])
def test_kmeans_on_cpu_tensors_is_the_reference_lloyd(data):
    import torch
    from burgers_hip import pod
    Q = ref.blobs() if data == "blobs" else ref.smooth_trajectory()
    rows = np.random.default_rng(3).choice(len(Q), 4, replace=False)
    want = ref.lloyd(Q, Q[rows])
    assert want["converged"] and want["margin"] > 1e-9
    for kw in (dict(init=Q[rows]), dict(seed=3)):                              # init=None draws the same rows from the seed
        got = pod.kmeans(torch.from_numpy(Q), 4, **kw)
        assert got.n_iter == want["n_iter"] and got.converged and got.changed == want["changed"]
        assert np.array_equal(got.labels.numpy(), want["labels"])
        assert np.linalg.norm(got.cluster_centers_ - want["centres"]) <= 1e-13 * np.linalg.norm(want["centres"])
        assert abs(got.inertia - want["inertia"]) <= 1e-12 * want["inertia"]
        assert np.array_equal(got.predict(Q), want["labels"]) and got.predict(Q[5]).shape == (1,)
    one = pod.kmeans(torch.from_numpy(Q), 4, init=Q[rows], max_iter=1)
    assert not one.converged and one.n_iter == 1
    if want["n_iter"] > 1:
        assert np.array_equal(one.labels.numpy(), want["seq"][1])             # the labels of the centres it returns
    bad = Q.copy(); bad[7, 2] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        pod.kmeans(torch.from_numpy(bad), 4, init=Q[rows])
    with pytest.raises(np.linalg.LinAlgError):
        pod.kmeans(torch.from_numpy(Q), 4, init=bad[6:10])
    with pytest.raises(ValueError):
        pod.kmeans(torch.from_numpy(Q), 4, init=Q[:3])


def test_build_local_bases_on_cpu_tensors_and_the_file_round_trip(tmp_path):
    import torch
    from burgers_hip import pod
    S = ref.synthetic_snapshots()
    C, m, seed = 3, 4, 1
    rows = np.random.default_rng(seed).choice(S.shape[1], C, replace=False)
    want = ref.builder(S, C, m, rows, 1.5, 1e-4, 10)
    assert min(want["margins"]) > 1e-9, want["margins"]
    got = pod.build_local_bases(torch.from_numpy(S), C, m, epsilon_squared=1e-4, max_modes=10, seed=seed)
    assert np.array_equal(got.labels.numpy(), want["labels"]) and np.array_equal(got.kmeans.labels.numpy(), want["labels"])
    assert np.array_equal(got.member_bits.numpy().view(np.uint64), ref.member_words(want["mask"]))
    assert got.member_counts == want["mask"].sum(0).tolist()
    for c in range(C):
        assert np.array_equal(pod.member_mask(got.member_bits, c).numpy(), want["mask"][:, c])
        assert got.local_bases[c].shape == want["bases"][c].shape and got.local_bases[c].is_contiguous()
        assert np.abs(got.singular_values[c].numpy() - want["svals"][c]).max() <= 1e-12 * want["svals"][c][0]
    # the centres live in the coordinates of the builder's own U_global, whose column signs are its own
    sgn = np.sign((got.U_global.numpy()[:, :m] * want["U_global"][:, :m]).sum(0))
    assert np.linalg.norm(got.centres.numpy() * sgn - want["centres"]) <= 1e-13 * np.linalg.norm(want["centres"])
    # a given U_global: the centres to 1e-13
    given = pod.build_local_bases(torch.from_numpy(S), C, m, U_global=want["U_global"], n_modes=[3, 4, 5], seed=seed)
    assert np.linalg.norm(given.centres.numpy() - want["centres"]) <= 1e-13 * np.linalg.norm(want["centres"])
    assert [given.local_bases[c].shape[1] for c in range(C)] == [3, 4, 5]
    assert sorted(got.local_bases) == list(range(C)) and got.num_global_modes == m

    d = pod.save_local_bases(str(tmp_path / "local"), got)
    for f in sorted(os.listdir(d)):
        assert f.endswith((".npy", ".npz"))
        z = np.load(os.path.join(d, f), allow_pickle=False)                   # raises on an object array
        for k in (z.files if hasattr(z, "files") else ()):
            assert z[k].dtype != object
    back = pod.load_local_bases(d)
    for name in ("centres", "U_global", "labels", "member_bits"):
        a, b = getattr(got, name), getattr(back, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert list(back.local_bases) == list(range(C)) and back.member_counts == got.member_counts
    for c in range(C):
        assert torch.equal(back.local_bases[c], got.local_bases[c]) and back.local_bases[c].is_contiguous()
        assert torch.equal(back.singular_values[c], got.singular_values[c])
    assert (back.num_global_modes, back.overlap) == (got.num_global_modes, got.overlap)
    assert (back.kmeans.n_iter, back.kmeans.converged, back.kmeans.inertia, back.kmeans.changed) == \
        (got.kmeans.n_iter, got.kmeans.converged, got.kmeans.inertia, got.kmeans.changed)
    assert np.array_equal(back.kmeans.cluster_centers_, got.kmeans.cluster_centers_)


def test_builder_refuses_what_the_device_loops_cannot_take():
    import torch
    from burgers_hip import pod
    S = torch.from_numpy(ref.synthetic_snapshots())
    with pytest.raises(ValueError):
        pod.build_local_bases(S, 65, 4, n_modes=3)
    with pytest.raises(ValueError):
        pod.build_local_bases(S, 3, 65, n_modes=3)
    with pytest.raises(ValueError):
        pod.build_local_bases(S, 3, 4)                                        # neither a tolerance nor a width
    with pytest.raises(ValueError):
        pod.build_local_bases(S, 3, 4, n_modes=[3, 3])
    with pytest.raises(ValueError):
        pod.build_local_bases(S, 3, 4, n_modes=3, overlap=-1.0)
