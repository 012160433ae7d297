"""The Python frame the hyper-reduced loops share (burgers_hip/rom.py), without a GPU: every plan type refuses a malformed
row sampling before it touches the device, and the result base decodes, caches and reshapes as each loop's result did."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from loop_cases import built_library

N = 12
PLANS = ["HyperPodPlan", "HyperWidePodPlan", "HyperAnnPlan", "HyperRbfPlan", "HyperQuadPlan", "HyperLocalPlan"]


def plan_maker(name):
    """sampling -> the plan ``name`` on a 12-node non-uniform mesh, every other operand valid."""
    from burgers_hip import rom
    rng = np.random.default_rng(12)
    X = np.cumsum(rng.uniform(0.5, 1.5, N))
    Q = np.linalg.qr(rng.standard_normal((N, 5)))[0]                       # orthonormal columns; disjoint blocks are orthogonal
    torch.manual_seed(12)
    model = nn.Sequential(nn.Linear(2, 4), nn.ELU(), nn.Linear(4, 3)).eval()           # float32, two layers
    rbf = (rng.uniform(-1, 1, (3, 2)), rng.standard_normal((3, 3)), 1.0, -np.ones(2), np.ones(2), -np.ones(3), np.ones(3), "gaussian")
    cls = getattr(rom, name)
    return {
        "HyperPodPlan": lambda s: cls(Q[:, :3], s, X, None),
        "HyperWidePodPlan": lambda s: cls(Q[:, :3], s, X, None),
        "HyperAnnPlan": lambda s: cls(Q[:, :2], Q[:, 2:], model, s, X, None),
        "HyperRbfPlan": lambda s: cls(Q[:, :2], Q[:, 2:], *rbf, s, X, None),
        "HyperQuadPlan": lambda s: cls(Q[:, :2], Q[:, 2:], s, X, None),                # n = 2: H has 3 columns, Phi^T H = 0
        "HyperLocalPlan": lambda s: cls(rng.standard_normal((2, 2)), {0: Q[:, :3], 1: Q[:, 3:]}, Q[:, :4], 2, s, X, None),
    }[name]


@pytest.mark.parametrize("name", PLANS)
def test_every_plan_refuses_a_bad_sampling_before_the_device(name, monkeypatch):
    from burgers_hip import lib, pod
    built_library()

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(lib, "require_device", no_device)
    make = plan_maker(name)
    rs = lambda rows, xi, proj="galerkin": pod.RowSampling(np.array(rows, dtype=np.int32), np.array(xi, dtype=np.float64), proj, 0.0, 0, 0.0)
    with pytest.raises(AssertionError, match="device"):                    # the operands are valid: a good sampling goes on to the device
        make(rs([0, 3, 7], [1, 0.5, 2]))
    rows_msg, weights_msg = "ascending, distinct and in", "finite and >= 0"                   # each refusal for its own reason
    for bad, why in ((rs([0, 5, 5], [1, 1, 1]), rows_msg), (rs([0, 7, 3], [1, 1, 1]), rows_msg), (rs([0, N], [1, 1]), rows_msg),
                     (rs([-1, 3], [1, 1]), rows_msg), (rs([0, 3], [1, -0.5]), weights_msg), (rs([0, 3], [1, np.nan]), weights_msg),
                     (rs([], []), rows_msg), (rs([0, 3], [1]), rows_msg), (rs([0, 3, 7], [1, 0.5, 2], "petrov"), "projection must be")):
        with pytest.raises(ValueError, match=why):
            make(bad)
    if name == "HyperLocalPlan":
        with pytest.raises(ValueError, match="row 0"):
            make(rs([1, 3, 7], [1, 0.5, 2]))


def fake_run(q, iters):
    """What _device_loop hands a result class, on the host."""
    B = q.shape[0]
    return types.SimpleNamespace(hist=q, iters=iters, flags=torch.zeros(B, dtype=torch.int32), info=torch.zeros(B, dtype=torch.int32),
                                 path="fake", _keep=("operands",))


def ints(*shape, seed):
    """Small integers as float64: every product and sum of the decodes below is exact."""
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).double()


@pytest.mark.parametrize("kind", ["pod", "closure", "local"])
def test_result_base(kind, monkeypatch):
    from burgers_hip import fom, rom
    monkeypatch.setattr(fom, "transpose_batched", lambda t: t.transpose(1, 2).contiguous())       # the HIP transpose, on the host
    B, nT, n = 2, 3, 3
    q, u0 = ints(B, nT + 1, n, seed=1), ints(B, N, seed=2)
    iters = torch.tensor([[2, 3, 1], [4, 1, 2]], dtype=torch.int32)
    run = fake_run(q, iters)
    want = torch.empty((B, nT + 1, N), dtype=torch.float64)
    if kind == "pod":
        plan = types.SimpleNamespace(Phi=ints(N, n, seed=3))
        res = rom.HyperRomResult(run, plan, u0)
        for b in range(B):
            for k in range(nT + 1):
                want[b, k] = plan.Phi @ q[b, k]
        assert not hasattr(res, "redone")
    elif kind == "closure":
        plan = types.SimpleNamespace(Up=ints(N, n, seed=3), Us=ints(N, 2, seed=4))
        q_s = ints(B, nT + 1, 2, seed=5)
        res = rom.HyperClosureRomResult(run, plan, u0, q_s)
        assert res.q_s is q_s and rom.HyperAnnRomResult is rom.HyperRbfRomResult is rom.HyperClosureRomResult
        for b in range(B):
            for k in range(nT + 1):
                want[b, k] = plan.Up @ q[b, k] + plan.Us @ q_s[b, k]
    else:
        plan = types.SimpleNamespace(N=N, C=2, stack=ints(2, N, n, seed=3))
        clusters = torch.tensor([[0, 1, 1], [1, 1, 1]], dtype=torch.int32)                       # sample 0 switches, sample 1 does not
        res = rom.HyperLocalRomResult(run, plan, u0, clusters)
        assert res.clusters is clusters
        for b in range(B):
            for k in range(nT):
                want[b, k + 1] = plan.stack[clusters[b, k]] @ q[b, k + 1]
    want[:, 0] = u0
    assert res.q is q and res.iters is iters and res.plan is plan and res.path == "fake" and res._keep == ("operands",)
    hist = res.hist
    assert hist.dtype == torch.float64 and torch.equal(hist, want)
    assert torch.equal(hist[:, 0], u0) and res.hist is hist                # column 0 is u0 itself; decoded once and kept
    assert tuple(res.snapshots().shape) == (B, N, nT + 1) and torch.equal(res.snapshots(), want.transpose(1, 2))
    assert res.newton_steps == int(iters.sum()) == 13
