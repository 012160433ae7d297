"""pod_prom_run takes the route the table says ("Host side of the device-side loops") and hand-built plans
come back in ``res.plan``.  The numerics of every route have their own tests (test_rom_*_gpu.py)."""
import numpy as np
import pytest
import torch

from conftest import mesh

pytestmark = pytest.mark.gpu
B, NSTEPS = 3, 2


def _case(N, r):
    X, _ = mesh(N)
    Phi, _ = np.linalg.qr(np.random.default_rng(1000 * N + r).standard_normal((N, r)))
    u0 = np.ones(N)
    return X, u0, np.linspace(4.5, 5.2, B), np.linspace(0.018, 0.028, B), np.ascontiguousarray(Phi)


@pytest.mark.parametrize("N,r,flags,path", [
    (17, 3, {}, "bg_rom_run"),
    (64, 41, {}, "bg_rom_run_wide"),
    (128, 97, {"blocked": True}, "bg_rom_run_blocked"),
    (128, 97, {}, "library"),
    (513, 3, {"long_mesh": True}, "bg_rom_run_long"),
    (513, 3, {}, "library"),
])
def test_route_taken(hip, N, r, flags, path):
    from burgers_hip import rom
    X, u0, mu1, mu2, Phi = _case(N, r)
    res = rom.pod_prom_run(X, u0, mu1, mu2, 0.05, NSTEPS, Phi, **flags)
    torch.cuda.synchronize()
    assert res.path == path
    hist = res.hist.cpu().numpy()
    assert hist.shape == (B, NSTEPS + 1, N) and np.isfinite(hist).all()
    assert np.array_equal(hist[:, 0], np.broadcast_to(u0, (B, N)))


@pytest.mark.parametrize("N,r,plan_type,run", [(128, 97, "BlockedPodPlan", "pod_prom_run_blocked"),
                                               (513, 3, "LongPodPlan", "pod_prom_run_long")])
def test_hand_built_plan_is_returned(hip, N, r, plan_type, run):
    from burgers_hip import rom
    X, u0, mu1, mu2, Phi = _case(N, r)
    plan = getattr(rom, plan_type)(Phi, torch.device("cuda", torch.cuda.current_device()))
    res = getattr(rom, run)(X, u0, mu1, mu2, 0.05, NSTEPS, plan, rom.PROJ["galerkin"])
    torch.cuda.synchronize()
    assert res.plan is plan and (plan.N, plan.r) == (N, r) and tuple(plan.Phi.shape) == (N, r)
    assert bool(torch.isfinite(res.hist).all()) and bool((res.hist[:, 0] == 1.0).all())
