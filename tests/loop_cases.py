"""What more than one device-loop test needs: the training snapshots and their singular vectors, the parameter draw, the
non-constant initial states, the comparisons of two results and of a POD loop with the oracle, the raw-ABI ``order`` and
plan-reuse checks of the streaming POD loops, the dense local clustering's widths, and the library handle and argument-validation check of the ABI tests.
The shapes each loop is tested at, and why, stay in that loop's test file.  torch and the oracle are imported where they are
used, so that the CPU-side ABI tests need neither."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import mesh, rel_l2

TOL = 1e-10
DENSE_WIDTHS = [8, 40, 17, 24, 12, 33, 25, 9, 40, 30, 20]


@functools.lru_cache(maxsize=None)
def training_snapshots(N, dt, E=0.0, seed=None):
    """(X, S, U): the mesh (``seed``: interior nodes moved by at most 0.2 h), the FOM snapshots (oracle, C) of the 3 x 3
    training grid over 200 steps, and all their left singular vectors.  One copy per process: callers slice it and leave it as it is."""
    from oracle import burgers_ref_c as brc
    X, _ = mesh(N)
    if seed is not None:
        X = X.copy()
        X[1:-1] += np.random.default_rng(seed).uniform(-0.2, 0.2, N - 2) * (100.0 / (N - 1))
    mu1 = np.repeat([4.25, 4.875, 5.5], 3); mu2 = np.tile([0.015, 0.0225, 0.03], 3)
    hist, _ = brc.fom_run(X, np.ones(N), mu1, mu2, dt, 200, E=E)
    S = np.ascontiguousarray(hist.reshape(-1, N).T)
    U = np.linalg.svd(S, full_matrices=False)[0]
    return X, S, U


def pod_basis(N, dt, r, E=0.0, seed=None):
    """(X, Phi): the mesh and the ``r`` leading left singular vectors of training_snapshots."""
    X, _, U = training_snapshots(N, dt, E, seed)
    return X, np.ascontiguousarray(U[:, :r])


def draw(B, seed=20251121):
    rng = np.random.default_rng(seed)
    return rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B)


RUN = [2, 6, 3, 7, 0, 8]
STEP = [20, 45, 70, 95, 120, 145]


def initial_states(N, dt, E, seed, B, steps=STEP):
    """(B, N) non-constant starts, one per sample, outside the span of a POD basis of training_snapshots(N, dt, E, seed): sample b
    is the stored FOM state of training run RUN[b] at step ``steps[b]`` (a moving front, at other parameters than draw(B) gives the
    sample) times 1 + 1e-3 sin((5 + 3 b) pi x / 100).  A new array: the caller may change it."""
    X, S, _ = training_snapshots(N, dt, E, seed)
    cols = [201 * RUN[b] + steps[b] for b in range(B)]
    wave = 1.0 + 1e-3 * np.sin((5 + 3 * np.arange(B))[:, None] * np.pi * X[None, :] / 100.0)
    return np.ascontiguousarray(S[:, cols].T * wave)


def to_np(t):
    return t.cpu().numpy()


def same(a, b):
    import torch
    for k in ("hist", "iters", "flags", "info"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def _worst(a, b):
    d, h = a.hist.flatten(1), b.hist.flatten(1)
    return float(((d - h).norm(dim=1) / h.norm(dim=1)).max())


def _margins(res, centres, Ug):
    """Relative gap between the best and second-best squared centre distance at the start of every step (host side)."""
    import torch
    u = res.hist[:, :-1].double()                                  # u^n of every step
    qg = u @ torch.as_tensor(Ug[:, :12], device=u.device)
    d = ((qg[:, :, None, :] - torch.as_tensor(centres, device=u.device)) ** 2).sum(-1)
    two = d.topk(2, dim=-1, largest=False).values
    return (two[..., 1] - two[..., 0]) / two[..., 1].clamp_min(1e-300)


def max_multiplier(X, dt, nT, mu1, mu2, Phi, proj, E):
    """Largest sub-diagonal multiplier of the unpivoted elimination over the systems of the reference's own run."""
    from oracle import burgers_ref as br
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


def check_pod_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, proj, E=0.0, samples=None, tol=TOL, u0=None):
    """Every listed sample (default: all) of a POD loop's result: rel-L2 of the history below ``tol``, every iteration count
    equal to the oracle's; no flag raised and no sample left marked.  ``u0``: the (B, N) starts of the run (None: ones)."""
    from oracle import burgers_ref as br
    hist, iters = to_np(res.hist), to_np(res.iters)
    for s in (range(len(mu1)) if samples is None else samples):
        start = np.ones_like(X, dtype=np.float64) if u0 is None else u0[s]
        U, ito = br.pod_prom_burgers(X, dt, nT, start, mu1[s], E, mu2[s], Phi, projection=proj, return_iters=True)
        err = rel_l2(hist[s].T, U)
        print(f"N={len(X)} r={Phi.shape[1]} {proj} sample {s}: rel-L2 {err:.2e}, iterations {iters[s].tolist()} / {ito.tolist()}")
        assert err < tol, (proj, s, err)
        assert np.array_equal(iters[s], ito), (proj, s)
    assert not bool(res.flags.any()) and bool((res.info == 0).all())


def check_order_entries_skipped(entry, ref, X, dt, mu1, mu2, p):
    """The raw entry point ``entry`` of a streaming POD loop with two entries of ``order`` outside [0, B), on the plan and
    inputs of the 3-step run ``ref``: the other samples are bit-equal to ``ref``, the rows of the samples no slot names keep
    what the caller put there."""
    import torch
    from burgers_hip import lib
    N, B, dev = len(X), len(mu1), ref.hist.device
    u0d = torch.ones((B, N), dtype=torch.float64, device=dev)
    mu1d, mu2d, Xd = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev), torch.as_tensor(X, device=dev)
    hist = torch.full((B, 4, N), -7.0, dtype=torch.float64, device=dev)
    iters = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    flags = torch.full((B,), -3, dtype=torch.int32, device=dev)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    order = torch.arange(B, dtype=torch.int32, device=dev)
    order[1], order[4] = -1, B + 5
    rc = getattr(lib.load(), entry)(N, B, ref.plan.r, 3, p, lib.ptr(Xd), lib.ptr(ref.plan.PhiP), lib.ptr(u0d), lib.ptr(mu1d),
                                    lib.ptr(mu2d), dt, 0.0, 1e-6, 20, lib.mesh_options(X, supg=True), lib.ptr(hist),
                                    lib.ptr(iters), lib.ptr(flags), lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    keep = [0, 2, 3, 5]
    assert torch.equal(hist[keep], ref.hist[keep]) and torch.equal(iters[keep], ref.iters[keep])
    assert torch.equal(flags[keep], ref.flags[keep]) and bool((info == 0).all())
    assert bool((hist[[1, 4]] == -7.0).all()) and bool((flags[[1, 4]] == -3).all())


def check_plan_reuse_restart_and_refusals(monkeypatch, run, Plan, entry, X, dt, Phi, other_r, too_long):
    """``run`` (rom.pod_prom_run_long or its wide sibling) with a basis and then with the plan that run built: the same plan
    object and the same bits; a run in two halves equals the run in one; a plan for another mesh or basis width, one column
    more than the loop takes and the mesh ``too_long`` (a shape) are refused with ValueError before anything is launched."""
    import torch
    from burgers_hip import rom
    N = len(X)
    mu1, mu2 = draw(5, seed=9)
    dev = torch.device("cuda", torch.cuda.current_device())
    p = rom.PROJ["lspg"]
    first = run(X, np.ones(N), mu1, mu2, dt, 5, Phi, p)
    again = run(X, np.ones(N), mu1, mu2, dt, 5, first.plan, p)
    torch.cuda.synchronize()
    assert again.plan is first.plan and again.path == entry
    if rom._ROUTES[entry].redo:
        assert first.redone == 0
    same(again, first)
    # restart: the second half of a run from the state the first half ended in
    head = run(X, np.ones(N), mu1, mu2, dt, 2, first.plan, p)
    tail = run(X, to_np(head.hist[:, -1]), mu1, mu2, dt, 3, first.plan, p)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([head.hist, tail.hist[:, 1:]], 1), first.hist)
    assert torch.equal(torch.cat([head.iters, tail.iters], 1), first.iters)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    X6, _ = mesh(600)
    with pytest.raises(ValueError):
        run(X6, np.ones(600), mu1, mu2, dt, 2, first.plan, p)                            # a plan for another N
    other = Plan(Phi[:600, :other_r], dev)                                               # another N and r
    with pytest.raises(ValueError):
        run(X, np.ones(N), mu1, mu2, dt, 2, other, p)
    with pytest.raises(ValueError):
        Plan(np.concatenate([Phi, Phi[:, :1]], axis=1), dev)                             # one column too many
    with pytest.raises(ValueError):
        Plan(np.zeros(too_long), dev)


def built_library():
    """The library, built if need be, and loaded: the ``L`` of the CPU-side ABI tests."""
    from burgers_hip import build, lib
    build.build_library()
    return lib.load()


def host_pointers():
    """(p, ip): a double and an int32 pointer into host memory that argument validation never reads."""
    buf, ibuf = (ctypes.c_double * 8)(), (ctypes.c_int32 * 8)()
    return ctypes.cast(buf, ctypes.POINTER(ctypes.c_double)), ctypes.cast(ibuf, ctypes.POINTER(ctypes.c_int32))


def check_pod_loop_argument_validation(L, entry, N, r, max_n, max_r, extra=()):
    """What every entry point with bg_rom_run's leading signature refuses before it launches anything, and with which
    code.  ``extra``: the arguments the entry takes between ``options`` and ``hist`` (bg_rom_run_blocked: work, slots).
    Returns the call it used, for the assertions particular to one entry."""
    from burgers_hip import lib
    null = None
    p, ip = host_pointers()

    def run(N=N, B=4, r=r, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.025, max_it=20, ops=p, hist=p, outs=ip, extra=extra):
        return getattr(L, entry)(N, B, r, nsteps, proj, ops, ops, ops, ops, ops, dt, 0.0, 1e-6, max_it, lib.BG_OPT_SUPG,
                                 *extra, hist, outs, outs, outs, null, null)

    assert run(N=2) == lib.BG_ERR_BAD_ARG
    assert run(r=0) == lib.BG_ERR_BAD_ARG
    assert run(nsteps=-1) == lib.BG_ERR_BAD_ARG
    assert run(max_it=0) == lib.BG_ERR_BAD_ARG
    assert run(dt=0.0) == lib.BG_ERR_BAD_ARG
    assert run(B=-1) == lib.BG_ERR_BAD_ARG
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=max_n + 1) == lib.BG_ERR_UNSUPPORTED_N
    assert run(r=max_r + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(ops=null) == lib.BG_ERR_BAD_ARG             # null operands, B > 0
    assert run(hist=null) == lib.BG_ERR_BAD_ARG            # null outputs, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(B=0, ops=null, hist=null, outs=null) == lib.BG_OK     # empty batch: nothing to do
    return run
