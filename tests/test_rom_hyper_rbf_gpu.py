"""bg_hyper_rbf_rom_run: the hyper-reduced POD-RBF PROM time loop on sampled mesh rows (csrc/rom_hyper_rbf.hip), against the
oracle (all rows, unit weights: the loop is then pod_rbf_prom itself), against the numpy restatement of the weighted-row
iteration (tests/hyper_rbf_ref.py) on a mesh beyond every other POD-RBF loop, and against bg_rbf_rom_run on the committed
closure.  reference: FEMBurgers.pod_rbf_prom, FEM/fem_burgers.py:1278-1398.

Everything is fp64, so the gate is the one of the other POD-RBF loops: rbf_long_cases.TOL = 1e-9 on the decoded history, q and
q_s, identical iteration counts, info == 0 and the reference's own cap pattern in the flags.  tests/test_rbf_row_sampling.py
shows on the CPU that the counts of every run compared here do not depend on the order of the sums or on operand noise."""
import numpy as np
import pytest
import torch

import hyper_rbf_ref as hrr
from conftest import mesh, rel_l2
from loop_cases import draw, to_np

pytestmark = pytest.mark.gpu
ENTRY, TOL = hrr.ENTRY, hrr.TOL
MAX_IT = 30


def run(X, dt, E, cl, kernel, s, proj, mu1, mu2, nT, **kw):
    from burgers_hip import rom
    res = rom.pod_rbf_run_hyper(X, np.ones(len(X)), mu1, mu2, dt, nT, *cl, s, rom.PROJ[proj.lower()], kernel=kernel, E=E, **kw)
    torch.cuda.synchronize()
    return res


def check_against(res, refs, Up, Us, what):
    """Every sample against its reference (U (N, nT+1), Q or None, Qs or None, iters): rel-L2 of the decoded history (and of q
    and q_s where the reference has them) below TOL, identical counts, info == 0, HIT_CAP exactly where the reference caps."""
    from burgers_hip import lib
    assert res.path == ENTRY and bool((res.info == 0).all())
    hist, q, qs, iters, flags = to_np(res.hist), to_np(res.q), to_np(res.q_s), to_np(res.iters), to_np(res.flags)
    for b, (U, Q, Qs, it) in enumerate(refs):
        err = rel_l2(hist[b].T, U)
        print(f"{what} m={res.plan.m} nodes={res.plan.n_nodes} sample {b}: rel-L2 {err:.2e}, iterations {iters[b].tolist()} / {it.tolist()}")
        assert err < TOL, (what, b, err)
        if Q is not None:
            assert rel_l2(q[b].T, Q) < TOL and rel_l2(qs[b].T[:, 1:], Qs[:, 1:]) < TOL and not qs[b, 0].any()
        assert np.array_equal(iters[b], it), (what, b)
        assert int(flags[b]) == (lib.BG_FLAG_HIT_CAP if it.max() >= MAX_IT else 0), (what, b, int(flags[b]))


def restatement(X, dt, E, cl, kernel, s, proj, mu1, mu2, nT):
    N = len(X)
    out = []
    for m1, m2 in zip(mu1, mu2):
        Q, Qs, it = hrr.hyper_rbf_prom(X, dt, nT, np.ones(N), m1, E, m2, *cl, proj, kernel, s.rows.numpy(), s.xi.numpy())
        out.append((hrr.decode(cl[0], cl[1], Q, Qs, np.ones(N)), Q, Qs, it))
    return out


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case,kernel", hrr.ALL_ROWS)
def test_all_rows_with_unit_weights_is_the_oracle(hip, case, kernel, proj):
    """full-256: m = N = 256 = NPAD of the S = 4 instantiation, the row limit, a uniform mesh read as a non-uniform one.
    perturbed-96: a ragged table on a graded mesh with diffusion."""
    from burgers_hip import lib
    from oracle import burgers_ref as br
    X, dt, E, cl = hrr.case_data(case, kernel)
    N, n, nbar, nT = len(X), 17, 79, hrr.NT_ALL
    mu1, mu2 = draw(3)
    res = run(X, dt, E, cl, kernel, hrr.sampling(np.arange(N), np.ones(N), proj), proj, mu1, mu2, nT)
    assert res.plan.m == N and res.plan.n_nodes == N and res.plan.wg_per_cu == 2
    assert tuple(res.q.shape) == (3, nT + 1, n) and tuple(res.q_s.shape) == (3, nT + 1, nbar)
    assert lib.mesh_is_uniform(X) == (case == "full-256")
    if case == "full-256":
        assert N == lib.limits("bg_hyper_rbf_rom_limits", 5)[3]
    assert np.array_equal(to_np(res.hist)[:, 0], np.ones((3, N)))                     # column 0 is u0 itself
    assert rel_l2(to_np(res.q[:, 0]), np.broadcast_to(cl[0].T @ np.ones(N), (3, n))) < 1e-14
    refs = []
    for s in range(3):
        U, ito = br.pod_rbf_prom(X, dt, nT, np.ones(N), mu1[s], E, mu2[s], *cl, projection=proj, kernel=kernel, return_iters=True)
        refs.append((U, None, None, ito))
    check_against(res, refs, cl[0], cl[1], f"{case} {kernel} {proj}")
    assert tuple(res.snapshots().shape) == (3, N, nT + 1)
    assert torch.equal(res.snapshots(), res.hist.transpose(1, 2))


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("kind", ["built", "limits"])
def test_sampled_rows_against_the_restatement(hip, kind, proj):
    """N = 2049, beyond every other POD-RBF loop, a closure fitted to that mesh.  "built": the builder's rows plus a few by
    hand (hyper_rbf_ref.long_sampling).  "limits": 256 rows and 767 table nodes, on the eight-wave instantiation."""
    from burgers_hip import lib
    X, dt, E, cl = hrr.long_data()
    s = hrr.long_sampling(kind, proj)
    mu1, mu2 = draw(2, seed=11)
    res = run(X, dt, E, cl, hrr.LONG_KERNEL, s, proj, mu1, mu2, hrr.NT_LONG)
    if kind == "limits":
        assert (res.plan.m, res.plan.n_nodes + 1) == lib.limits("bg_hyper_rbf_rom_limits", 5)[3:]      # 256 rows, 767 nodes
        assert res.plan.wg_per_cu == 1 and res.plan.UTn.shape[1] == 1024
    else:
        assert res.plan.wg_per_cu == 2 and res.plan.UTn.shape[1] == 512
    check_against(res, restatement(X, dt, E, cl, hrr.LONG_KERNEL, s, proj, mu1, mu2, hrr.NT_LONG), cl[0], cl[1], f"long-{kind} {proj}")


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_rows_left_out_of_the_perturbed_mesh(hip, proj):
    """perturbed-96 with rows 10, 50, 51 and 70 left out, unit weights: every node stays in the table, but from row 11 on a
    row that is only a neighbour sits between sampled ones -- it must assemble as nothing (weight 0, not the Dirichlet or
    the last row), and with row 10 gone the table position of a sampled row and its index among the sampled rows differ,
    which all-rows runs hide.  Kernel and samples per projection: hyper_rbf_ref.LEFT_OUT_RUNS, two of draw(10) at which the
    restatement converges in every one of the six steps, so all six are compared."""
    kernel, pick = hrr.LEFT_OUT_RUNS[proj]
    X, dt, E, cl = hrr.case_data("perturbed-96", kernel)
    rows = hrr.left_out_rows()
    s = hrr.sampling(rows, np.ones(len(rows)), proj)
    mu1, mu2 = (v[list(pick)] for v in draw(10))
    res = run(X, dt, E, cl, kernel, s, proj, mu1, mu2, hrr.NT_LEFT)
    assert res.plan.m == 92 and res.plan.n_nodes == len(X) and not bool(res.flags.any())
    check_against(res, restatement(X, dt, E, cl, kernel, s, proj, mu1, mu2, hrr.NT_LEFT), cl[0], cl[1], f"left-out {kernel} {proj}")


@pytest.mark.parametrize("proj,kernel", [("Galerkin", "gaussian"), ("LSPG", "imq")])
def test_committed_closure_against_the_full_loop(hip, proj, kernel):
    """N = 512, the builder's default sampling (200 rows, 366 .. 393 table nodes: the S = 8 four-wave instantiation): the
    hyper-reduced loop against bg_rbf_rom_run on the same batch.  The error is at most twice the CPU restatement's error
    against the oracle for the same sampling and samples."""
    from burgers_hip import rom
    from oracle import burgers_ref as br
    X, dt, cl = hrr.committed(kernel)
    s = hrr.committed_sampling(kernel, proj)
    B, nT = 4, 8
    mu1, mu2 = draw(B)
    hyp = run(X, dt, 0.0, cl, kernel, s, proj, mu1, mu2, nT)
    full = rom.pod_rbf_run_fused(X, np.ones(512), mu1, mu2, dt, nT, *cl, projection=proj, kernel=kernel)
    torch.cuda.synchronize()
    assert hyp.path == ENTRY and full.path == "bg_rbf_rom_run" and bool((hyp.info == 0).all())
    assert 256 < hyp.plan.n_nodes <= 512 and hyp.plan.wg_per_cu == 2
    hh, fh = to_np(hyp.hist), to_np(full.hist)
    for b in range(B):
        U = br.pod_rbf_prom(X, dt, nT, np.ones(512), mu1[b], 0.0, mu2[b], *cl, projection=proj, kernel=kernel)
        Q, Qs, _ = hrr.hyper_rbf_prom(X, dt, nT, np.ones(512), mu1[b], 0.0, mu2[b], *cl, proj, kernel, s.rows.numpy(), s.xi.numpy())
        cpu = rel_l2(hrr.decode(cl[0], cl[1], Q, Qs, np.ones(512)), U)
        err = rel_l2(hh[b].T, fh[b].T)
        print(f"{proj} {kernel} sample {b}: m = {s.m}, nodes = {hyp.plan.n_nodes}, rel-L2 {err:.2e} (restatement against the oracle: {cpu:.2e})")
        assert err <= 2.0 * cpu, (proj, b, err, cpu)


def left_out_run(B, **kw):
    kernel, _ = hrr.LEFT_OUT_RUNS["LSPG"]
    X, dt, E, cl = hrr.case_data("perturbed-96", kernel)
    rows = hrr.left_out_rows()
    mu1, mu2 = draw(B)
    s = kw.pop("s", None) or hrr.sampling(rows, np.ones(len(rows)), "LSPG")
    sel = kw.pop("sel", slice(None))
    return run(X, dt, E, cl, kernel, s, "LSPG", mu1[sel], mu2[sel], 3, **kw)


def test_a_trajectory_does_not_depend_on_the_batch(hip):
    """Alone, in a permuted batch, without the balanced order and in a batch larger than the grid: bit-identical."""
    B = 520
    big = left_out_run(B)
    assert B > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    perm = np.random.default_rng(2).permutation(B)
    shuffled = left_out_run(B, s=big.plan, sel=perm)
    assert shuffled.plan is big.plan
    for k in ("q", "q_s", "iters", "flags", "info"):
        assert torch.equal(getattr(shuffled, k), getattr(big, k)[torch.as_tensor(perm, device=big.q.device)]), k
    for b in (0, 7, B - 1):
        alone = left_out_run(B, s=big.plan, sel=slice(b, b + 1))
        for k in ("q", "q_s", "iters", "flags", "info"):
            assert torch.equal(getattr(alone, k)[0], getattr(big, k)[b]), (k, b)
    unbalanced = left_out_run(B, s=big.plan, balance=False)
    assert torch.equal(unbalanced.q, big.q) and torch.equal(unbalanced.q_s, big.q_s) and torch.equal(unbalanced.iters, big.iters)


def test_order_entries_outside_the_batch_are_skipped(hip):
    """The raw C call with order = [1, 4, 0, -3, 7] on a batch of five: samples 1, 4 and 0 are bit-equal to the wrapper's
    run, samples 2 and 3, which no slot names, keep what the caller put there."""
    from burgers_hip import lib, rom
    B, nT = 5, 3
    ref = left_out_run(B)
    p = ref.plan
    kernel, _ = hrr.LEFT_OUT_RUNS["LSPG"]
    X, dt, E, _ = hrr.case_data("perturbed-96", kernel)
    mu1, mu2 = draw(B)
    dev = ref.q.device
    f64 = dict(dtype=torch.float64, device=dev)
    u0 = torch.ones((B, p.N), **f64)
    q0 = rom._project_rows(u0, p.Up)
    u0n = u0[:, p.nodes].contiguous()
    mu1d, mu2d = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev)
    qh, qsh = torch.full((B, nT + 1, p.n), -7.0, **f64), torch.full((B, nT + 1, p.nbar), -7.0, **f64)
    iters = torch.full((B, nT), -5, dtype=torch.int32, device=dev)
    flags = torch.full((B,), -3, dtype=torch.int32, device=dev)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    order = torch.tensor([1, 4, 0, -3, B + 2], dtype=torch.int32, device=dev)
    rc = lib.load().bg_hyper_rbf_rom_run(
        p.N, B, p.n, p.nbar, p.Ns, p.m, p.n_nodes, nT, lib.BG_PROJ_LSPG, p.kind, lib.ptr(p.node), lib.ptr(p.xn), lib.ptr(p.pos),
        lib.ptr(p.xi), lib.ptr(p.UTn), lib.ptr(p.XtT), lib.ptr(p.Wd), lib.ptr(p.bias), lib.ptr(p.x_min), lib.ptr(p.dx), p.eps,
        lib.ptr(q0), lib.ptr(u0n), lib.ptr(mu1d), lib.ptr(mu2d), dt, E, 1e-6, MAX_IT, lib.mesh_options(X, supg=True),
        lib.ptr(qh), lib.ptr(qsh), lib.ptr(iters), lib.ptr(flags), lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    named, rest = [0, 1, 4], [2, 3]
    assert torch.equal(qh[named], ref.q[named]) and torch.equal(qsh[named], ref.q_s[named])
    assert torch.equal(iters[named], ref.iters[named]) and torch.equal(flags[named], ref.flags[named]) and bool((info == 0).all())
    assert bool((qh[rest] == -7.0).all()) and bool((qsh[rest] == -7.0).all())
    assert bool((iters[rest] == -5).all()) and bool((flags[rest] == -3).all())


def test_the_cap_is_flagged(hip):
    from burgers_hip import lib
    res = left_out_run(3, max_newton=2)
    assert bool((res.iters == 2).all()) and bool((res.flags == lib.BG_FLAG_HIT_CAP).all()) and bool((res.info == 0).all())


def test_routing_is_opt_in(hip):
    """pod_rbf_run(hyper=) with a sampling and with a plan, and the facade, reach the new entry and equal the direct call; a
    sampling trained for the other projection, another mesh and an unknown kernel are refused; without hyper= the paths
    are as before."""
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    kernel, nT = "imq", 3
    X, dt, E, cl = hrr.case_data("perturbed-96", kernel)
    N = len(X)
    s = hrr.sampling(np.arange(N), np.ones(N), "Galerkin")
    mu1, mu2 = draw(2)
    direct = run(X, dt, E, cl, kernel, s, "Galerkin", mu1, mu2, nT)
    kw = dict(projection="Galerkin", kernel=kernel, E=E)
    res = rom.pod_rbf_run(X, np.ones(N), mu1, mu2, dt, nT, *cl, hyper=s, **kw)
    assert res.path == ENTRY and torch.equal(res.q, direct.q) and torch.equal(res.q_s, direct.q_s) and torch.equal(res.hist, direct.hist)
    again = rom.pod_rbf_run(X, np.ones(N), mu1, mu2, dt, nT, *([None] * 9), hyper=res.plan, **kw)
    assert again.plan is res.plan and torch.equal(again.q, direct.q)
    T = mesh(N)[1]
    U = FEMBurgers(X, T).pod_rbf_prom(dt, nT, np.ones(N), mu1[0], E, mu2[0], *cl, projection="Galerkin", kernel=kernel, hyper=s)
    assert np.array_equal(U, to_np(direct.hist[0]).T)
    with pytest.raises(ValueError):
        rom.pod_rbf_run(X, np.ones(N), mu1, mu2, dt, nT, *cl, hyper=s, projection="LSPG", kernel=kernel, E=E)
    with pytest.raises(ValueError):
        rom.pod_rbf_run(X, np.ones(N), mu1, mu2, dt, nT, *cl, hyper=s, projection="Galerkin", kernel="cubic", E=E)
    X2 = X.copy(); X2[5] += 1e-3
    with pytest.raises(ValueError):
        rom.pod_rbf_run_hyper(X2, np.ones(N), mu1, mu2, dt, nT, *cl, res.plan, rom.PROJ["galerkin"], kernel=kernel, E=E)
    # without hyper= nothing routes here
    assert rom.pod_rbf_run(X, np.ones(N), mu1, mu2, dt, 2, *cl, **kw).path == "host"
    assert rom.pod_rbf_run(X, np.ones(N), mu1, mu2, dt, 2, *cl, fused=True, **kw).path == "bg_rbf_rom_run"
