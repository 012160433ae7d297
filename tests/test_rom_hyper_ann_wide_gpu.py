"""bg_hyper_ann_rom_run_wide: the hyper-reduced POD-ANN PROM time loop for up to 20 primary modes on sampled mesh rows
(csrc/rom_hyper_ann_wide.hip), against the oracle (all rows, unit weights: the loop is then pod_ann_prom itself), against the
numpy restatement of the weighted-row iteration (tests/hyper_ann_ref.py) on a mesh beyond every other POD-ANN loop, one
sampling per instantiation, and against bg_ann_rom_run_wide on the reference's second model size.
reference: FEMBurgers.pod_ann_prom, FEM/fem_burgers.py:1177-1251, compute_ann_jacobian :1254-1275.

The closure and its Jacobian are float32 in the reference, the oracle and the kernel, so every comparison of a trajectory
is float32-limited: TOL32 = 5e-6 on the decoded history, on q and on q_s, iteration counts within 1 (the gate of
tests/test_ann_fused_gpu.py and tests/test_rom_hyper_ann_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

import ann_wide_cases as aw
import hyper_ann_ref as har
import hyper_ann_wide_cases as hw
from conftest import mesh, rel_l2
from hyper_ref import training_runs
from loop_cases import draw, initial_states, to_np

pytestmark = pytest.mark.gpu
ENTRY, NT, TOL32 = hw.ENTRY, hw.NT, aw.TOL32
sampling = hw.sampling


def _case(case):
    return hw.CASES[case] if isinstance(case, str) and case in hw.CASES else (har.CASES[case] if isinstance(case, str) else case)


def run(case, s, proj, mu1, mu2, nT=NT, u0=None, **kw):
    from burgers_hip import rom
    c = _case(case)
    N, dt, E = c[0], c[1], c[7]
    X, Up, Us, model = har.case_data(c)
    res = rom.pod_ann_run_hyper_wide(X, np.ones(N) if u0 is None else u0, mu1, mu2, dt, nT, Up, Us, model, s,
                                     rom.PROJ[proj.lower()], E=E, **kw)
    torch.cuda.synchronize()
    return res


def check_against_restatement(res, case, s, proj, mu1, mu2, nT=NT, u0=None, cap=50, **kw):
    """Every sample: rel-L2 of the decoded history against the restatement's below TOL32, q and q_s likewise, counts within
    1; the restatement stays below ``cap`` in every step, and the loop raises no flag.  Returns the restatement's counts."""
    c = _case(case)
    N, dt, E = c[0], c[1], c[7]
    X, Up, Us, model = har.case_data(c)
    Ws, bs = aw.weights(model)
    assert res.path == ENTRY and res.plan.m == s.m and bool((res.info == 0).all())
    hist, q, qs, iters = to_np(res.hist), to_np(res.q), to_np(res.q_s), to_np(res.iters)
    assert np.array_equal(qs[:, 0], np.zeros_like(qs[:, 0]))                     # no closure value belongs to u0
    counts = []
    for b in range(len(mu1)):
        start = np.ones(N) if u0 is None else u0[b]
        Q, Qs, it = har.hyper_ann_prom(X, dt, nT, start, mu1[b], E, mu2[b], Up, Us, Ws, bs, proj, s.rows.numpy(), s.xi.numpy(), **kw)
        err = rel_l2(hist[b].T, har.decode(Up, Us, Q, Qs, start))
        eq, eqs = rel_l2(q[b].T, Q), rel_l2(qs[b].T, Qs)
        print(f"N={N} m={s.m} nodes={res.plan.n_nodes} {proj} sample {b}: rel-L2 {err:.2e}, q {eq:.2e}, q_s {eqs:.2e}, "
              f"iterations {iters[b].tolist()} / {it.tolist()}, flags {int(res.flags[b])}")
        assert it.max() < cap and int(res.flags[b]) == 0, (proj, b)
        assert err < TOL32, (proj, b, err)
        assert eq < TOL32 and eqs < TOL32, (proj, b, eq, eqs)
        assert np.abs(iters[b] - it).max() <= 1, (proj, b)
        counts.append(it)
    return counts


def left_out_sampling(proj, N=96):
    rows = np.setdiff1d(np.arange(N), hw.LEFT_OUT)
    return sampling(rows, np.ones(len(rows)), proj)


# ---- 1. all rows, unit weights: the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(hw.CASES))
def test_all_rows_with_unit_weights_is_the_oracle(hip, case, proj):
    """wide-full-256: the reference's second model size, m = N = 256 (the row limit), a uniform mesh read as a non-uniform
    one.  wide-perturbed-96: n = 20, a non-uniform mesh with diffusion, a hidden width that is no multiple of 4."""
    from burgers_hip import lib
    from oracle import burgers_ref as br
    N, dt, n, nbar, _, _, _, E, _ = hw.CASES[case]
    X, Up, Us, model = har.case_data(hw.CASES[case])
    Ws, bs = aw.weights(model)
    mu1, mu2 = draw(3)
    res = run(case, sampling(np.arange(N), np.ones(N), proj), proj, mu1, mu2)
    assert res.path == ENTRY and res.plan.m == N and res.plan.n_nodes == N
    assert tuple(res.q.shape) == (3, NT + 1, n) and tuple(res.q_s.shape) == (3, NT + 1, nbar)
    assert lib.mesh_is_uniform(X) == (case == "wide-full-256")
    if case == "wide-full-256":
        assert N == lib.limits("bg_hyper_ann_rom_wide_limits", 6)[4]
    hist, iters = to_np(res.hist), to_np(res.iters)
    assert np.array_equal(hist[:, 0], np.ones((3, N)))                      # column 0 is u0 itself
    assert rel_l2(to_np(res.q[:, 0]), np.broadcast_to(Up.T @ np.ones(N), (3, n))) < 1e-14
    assert not bool(res.flags.any()) and bool((res.info == 0).all())
    for s in range(3):
        U, ito = br.pod_ann_prom(X, dt, NT, np.ones(N), mu1[s], E, mu2[s], Up, Us, Ws, bs, projection=proj, return_iters=True)
        err = rel_l2(hist[s].T, U)
        print(f"{case} {proj} sample {s}: rel-L2 {err:.2e}, iterations {iters[s].tolist()} / {ito.tolist()}")
        assert err < TOL32, (case, proj, s, err)
        assert np.abs(iters[s] - ito).max() <= 1
    assert tuple(res.snapshots().shape) == (3, N, NT + 1)


# ---- 2. sampled rows on N = 2049, one sampling per instantiation -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_sampling(kind, proj):
    """"built": build_ann_row_sampling's rows (training runs 0, 4, 8, every 10th step, min_rows = 120) plus rows added by hand
    with a small weight, so that 0, 1, N - 2, N - 1, an adjacent pair (700, 701) and an isolated row (1500) are present
    (at most 256 table nodes).  "spread": the same plus rows 12, 36, ..., 2028 (257 .. 512 table nodes).  "limits": rows 0, 8,
    ..., 2040 with weight 8 (row 0: 1): m = 256 and 767 table nodes, both limits at once."""
    from burgers_hip import pod
    N, dt = hw.LONG17[0], hw.LONG17[1]
    if kind == "limits":
        rows = np.arange(0, N - 1, 8)
        xi = np.full(len(rows), 8.0); xi[0] = 1.0
        assert len(rows) == 256
        return sampling(rows, xi, proj)
    X, Up, Us, model = har.case_data(hw.LONG17)
    s = pod.build_ann_row_sampling(X, Up, Us, model, training_runs(N, dt, keep=[0, 4, 8]), dt, proj, stride=10, min_rows=120)
    w = dict(zip(s.rows.tolist(), s.xi.tolist()))
    for extra in (0, 1, N - 2, N - 1, 700, 701, 1500) + (tuple(range(12, 2040, 24)) if kind == "spread" else ()):
        w.setdefault(extra, 0.05)
    rows = np.array(sorted(w), dtype=np.int32)
    assert len(rows) <= pod.hyper_ann_wide_rom_limits()[4]
    return sampling(rows, [w[int(i)] for i in rows], proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("kind", ["built", "spread", "limits"])
def test_sampled_rows_against_the_restatement(hip, kind, proj):
    from burgers_hip import lib
    s = long_sampling(kind, proj)
    mu1, mu2 = draw(2, seed=11)
    res = run(hw.LONG17, s, proj, mu1, mu2)
    nodes = res.plan.n_nodes
    print(f"{kind} {proj}: m = {s.m}, nodes = {nodes}")
    if kind == "built":
        assert nodes <= 256
    elif kind == "spread":
        assert 256 < nodes <= 512
    else:
        assert (res.plan.m, nodes + 1) == lib.limits("bg_hyper_ann_rom_wide_limits", 6)[4:]      # 256 rows, 767 nodes
    assert res.plan.wg_per_cu == lib.load().bg_hyper_ann_rom_wide_workgroups_per_cu(nodes)
    assert res.plan.UTn.shape == (17 + 79, lib.load().bg_hyper_ann_rom_wide_ut_ld(nodes))
    check_against_restatement(res, hw.LONG17, s, proj, mu1, mu2)


# ---- 3. rows left out: table position against row index --------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_rows_left_out_of_the_perturbed_mesh(hip, proj):
    """wide-perturbed-96 with rows 10, 50, 51 and 70 left out, unit weights: every node stays in the table, but from row 11 on
    a row that is only a neighbour sits between sampled ones -- it must assemble as nothing (weight 0, not the Dirichlet or
    the last row), and with row 10 gone the table position of a sampled row and its index among the sampled rows differ,
    which all-rows runs hide.  The restatement is 2.0e-2 .. 2.4e-2 away from the all-rows run here."""
    s = left_out_sampling(proj)
    mu1, mu2 = (v[[4, 5]] for v in draw(10))
    res = run("wide-perturbed-96", s, proj, mu1, mu2)
    assert res.plan.m == 92 and res.plan.n_nodes == 96
    check_against_restatement(res, "wide-perturbed-96", s, proj, mu1, mu2)


# ---- 4. N = 512, the thesis shape against the full loop ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_a_sampling(proj):
    from burgers_hip import pod
    X, Up, Us = aw.case_bases(aw.CASE_A)
    return pod.build_ann_row_sampling(X, Up, Us, aw.case_model(aw.CASE_A), training_runs(512, 0.05), 0.05, proj, tau=1e-4)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_thesis_shape_against_the_full_loop(hip, proj):
    """N = 512, n = 17, nbar = 79, the builder's sampling: the hyper-reduced loop against bg_ann_rom_run_wide on the same
    batch.  The error is at most twice the CPU restatement's error against the oracle for the same sampling and sample."""
    from burgers_hip import rom
    X, Up, Us = aw.case_bases(aw.CASE_A)
    model = aw.case_model(aw.CASE_A)
    Ws, bs = aw.weights(model)
    s = case_a_sampling(proj)
    B, nT, dt = 4, 12, 0.05
    mu1, mu2 = draw(B)
    p = rom.PROJ[proj.lower()]
    hyp = rom.pod_ann_run_hyper_wide(X, np.ones(512), mu1, mu2, dt, nT, Up, Us, model, s, p)
    full = rom.pod_ann_run_wide(X, np.ones(512), mu1, mu2, dt, nT, Up, Us, model, p)
    torch.cuda.synchronize()
    assert hyp.path == ENTRY and full.path == aw.WIDE and bool((hyp.info == 0).all())
    hh, fh = to_np(hyp.hist), to_np(full.hist)
    for b in range(B):
        U, _ = aw.oracle(aw.CASE_A, mu1[b], mu2[b], nT, proj)
        Q, Qs, _ = har.hyper_ann_prom(X, dt, nT, np.ones(512), mu1[b], 0.0, mu2[b], Up, Us, Ws, bs, proj, s.rows.numpy(), s.xi.numpy())
        cpu = rel_l2(har.decode(Up, Us, Q, Qs, np.ones(512)), U)
        err = rel_l2(hh[b].T, fh[b].T)
        print(f"{proj} sample {b}: m = {s.m}, nodes = {hyp.plan.n_nodes}, rel-L2 {err:.2e} (restatement against the oracle: {cpu:.2e})")
        assert err <= 2.0 * cpu, (proj, b, err, cpu)


# ---- 5. n <= 8 through the wide entry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_a_narrow_model_through_the_wide_entry(hip, proj):
    from oracle import burgers_ref as br
    case = "perturbed-96"
    N, dt, n, nbar, _, _, _, E, _ = har.CASES[case]
    assert n == 8
    X, Up, Us, model = har.case_data(case)
    Ws, bs = aw.weights(model)
    mu1, mu2 = draw(3)
    res = run(case, sampling(np.arange(N), np.ones(N), proj), proj, mu1, mu2)
    assert res.path == ENTRY and bool((res.info == 0).all())
    hist, iters = to_np(res.hist), to_np(res.iters)
    for s in range(3):
        U, ito = br.pod_ann_prom(X, dt, NT, np.ones(N), mu1[s], E, mu2[s], Up, Us, Ws, bs, projection=proj, return_iters=True)
        err = rel_l2(hist[s].T, U)
        print(f"{case} {proj} sample {s}: rel-L2 {err:.2e}, iterations {iters[s].tolist()} / {ito.tolist()}")
        assert err < TOL32, (proj, s, err)
        assert np.abs(iters[s] - ito).max() <= 1


# ---- 6. a trajectory does not depend on the batch --------------------------------------------------------------------------
def test_a_trajectory_does_not_depend_on_the_batch(hip):
    """Alone, in a permuted batch, and in a batch larger than the grid: bit-identical."""
    case, proj = "wide-perturbed-96", "LSPG"
    s = left_out_sampling(proj)
    B = 520
    mu1, mu2 = draw(B)
    big = run(case, s, proj, mu1, mu2)
    assert B > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    perm = np.random.default_rng(2).permutation(B)
    shuffled = run(case, big.plan, proj, mu1[perm], mu2[perm])
    assert shuffled.plan is big.plan
    for k in ("q", "q_s", "iters", "flags", "info"):
        assert torch.equal(getattr(shuffled, k), getattr(big, k)[torch.as_tensor(perm, device=big.q.device)]), k
    for b in (0, 7, B - 1):
        alone = run(case, big.plan, proj, mu1[b:b + 1], mu2[b:b + 1])
        for k in ("q", "q_s", "iters", "flags", "info"):
            assert torch.equal(getattr(alone, k)[0], getattr(big, k)[b]), (k, b)
    unbalanced = run(case, big.plan, proj, mu1, mu2, balance=False)
    for k in ("q", "q_s", "iters", "flags", "info"):
        assert torch.equal(getattr(unbalanced, k), getattr(big, k)), k


# ---- 7. controls and starts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_a_looser_tolerance(hip, proj):
    s = left_out_sampling(proj)
    mu1, mu2 = (v[[4, 5]] for v in draw(10))
    res = run("wide-perturbed-96", s, proj, mu1, mu2, tol=1e-3)
    counts = check_against_restatement(res, "wide-perturbed-96", s, proj, mu1, mu2, tol=1e-3)
    for it in counts:
        assert it.tolist() in ([4, 3, 3, 3, 3, 3], [4, 2, 2, 2, 2, 2])            # fewer than the default run's [6, 5, 5, 5, 5, 5]


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_the_cap_is_flagged(hip, proj):
    from burgers_hip import lib
    s = left_out_sampling(proj)
    mu1, mu2 = (v[[4, 5]] for v in draw(10))
    res = run("wide-perturbed-96", s, proj, mu1, mu2, max_it=3)
    assert bool((res.iters == 3).all()) and bool((res.flags == lib.BG_FLAG_HIT_CAP).all()) and bool((res.info == 0).all())
    c = hw.CASES["wide-perturbed-96"]
    X, Up, Us, model = har.case_data(c)
    Ws, bs = aw.weights(model)
    hist, q, qs = to_np(res.hist), to_np(res.q), to_np(res.q_s)
    for b in range(2):
        Q, Qs, it = har.hyper_ann_prom(X, c[1], NT, np.ones(96), mu1[b], c[7], mu2[b], Up, Us, Ws, bs, proj, s.rows.numpy(),
                                       s.xi.numpy(), max_it=3)
        err = rel_l2(hist[b].T, har.decode(Up, Us, Q, Qs, np.ones(96)))
        print(f"max_it=3 {proj} sample {b}: rel-L2 {err:.2e}, q {rel_l2(q[b].T, Q):.2e}, q_s {rel_l2(qs[b].T, Qs):.2e}")
        assert it.tolist() == [3] * NT
        assert err < TOL32 and rel_l2(q[b].T, Q) < TOL32 and rel_l2(qs[b].T, Qs) < TOL32


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_non_constant_starts_outside_the_span(hip, proj):
    """Six stored FOM states with a ripple on top (loop_cases.initial_states), one per sample; sample 3 caps in step 4 under
    Galerkin in the restatement and is left out, the other five converge in at most 8 iterations under both projections."""
    s = left_out_sampling(proj)
    keep = [0, 1, 2, 4, 5]
    u0 = initial_states(96, 0.05, 0.01, 7, 6)[keep]
    mu1, mu2 = (v[keep] for v in draw(6))
    assert np.ptp(u0, axis=1).min() > 0.1                                      # not constant
    res = run("wide-perturbed-96", s, proj, mu1, mu2, u0=u0)
    assert np.array_equal(to_np(res.hist[:, 0]), u0)
    counts = check_against_restatement(res, "wide-perturbed-96", s, proj, mu1, mu2, u0=u0, cap=9)
    assert max(int(it.max()) for it in counts) <= 8


# ---- 8. routing is opt-in --------------------------------------------------------------------------------------------------
def test_routing_is_opt_in(hip):
    """pod_ann_run(hyper=) with n = 20 and the facade reach the new entry; a sampling trained for the other projection,
    another mesh and a float64 closure are refused; n <= 8 still goes to bg_hyper_ann_rom_run."""
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    case = "wide-perturbed-96"
    N, dt, n, _, _, _, _, E, _ = hw.CASES[case]
    assert n == 20
    X, Up, Us, model = har.case_data(hw.CASES[case])
    s = sampling(np.arange(N), np.ones(N), "Galerkin")
    mu1, mu2 = draw(2)
    direct = run(case, s, "Galerkin", mu1, mu2)
    res = rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, NT, Up, Us, model, projection="Galerkin", E=E, hyper=s)
    assert res.path == ENTRY and isinstance(res.plan, rom.HyperAnnWidePlan)
    assert torch.equal(res.q, direct.q) and torch.equal(res.q_s, direct.q_s) and torch.equal(res.hist, direct.hist)
    again = rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, NT, None, None, None, projection="Galerkin", E=E, hyper=res.plan)
    assert again.plan is res.plan and again.path == ENTRY and torch.equal(again.q, direct.q) and torch.equal(again.q_s, direct.q_s)
    T = mesh(N)[1]
    U = FEMBurgers(X, T).pod_ann_prom(dt, NT, np.ones(N), mu1[0], E, mu2[0], Up, Us, model, projection="Galerkin", hyper=s)
    assert np.array_equal(U, to_np(direct.hist[0]).T)
    with pytest.raises(ValueError):
        rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, NT, Up, Us, model, projection="LSPG", E=E, hyper=s)
    with pytest.raises(ValueError):
        rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, NT, Up, Us, model, projection="Galerkin", E=E, hyper=s, ann_dtype=torch.float64)
    X2 = X.copy(); X2[5] += 1e-3
    with pytest.raises(ValueError):
        rom.pod_ann_run(X2, np.ones(N), mu1, mu2, dt, NT, Up, Us, model, projection="Galerkin", E=E, hyper=res.plan)
    with pytest.raises(ValueError):                                        # the narrow loop's plan keeps refusing n = 20
        rom.HyperAnnPlan(Up, Us, model, s, X, None)
    # without hyper= the same model routes as today: the host-driven iteration, or bg_ann_rom_run_wide with wide=True
    plain = rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, 2, Up, Us, model, projection="Galerkin", E=E)
    assert getattr(plain, "path", None) not in (ENTRY, hw.NARROW, aw.WIDE)
    assert rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, 2, Up, Us, model, projection="Galerkin", E=E, wide=True).path == aw.WIDE
    # n <= 8 with a sampling still takes the narrow loop
    c8 = "perturbed-96"
    X8, Up8, Us8, model8 = har.case_data(c8)
    r8 = rom.pod_ann_run(X8, np.ones(96), mu1, mu2, har.CASES[c8][1], 2, Up8, Us8, model8, projection="Galerkin", E=har.CASES[c8][7],
                         hyper=sampling(np.arange(96), np.ones(96), "Galerkin"))
    assert r8.path == hw.NARROW and isinstance(r8.plan, rom.HyperAnnPlan)
