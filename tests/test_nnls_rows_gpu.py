"""pod.nnls_rows_device and the bg_nnls_* steps under it (csrc/nnls.hip) against pod.nnls_rows, the host's active-set NNLS.

Fixtures: the training matrices of pod.row_sampling_system on loop_cases.pod_basis and hyper_ref.training_runs.  On each of
them the smallest relative gap between the best and the second-best gradient entry over the whole fit is far above the 1e-12
by which a reordered sum moves an entry (9.4e-4 / 2.4e-4 at N = 96, 2.5e-4 / 6.9e-6 at N = 256, 5.8e-5 / 4.4e-5 at N = 600,
Galerkin / LSPG), so host and device must pick the same rows; the weights then agree to summation order, 1e-9 of the largest.
The pieces are held to bounds of their own: a dot product of ``rows`` terms to 1e-13 of sum |a_i| |r_i| (the bound of any
summation order is rows 2^-53 of it, 2.9e-14 at the 257 rows used), Q^T Q - I to 1e-13 in the 2-norm and the back-substituted
solution to 1e-11 of numpy's on columns with a condition number below 20."""
import functools

import numpy as np
import pytest
import torch

from hyper_ref import training_runs
from loop_cases import draw, pod_basis

pytestmark = pytest.mark.gpu

# (N, r, dt, keep, stride, tau, min_rows); the number of columns that leave during the fit, by projection
CASES = {"n96": (96, 17, 0.2, None, 10, 1e-4, None), "n256": (256, 40, 0.05, None, 10, 1e-3, 100),
         "n600": (600, 96, 0.05, (0, 4, 8), 20, 1e-3, 200)}
SHAPES = {"n96": (3060, 96), "n256": (7200, 256), "n600": (2880, 600)}
DROPS = {("n96", "galerkin"): 7, ("n96", "lspg"): 10, ("n256", "galerkin"): 2, ("n256", "lspg"): 0, ("n600", "galerkin"): 8,
         ("n600", "lspg"): 6}


@functools.lru_cache(maxsize=None)
def system(case, proj):
    """(G, pairs, tau, min_rows, max_rows, host): the training matrix and the host's RowSampling of it."""
    from burgers_hip import pod
    N, r, dt, keep, stride, tau, min_rows = CASES[case]
    X, Phi = pod_basis(N, dt, r)
    G, pairs = pod.row_sampling_system(X, Phi, training_runs(N, dt, keep=None if keep is None else list(keep)), dt, proj, 0.0, True, stride)
    assert G.shape == SHAPES[case]
    min_rows = min(3 * r, N) if min_rows is None else min_rows
    max_rows = pod.hyper_rom_limits()[1] if r <= pod.hyper_rom_limits()[0] else pod.hyper_wide_rom_limits()[1]
    return G, pairs, tau, min_rows, max_rows, pod._fit_row_sampling(G, pairs, proj, tau, min_rows, max_rows)


def nnls_arguments(G, tau, min_rows, max_rows):
    """What _fit_row_sampling hands to nnls_rows."""
    d = G.sum(axis=1)
    return (G[:, 1:], d - G[:, 0], float(tau) * float(np.linalg.norm(d)) / float(np.linalg.norm(d - G[:, 0])), max(min_rows - 1, 0),
            max_rows - 1)


def check_contract(G, s, tau, min_rows, max_rows):
    """The contract of test_row_sampling.py, recomputed from G in numpy."""
    rows, xi = s.rows.numpy(), s.xi.numpy()
    d = G.sum(axis=1)
    assert np.isfinite(xi).all() and (xi >= 0.0).all()
    assert (np.diff(rows) > 0).all() and rows[0] == 0 and xi[0] == 1.0
    assert min_rows <= s.m <= max_rows
    residual = np.linalg.norm(G[:, rows] @ xi - d) / np.linalg.norm(d)
    assert residual <= tau and abs(residual - s.residual) <= 1e-12


@pytest.mark.parametrize("proj", ["galerkin", "lspg"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_device_fit_picks_the_hosts_rows(hip, case, proj):
    from burgers_hip import pod
    G, pairs, tau, min_rows, max_rows, host = system(case, proj)
    dev = pod._fit_row_sampling(G, pairs, proj, tau, min_rows, max_rows, solver="device")
    info = {}
    x, rel = pod.nnls_rows_device(*nnls_arguments(G, tau, min_rows, max_rows), info=info)
    hx = host.xi.numpy()
    same = np.array_equal(dev.rows.numpy(), host.rows.numpy())
    worst = float(np.abs(dev.xi.numpy() - hx).max() / hx.max()) if same else float("nan")
    print(f"{case} {proj}: {dev.m} rows (host {host.m}), weights within {worst:.2e} of the largest, {info}")
    assert same
    assert worst <= 1e-9
    check_contract(G, dev, tau, min_rows, max_rows)
    # a second call: the same bits
    assert np.array_equal(np.flatnonzero(x > 0.0) + 1, dev.rows.numpy()[1:]) and np.array_equal(x[x > 0.0], dev.xi.numpy()[1:])
    assert info["adds"] - info["drops"] == dev.m - 1 and info["solves"] >= info["adds"] and info["dependent"] == 0
    assert info["drops"] >= min(DROPS[case, proj], 1)          # at least one wherever the host drops: the rebuild has run
    assert info["min_ratio"] > 1e-5                             # the dependence threshold is 2.3e-10


def test_more_rows_than_allowed_and_no_column_left(hip):
    from burgers_hip import pod
    G, pairs, tau, min_rows, _, _ = system("n96", "galerkin")
    with pytest.raises(ValueError, match="max_rows"):
        pod._fit_row_sampling(G, pairs, "galerkin", tau, min_rows, 20, solver="device")
    rng = np.random.default_rng(5)
    A = rng.random((40, 12))
    d = A @ (0.5 + rng.random(12))
    with pytest.raises(ValueError, match="no column left"):      # every column ends active
        pod.nnls_rows_device(A, d, 1e-10, 13, 30)
    with pytest.raises(ValueError, match="no column left"):
        pod.nnls_rows(A, d, 1e-10, 13, 30)
    info = {}
    x, rel = pod.nnls_rows_device(A, d, 1e-10, 12, 30, info=info)
    assert (x > 0.0).all() and rel <= 1e-10 and info["adds"] - info["drops"] == 12
    with pytest.raises(ValueError, match="max_cols"):
        pod.nnls_rows_device(A, d, 1e-10, 12, pod.nnls_limits()[0] + 1)


def test_a_duplicated_column_is_dependent_and_never_enters(hip):
    """A column in the span of the active ones has a zero gradient, so the iteration picks the copy only when nothing better
    is left: here in the fill phase of an exact fit (19 columns carry d, column 15 copies column 4, column 20 is spare,
    ``min_cols`` = 20), where rounding decides between the copy and the spare column and whether the spare column's weight
    comes out positive.  Over the seeds the copy never enters, every result returned satisfies the contract, and at least one
    run reports the copy as dependent and still returns (each seed does so with probability about 1/4)."""
    from burgers_hip import pod
    reported = returned = 0
    for seed in range(40):
        rng = np.random.default_rng(100 + seed)
        A = rng.random((60, 21))
        A[:, 15] = A[:, 4]
        xt = 0.5 + rng.random(21)
        xt[[15, 20]] = 0.0
        d = A @ xt
        info = {}
        try:
            x, rel = pod.nnls_rows_device(A, d, 1e-10, 20, 21, info=info)
        except ValueError as e:
            assert "no column left" in str(e)
            continue
        returned += 1
        assert x[15] == 0.0 and (x >= 0.0).all() and np.isfinite(x).all() and int((x > 0.0).sum()) == 20
        assert np.linalg.norm(A @ x - d) <= 1e-10 * np.linalg.norm(d) and rel <= 1e-10
        reported += info["dependent"]
    print(f"{returned} of 40 runs returned, the copy was reported dependent in {reported} of them")
    assert reported >= 1
    assert returned >= 8          # a run returns when the spare column's weight comes out positive: half of them (8 or fewer of 40: 1e-4)


def test_a_copy_of_an_active_column_is_reported_and_not_appended(hip):
    """The same through the steps, with nothing left to rounding: twelve columns active, column 4 among them, every other
    column tabu but its copy 15, so the pick is the copy; the append reports it dependent, marks it tabu and appends nothing,
    the solve queued behind it does nothing, and the next pick finds no column."""
    from burgers_hip import lib
    rng = np.random.default_rng(7)
    A = rng.random((60, 21))
    A[:, 15] = A[:, 4]
    d = A[:, :12] @ (0.5 + rng.random(12))
    ws = workspace(A, d, 21)
    ws.order[:12] = torch.arange(12, dtype=torch.int32)
    for c in range(12):
        ws.append(c, rebuild=True)
    ws.solve(12)
    st = ws.read()
    assert int(st["accepted"]) == 1 and int(st["count"]) == 12
    x12, Q12 = ws.x.clone(), ws.Q.clone()
    ws.tabu[12:] = 1
    ws.tabu[15] = 0
    ws.residual(12)
    ws.pick(float(np.linalg.norm(d)), 1.0, 20, 21)                      # tau = 1: the fill phase, any finite gradient is taken
    st = ws.read()
    assert int(st["pick"]) == 15 and int(st["stop"]) == lib.BG_NNLS_GO and int(st["fit_done"]) == 1
    ws.append(12)
    ws.solve(13)
    st = ws.read()
    print(f"the copy: |v| / |a| = {float(st['ratio']):.2e}")
    assert int(st["dependent"]) == 1 and int(st["count"]) == 12 and int(st["accepted"]) == 0 and int(st["stop"]) == lib.BG_NNLS_GO
    assert float(st["ratio"]) <= 1e-14                                  # far below the cut at 2.3e-10
    assert ws.tabu.tolist() == [0] * 12 + [1] * 9 and ws.active.tolist() == [1] * 12 + [0] * 9
    assert torch.equal(ws.x, x12) and torch.equal(ws.Q, Q12)            # nothing appended, nothing solved
    ws.pick(float(np.linalg.norm(d)), 1.0, 20, 21)
    st = ws.read()
    assert int(st["pick"]) == -1 and int(st["stop"]) == lib.BG_NNLS_NO_COLUMN


# ---- the pieces ---------------------------------------------------------------------------------------------------------------
def workspace(G, d, kmax):
    from burgers_hip import pod
    return pod.NnlsWorkspace(G, d, kmax)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_gradient_and_pick(hip, rows, n):
    from burgers_hip import lib
    rng = np.random.default_rng(rows * 100 + n)
    G, res = rng.standard_normal((rows, n)), rng.standard_normal(rows)
    ws = workspace(G, res, 4)
    want = G.T @ res
    bound = 1e-13 * (np.abs(G).T @ np.abs(res))

    def pick(active=(), tabu=()):
        ws.active.zero_(); ws.tabu.zero_()
        if len(active):
            ws.active[torch.as_tensor(active, device=ws.device)] = 1
        if len(tabu):
            ws.tabu[torch.as_tensor(tabu, device=ws.device)] = 1
        ws.pick(2.0 * np.linalg.norm(res), 1e-3, 0, 4)
        return ws.read(), ws.w.cpu().numpy()

    st, w = pick()
    assert (np.abs(w - want) <= bound).all()
    assert int(st["pick"]) == int(np.argmax(want)) and abs(float(st["w"]) - want.max()) <= bound.max()
    assert abs(float(st["resnorm"]) - np.linalg.norm(res)) <= 1e-14 * np.linalg.norm(res)
    assert float(st["rel"]) == float(st["resnorm"]) / (2.0 * np.linalg.norm(res)) and int(st["fit_done"]) == 0
    assert int(st["stop"]) == (lib.BG_NNLS_GO if want.max() > 0.0 else lib.BG_NNLS_NO_COLUMN)
    if n > 1:
        order = np.argsort(-want)
        st, w = pick(active=order[:1], tabu=order[1:3])                   # the three best masked: the fourth is picked
        assert int(st["pick"]) == int(order[3])
        keep = np.setdiff1d(np.arange(n), order[:3])
        assert (np.abs(w[keep] - want[keep]) <= bound[keep]).all()
        # an exact tie between two columns that beat the rest: the lower index wins
        hi, lo = int(order[0]), int(order[5])
        G2 = G.copy()
        G2[:, lo] = G2[:, hi]
        tie = workspace(G2, res, 4)
        tie.pick(1.0, 1e-3, 0, 4)
        assert int(tie.read()["pick"]) == min(hi, lo)
    st, _ = pick(active=np.arange(n))                                     # every column masked: reported
    assert int(st["pick"]) == -1 and int(st["stop"]) == lib.BG_NNLS_NO_COLUMN and float(st["w"]) == -np.inf


@pytest.mark.parametrize("k", [1, 2, 64, 65])
def test_append_then_solve(hip, k):
    rows = 131
    rng = np.random.default_rng(k)
    A = np.linalg.qr(rng.standard_normal((rows, k)))[0] @ (np.eye(k) + 0.3 * rng.random((k, k)) / k)      # condition number < 20
    assert np.linalg.cond(A) < 20.0
    xt = 0.5 + rng.random(k)
    b = A @ xt + 0.1 * rng.standard_normal(rows)
    ws = workspace(A, b, k)
    ws.order.copy_(torch.arange(k, dtype=torch.int32))
    for c in range(k):
        ws.append(c, rebuild=True)                                         # the columns in the order 0 .. k - 1
    ws.solve(k)
    st = ws.read()
    Q, R = ws.Q[:, :rows].cpu().numpy().T, np.triu(ws.R.cpu().numpy().T)
    s = np.linalg.lstsq(A, b, rcond=None)[0]
    assert s.min() > 0.0
    assert int(st["count"]) == k and int(st["accepted"]) == 1 and int(st["p0"]) == k
    assert np.linalg.norm(Q.T @ Q - np.eye(k), 2) <= 1e-13
    assert np.linalg.norm(Q @ R - A) <= 1e-13 * np.linalg.norm(A) and (np.diag(R) > 0.0).all()
    assert np.abs(ws.z.cpu().numpy() - Q.T @ b).max() <= 1e-13 * np.linalg.norm(b)
    assert np.abs(ws.x.cpu().numpy() - s).max() <= 1e-11 * np.abs(s).max()
    assert bool((ws.active == 1).all())
    ws.residual(k)
    assert np.abs(ws.res[:rows].cpu().numpy() - (b - A @ s)).max() <= 1e-12 * np.linalg.norm(b)


def test_two_entries_reaching_zero_at_once_both_leave(hip):
    """Unit columns, so Q = R = I and s = b.  From x = (1, 1, 1, 1) towards s = (2, -1, 3, -1): both negative entries have the
    ratio 1/2, the step is x + (s - x) / 2 = (1.5, 0, 2, 0), exactly, and positions 1 and 3 leave."""
    A = np.eye(6)[:, :4]
    b = np.array([2.0, -1.0, 3.0, -1.0, 0.5, 0.0])
    ws = workspace(A, b, 4)
    ws.order.copy_(torch.tensor([2, 0, 3, 1], dtype=torch.int32))         # insertion order: columns 2, 0, 3, 1
    for c in range(4):
        ws.append(c, rebuild=True)
    ws.x.fill_(1.0)
    ws.solve(4)
    st = ws.read()
    # in insertion order s = (3, 2, -1, -1): positions 2 and 3 (columns 3 and 1) leave
    assert int(st["accepted"]) == 0 and int(st["count"]) == 2 and int(st["p0"]) == 2 and int(st["stop"]) == 0
    assert ws.order[:2].tolist() == [2, 0] and ws.x[:2].tolist() == [2.0, 1.5]
    assert ws.active.tolist() == [1, 0, 1, 0]
    ws.solve(2)                                                            # what stays is solved again and accepted
    st = ws.read()
    assert int(st["accepted"]) == 1 and int(st["count"]) == 2 and ws.x[:2].tolist() == [3.0, 2.0]
    ws.residual(2)
    assert ws.res[:6].tolist() == [0.0, -1.0, 0.0, -1.0, 0.5, 0.0]
    # a drop in the middle: positions behind it move up and the QR is valid up to p0 only
    ws = workspace(A, np.array([2.0, -1.0, 3.0, 4.0, 0.0, 0.0]), 4)
    ws.order.copy_(torch.tensor([0, 1, 2, 3], dtype=torch.int32))
    for c in range(4):
        ws.append(c, rebuild=True)
    ws.x.fill_(1.0)
    ws.solve(4)
    st = ws.read()
    assert int(st["accepted"]) == 0 and int(st["count"]) == 3 and int(st["p0"]) == 1
    assert ws.order[:3].tolist() == [0, 2, 3] and ws.x[:3].tolist() == [1.5, 2.0, 2.5] and ws.active.tolist() == [1, 0, 1, 1]
    for c in range(1, 3):
        ws.append(c, rebuild=True)
    ws.solve(3)
    st = ws.read()
    assert int(st["accepted"]) == 1 and ws.x[:3].tolist() == [2.0, 3.0, 4.0]


def test_a_new_column_whose_solution_is_exactly_zero_leaves(hip):
    """x = 0 and s = 0 for the column just appended (a sum that cancels exactly, as happens in the fill phase of an exact fit):
    the host's quotient x / (x - s) would be 0 / 0; the column reaches 0 at once and leaves, the others stay as they are."""
    A = np.eye(4)[:, :2]
    ws = workspace(A, np.array([2.0, 0.0, 1.0, 0.0]), 2)
    ws.order.copy_(torch.tensor([0, 1], dtype=torch.int32))
    ws.append(0, rebuild=True)
    ws.solve(1)
    st = ws.read()
    assert int(st["accepted"]) == 1 and ws.x.tolist() == [2.0, 0.0]
    ws.append(1, rebuild=True)
    assert ws.z.tolist() == [2.0, 0.0]
    ws.solve(2)
    st = ws.read()
    assert int(st["accepted"]) == 0 and int(st["count"]) == 1 and int(st["p0"]) == 1 and ws.x[:1].tolist() == [2.0]
    assert ws.active.tolist() == [1, 0]


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_built_on_the_device_the_sampling_runs_the_loop_as_the_hosts_does(hip, proj):
    from burgers_hip import pod, rom
    N, r, dt, _, stride, tau, _ = CASES["n96"]
    X, Phi = pod_basis(N, dt, r)
    runs = training_runs(N, dt)
    dev = pod.build_row_sampling(X, Phi, runs, dt, proj, tau=tau, stride=stride, solver="device")
    host = system("n96", proj.lower())[5]
    assert isinstance(dev, pod.RowSampling) and np.array_equal(dev.rows.numpy(), host.rows.numpy())
    assert dev.projection == host.projection and dev.pairs == host.pairs and dev.tau == host.tau
    mu1, mu2 = draw(4)
    a = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, 12, Phi, dev, rom.PROJ[proj.lower()])
    b = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, 12, Phi, host, rom.PROJ[proj.lower()])
    torch.cuda.synchronize()
    assert not bool(a.flags.any()) and torch.equal(a.iters, b.iters) and int(a.iters.sum()) > 0
