"""Every device-side ROM time loop (the 19 entries of rom._ROUTES) from per-sample, non-constant, out-of-span initial states,
against the reference its own test file uses, called with the same u0.  Every other test of these loops starts from
u0 = ones for all samples, where a read of u0 at the wrong node or of another sample's u0, a start from the projection of
u0, and every term of the first assembly that multiplies u_x cannot be seen.

The starts: loop_cases.initial_states -- sample b is a stored FOM state of another training run than its own parameters,
with a moving front, times 1 + 1e-3 sin((5 + 3 b) pi x / 100).  B = 6 (one full group of four and a ragged one on the
quadratic routes), mu = draw(6), nT = 4 (the local loops: 12, so that every sample switches cluster after its start).
Shapes: the perturbed meshes with diffusion of the routes' own files where the route takes them, 513 nodes for the loops
of 513 .. 1024 nodes, rows 10, 50, 51, 70 (and the last but one) left out on the hyper routes so that sampled index != mesh
row; the wide POD routes at r = 41 and at one width of their files (96 once, on bg_rom_run_wide).  bg_rbf_rom_run_long
runs a closure fitted to its mesh (fitted_closure): the fixture closure carried to more than 512 nodes misses condition 2.

Conditions on the references, asserted in ``reference`` on the reference's own output (CPU) before anything is compared
(measured: the extreme over the samples, projections and cases of a family):
  1. |u0 - Phi Phi^T u0| / |u0| >= 1e-4 for the basis the case projects on (the closures: U_p; the local loops: every
     cluster's basis).  Smallest: POD 1.3e-4, quadratic 3.7e-2, POD-ANN 6.5e-2, POD-RBF 4.6e-2, local 3.5e-3.
  2. every step converges below the cap.  Most iterations: POD 8 (20), quadratic 10 (25), POD-ANN 11 (50), POD-RBF 27 in
     step 1 and 12 afterwards (30), local 7 (20).
  3. the counts at tol * 1.001 and tol / 1.001 are those at tol: no stopping decision sits on the edge.  Where a sample
     missed 2 or 3 at loop_cases.STEP its step is moved (``moved``, next to the case); four more are moved for the
     conditions of tests/test_rom_controls_gpu.py, which runs these cases off the default tol and cap.
  4. the local loops start in a cluster other than 0, not the same for all samples, with a tie margin >= 1e-8.  First
     clusters 2, 5, 6, 4, 5, 9 on 96 nodes and 2, 5, 6, 4, 4, 9 on 513; smallest margin of any pick 1.1e-3.
  5. steps 1 .. nT of the reference move by at least 10 gates when u0 is shifted by one node, replaced by the next
     sample's, or replaced by the route's own decode of its projected coordinates.  Smallest rel-L2 moves
     (shift / next sample / projected), oracle and then restatement:
       POD        2.3e-3 / 0.19 / 1.2e-5      2.3e-3 / 0.20 / 3.4e-5
       quadratic  2.6e-2 / 0.19 / 1.1e-2      0.11 / 0.20 / 1.1e-2
       POD-ANN    5.5e-2 / 0.18 / 4.7e-2      4.8e-2 / 0.18 / 6.7e-2
       POD-RBF    2.3e-2 / 0.18 / 2.4e-5      5.8e-2 / 0.18 / 1.2e-2
       local      1.2e-2 / 4.4e-2 / 7.6e-5    0.13 / 0.19 / 1.1e-3
     At u0 = ones the first two are exactly 0.

Gates: the fp64 loops against the oracle loop_cases.TOL = 1e-10 with equal iteration counts (the local loops: equal cluster
sequences too), against the restatements (sampled rows) max(TOL, 10 d), d the restatement's spread between summing the rows
forwards and backwards (at most 2.4e-14 here, so TOL); the POD-ANN loops TOL32 = 5e-6 with counts within 1.  No flag, info
0, hist[:, 0] is u0 bitwise; on the hyper routes q[:, 0] is Phi^T u0 to 1e-14.  Worst rel-L2 measured on the MI355X,
against the oracle / the restatement: POD 2.2e-15 / 8.0e-16, quadratic 5.5e-14 / 9.4e-15, POD-RBF 4.9e-14 / 5.7e-14,
local 1.2e-15 / 5.4e-16 (gate 1e-10); POD-ANN 5.0e-8 / 4.7e-8 (gate 5e-6).  No route missed its gate."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ann_wide_cases as aw
import hyper_ann_ref as har
import hyper_local_ref as hl
import hyper_quad_ref as hq
import hyper_rbf_ref as hrr
import rbf_long_cases as rc
from conftest import load_golden, rel_l2
from hyper_ref import hyper_prom
from loop_cases import STEP, TOL, check_pod_vs_oracle, draw, initial_states, pod_basis, to_np, training_snapshots

pytestmark = pytest.mark.gpu
B, NT, NT_LOCAL = 6, 4, 12
MU1, MU2 = draw(B)
PERTURBED = (96, 0.2, 0.01, 7)                  # N, dt, E, mesh seed of test_rom_hyper_gpu.FULL["perturbed"]
PERTURBED_WIDE = (160, 0.2, 0.01, 7)            # ... of test_rom_hyper_wide_gpu.FULL["perturbed"]
LEFT_OUT = [10, 50, 51, 70]                     # rows left out of a 96-node mesh: sampled index != mesh row from row 11 on
LOCAL_STEPS = [9, 17, 26, 13, 22, 30]           # the local loops' starts: inside the 40 steps the centres come from


def shifted(u):
    """u moved by one node, node 0 kept."""
    v = np.roll(u, 1)
    v[0] = u[0]
    return v


def unit_sampling(rows, proj):
    from burgers_hip import pod
    return pod.RowSampling(np.asarray(rows, dtype=np.int32), np.ones(len(rows)), proj.lower(), 0.0, 0, 0.0)


def _p(proj):
    from burgers_hip import rom
    return rom.PROJ[proj.lower()]


def controls(tol, max_it, f=1.0, names=("tol", "max_it")):
    """The stopping controls as keyword arguments under the spelling ``names`` of a reference or runner: the tolerance in
    force (None: 1e-6) times ``f``, and the cap only where one is given (None: the callee's own default)."""
    kw = {names[0]: (1e-6 if tol is None else tol) * f}
    if max_it is not None:
        kw[names[1]] = max_it
    return kw


NEWTON = ("newton_tol", "newton_itmax")         # the quadratic manifold's spelling of tol and max_it
RBF = ("tol_newton", "max_newton")              # POD-RBF's


def _mu(mu):
    return (MU1, MU2) if mu is None else mu


# ---- the cases: what the reference and the loop of one route are run on ------------------------------------------------------------
# A case is a SimpleNamespace: entry, family, X, u0 (B, N), nT, cap, gate, rows (None: all, the oracle), span (the bases of
# condition 1), ref(proj, b, start, f, backwards, tol, max_it) -> (U (N, nT+1), iters, extra), projected(proj, b, start),
# launch(proj, u0, tol, max_it, mu, balance) -> res, facade(proj, u0, tol, max_it) -> res of the family's routing front end,
# q0(start) -> what q[:, 0] must be (hyper routes).  tol and max_it (None: 1e-6 and the family's default cap) go to the
# reference and to the runner under its own spelling (``controls``); mu = (mu1, mu2) replaces the draw in a launch and
# ``balance`` is the runner's (tests/test_rom_controls_gpu.py).
def pod_case(entry, shape, r, run, left_out=None, Phi=None, steps=STEP):
    from oracle import burgers_ref as br
    N, dt, E, seed = shape
    X, P = pod_basis(N, dt, r, E=E, seed=seed)
    if Phi is not None:
        P = Phi
    rows = None if left_out is None else np.setdiff1d(np.arange(N), left_out)

    def ref(proj, b, start, f=1.0, backwards=False, tol=None, max_it=None):
        kw = controls(tol, max_it, f)
        if rows is None:
            U, it = br.pod_prom_burgers(X, dt, NT, start, MU1[b], E, MU2[b], P, projection=proj, return_iters=True, **kw)
            return U, it, {}
        Q, it = hyper_prom(X, dt, NT, start, MU1[b], E, MU2[b], P, proj, rows, np.ones(len(rows)), backwards=backwards, **kw)
        U = P @ Q
        U[:, 0] = start
        return U, it, {"Q": Q}

    def launch(proj, u0, tol=None, max_it=None, mu=None, balance=True):
        from burgers_hip import rom
        kw = controls(tol, max_it)
        if rows is None:
            return getattr(rom, run)(X, u0, *_mu(mu), dt, NT, P, _p(proj), E=E, balance=balance, **kw)
        return rom.pod_prom_run_hyper(X, u0, *_mu(mu), dt, NT, P, unit_sampling(rows, proj), _p(proj), E=E, balance=balance, **kw)

    def facade(proj, u0, tol=None, max_it=None):
        from burgers_hip import rom
        return rom.pod_prom_run(X, u0, MU1, MU2, dt, NT, P, projection=proj, E=E, fused=True, **controls(tol, max_it))

    return SimpleNamespace(entry=entry, family="POD", X=X, dt=dt, E=E, Phi=P, u0=initial_states(N, dt, E, seed, B, steps), nT=NT, cap=20, gate=TOL,
                           rows=rows, span=[P], ref=ref, projected=lambda proj, b, u: P @ (P.T @ u), launch=launch, facade=facade,
                           q0=lambda u: P.T @ u)


def quad_case(entry, case, run, left_out=None, steps=STEP):
    from oracle import burgers_ref as br
    N, dt, n, E, seed = hq._case(case)
    X, Phi, H = hq.case_data(case)
    rows = None if left_out is None else np.setdiff1d(np.arange(N), left_out)

    def ref(proj, b, start, f=1.0, backwards=False, tol=None, max_it=None):
        if rows is None:
            U, it = br.pod_quadratic_manifold(X, dt, NT, start, MU1[b], E, MU2[b], Phi, H, projection=proj, return_iters=True,
                                              **controls(tol, max_it, f, NEWTON))
            return U, it, {}
        Q, it = hq.hyper_quad_prom(X, dt, NT, start, MU1[b], E, MU2[b], Phi, H, proj, rows, np.ones(len(rows)), backwards=backwards,
                                   **controls(tol, max_it, f))
        return hq.decode(Phi, H, Q, start), it, {"Q": Q}

    def projected(proj, b, u):
        q = Phi.T @ u
        return Phi @ q + H @ br.get_sym(q)

    def launch(proj, u0, tol=None, max_it=None, mu=None, balance=True):
        from burgers_hip import rom
        kw = controls(tol, max_it, names=NEWTON)
        if run == "fused":
            plan = rom.QuadFusedPlan(Phi, H, torch.device("cuda", torch.cuda.current_device()))
            return rom.quadratic_run_fused(X, u0, *_mu(mu), dt, NT, plan, _p(proj), E=E, balance=balance, **kw)
        if run == "long":
            return rom.quadratic_run_long(X, u0, *_mu(mu), dt, NT, (Phi, H), _p(proj), E=E, balance=balance, **kw)
        return rom.quadratic_run_hyper(X, u0, *_mu(mu), dt, NT, Phi, H, unit_sampling(rows, proj), _p(proj), E=E, balance=balance, **kw)

    def facade(proj, u0, tol=None, max_it=None):
        from burgers_hip import rom
        return rom.quadratic_run(X, u0, MU1, MU2, dt, NT, Phi, H, projection=proj, E=E, long_mesh=True, **controls(tol, max_it, names=NEWTON))

    return SimpleNamespace(entry=entry, family="quadratic", X=X, u0=initial_states(N, dt, E, seed, B, steps), nT=NT, cap=hq.CAP, gate=TOL,
                           rows=rows, span=[Phi], ref=ref, projected=projected, launch=launch, facade=facade, q0=lambda u: Phi.T @ u)


ANN_WIDE = (96, 0.05, 12, 40, (64,), 112, 3.0, 0.01, 7)         # perturbed-96 with 12 primary modes: beyond bg_ann_rom_run's 8


def ann_case(entry, case, run, left_out=None, steps=STEP):
    from oracle import burgers_ref as br
    N, dt, n, nbar, _, _, _, E, seed = har.CASES[case] if isinstance(case, str) else case
    X, Up, Us, model = har.case_data(case)
    Ws, bs = aw.weights(model)
    rows = None if left_out is None else np.setdiff1d(np.arange(N), left_out)

    def ref(proj, b, start, f=1.0, backwards=False, tol=None, max_it=None):
        kw = controls(tol, max_it, f)
        if rows is None:
            U, it = br.pod_ann_prom(X, dt, NT, start, MU1[b], E, MU2[b], Up, Us, Ws, bs, projection=proj, return_iters=True, **kw)
            return U, it, {}
        Q, Qs, it = har.hyper_ann_prom(X, dt, NT, start, MU1[b], E, MU2[b], Up, Us, Ws, bs, proj, rows, np.ones(len(rows)),
                                       backwards=backwards, **kw)
        return har.decode(Up, Us, Q, Qs, start), it, {"Q": Q}

    def projected(proj, b, u):
        q = Up.T @ u
        return Up @ q + Us @ br.mlp_forward(Ws, bs, q.astype(np.float32)).astype(np.float64)

    def launch(proj, u0, tol=None, max_it=None, mu=None, balance=True):
        from burgers_hip import rom
        kw = controls(tol, max_it)
        if rows is None:
            return getattr(rom, run)(X, u0, *_mu(mu), dt, NT, Up, Us, model, _p(proj), E=E, balance=balance, **kw)
        return rom.pod_ann_run_hyper(X, u0, *_mu(mu), dt, NT, Up, Us, model, unit_sampling(rows, proj), _p(proj), E=E, balance=balance, **kw)

    def facade(proj, u0, tol=None, max_it=None):
        from burgers_hip import rom
        return rom.pod_ann_run(X, u0, MU1, MU2, dt, NT, Up, Us, model, projection=proj, E=E, wide=True, **controls(tol, max_it))

    return SimpleNamespace(entry=entry, family="POD-ANN", X=X, u0=initial_states(N, dt, E, seed, B, steps), nT=NT, cap=50, gate=aw.TOL32,
                           rows=rows, span=[Up], ref=ref, projected=projected, launch=launch, facade=facade, q0=lambda u: Up.T @ u)


@functools.lru_cache(maxsize=None)
def fitted_closure(N, dt, kernel, eps=1.0):
    """The nine closure arguments of a closure fitted to the N-node mesh in numpy, by the recipe of hyper_rbf_ref.long_data:
    U_p, U_s the singular vectors 0 .. 16 and 17 .. 95 of the training snapshots, the centres every 6th snapshot in reduced
    coordinates scaled to [-1, 1], W = solve(K + 1e-8 I, Ys).  (From a FOM state the fixture closure interpolated to a mesh
    of more than 512 nodes reaches the cap of 30 in the first step of most samples, at 513, 600 and 1024 nodes alike.)"""
    X, S, U = training_snapshots(N, dt, 0.0, None)
    Up, Us = np.ascontiguousarray(U[:, :17]), np.ascontiguousarray(U[:, 17:96])
    Sc = S[:, ::6]
    Qp, Qs = (Up.T @ Sc).T, (Us.T @ Sc).T
    x_min, x_max, y_min, y_max = Qp.min(0), Qp.max(0), Qs.min(0), Qs.max(0)
    scale = lambda A, lo, hi: 2.0 * ((A - lo) / np.where(hi - lo < 1e-15, 1.0, hi - lo)) - 1.0
    Xt, Ys = scale(Qp, x_min, x_max), scale(Qs, y_min, y_max)
    r2 = ((Xt[:, None, :] - Xt[None]) ** 2).sum(-1)
    K = np.exp(-eps ** 2 * r2) if kernel == "gaussian" else 1.0 / np.sqrt(1.0 + eps ** 2 * r2)
    W = np.linalg.solve(K + 1e-8 * np.eye(len(K)), Ys)
    return Up, Us, Xt, W, eps, x_min, x_max, y_min, y_max


def rbf_case(entry, shape, kernel, run, left_out=None, steps=STEP, fitted=False):
    from oracle import burgers_ref as br
    N, dt, E, seed = shape
    X = training_snapshots(N, dt, E, seed)[0]
    cl = fitted_closure(N, dt, kernel) if fitted else rc.closure(N, kernel)
    Up, Us = cl[0], cl[1]
    rows = None if left_out is None else np.setdiff1d(np.arange(N), left_out)

    def ref(proj, b, start, f=1.0, backwards=False, tol=None, max_it=None):
        if rows is None:
            U, it = br.pod_rbf_prom(X, dt, NT, start, MU1[b], E, MU2[b], *cl, projection=proj, kernel=kernel, return_iters=True,
                                    **controls(tol, max_it, f, RBF))
            return U, it, {}
        Q, Qs, it = hrr.hyper_rbf_prom(X, dt, NT, start, MU1[b], E, MU2[b], *cl, proj, kernel, rows, np.ones(len(rows)),
                                       backwards=backwards, **controls(tol, max_it, f))
        return hrr.decode(Up, Us, Q, Qs, start), it, {"Q": Q}

    def projected(proj, b, u):
        q = Up.T @ u
        return Up @ q + Us @ br.rbf_value(q, cl[2], cl[3], cl[4], kernel, *cl[5:])

    def launch(proj, u0, tol=None, max_it=None, mu=None, balance=True):
        from burgers_hip import rom
        kw = controls(tol, max_it, names=RBF)
        if rows is None:
            return getattr(rom, run)(X, u0, *_mu(mu), dt, NT, *cl, projection=proj, kernel=kernel, E=E, balance=balance, **kw)
        return rom.pod_rbf_run_hyper(X, u0, *_mu(mu), dt, NT, *cl, unit_sampling(rows, proj), _p(proj), kernel=kernel, E=E, balance=balance, **kw)

    def facade(proj, u0, tol=None, max_it=None):
        from burgers_hip import rom
        return rom.pod_rbf_run(X, u0, MU1, MU2, dt, NT, *cl, projection=proj, kernel=kernel, E=E, fused=True, long_mesh=True,
                               **controls(tol, max_it, names=RBF))

    return SimpleNamespace(entry=entry, family="POD-RBF", X=X, u0=initial_states(N, dt, E, seed, B, steps), nT=NT, cap=30, gate=TOL,
                           rows=rows, span=[Up], ref=ref, projected=projected, launch=launch, facade=facade, q0=lambda u: Up.T @ u)


def local_case(entry, shape, run, left_out=None, steps=LOCAL_STEPS):
    from oracle import burgers_ref as br
    N, dt, E, seed = shape
    X, centres, bases, Ug = hl.dense_clustering(N, dt, E, seed)
    rows = None if left_out is None else np.setdiff1d(np.arange(N), left_out)

    def first_pick(u):
        """(cluster, relative gap to the second-best squared centre distance) of the pick from u."""
        d2 = ((centres - (Ug[:, :hl.MG].T @ u)[None, :]) ** 2).sum(1)
        two = np.sort(d2)[:2]
        return int(np.argmin(d2)), float((two[1] - two[0]) / two[1])

    def ref(proj, b, start, f=1.0, backwards=False, tol=None, max_it=None):
        kw = controls(tol, max_it, f)
        if rows is None:
            U, it, cl = br.local_prom_burgers(X, dt, NT_LOCAL, start, MU1[b], E, MU2[b], centres, bases, Ug, hl.MG, projection=proj,
                                              return_iters=True, **kw)
            return U, it, {"clusters": cl, "margin": first_pick(start)[1]}
        U, Q, it, cl, margin = hl.hyper_local_prom(X, dt, NT_LOCAL, start, MU1[b], E, MU2[b], centres, bases, Ug, hl.MG, proj, rows,
                                                   np.ones(len(rows)), backwards=backwards, **kw)
        return U, it, {"Q": Q, "clusters": cl, "margin": margin}

    def projected(proj, b, u):
        P = bases[first_pick(u)[0]]
        return P @ (P.T @ u)

    def launch(proj, u0, tol=None, max_it=None, mu=None, balance=True):
        from burgers_hip import rom
        kw = controls(tol, max_it)
        if rows is None:
            return getattr(rom, run)(X, u0, *_mu(mu), dt, NT_LOCAL, centres, bases, Ug, hl.MG, projection=proj, E=E, balance=balance, **kw)
        return rom.local_prom_run_hyper(X, u0, *_mu(mu), dt, NT_LOCAL, centres, bases, Ug, hl.MG, unit_sampling(rows, proj), _p(proj), E=E,
                                        balance=balance, **kw)

    def facade(proj, u0, tol=None, max_it=None):
        from burgers_hip import rom
        return rom.local_prom_run(X, u0, MU1, MU2, dt, NT_LOCAL, centres, bases, Ug, hl.MG, projection=proj, E=E, fused=True, long_mesh=True,
                                  **controls(tol, max_it))

    return SimpleNamespace(entry=entry, family="local", X=X, u0=initial_states(N, dt, E, seed, B, steps), nT=NT_LOCAL, cap=20,
                           gate=TOL, rows=rows, span=list(bases.values()), ref=ref, projected=projected, launch=launch, facade=facade,
                           bases=bases, q0=None)


def moved(steps):
    """STEP with the steps of some samples moved: where a reference of that case misses condition 2 or 3 at STEP (given next to
    the case), the sample starts from another step of the same training run."""
    return [steps.get(b, s) for b, s in enumerate(STEP)]


LOCAL_96 = (96, 0.07, 0.01, 3)                  # test_rom_hyper_local_gpu.FULL["perturbed"]
RBF_96 = (96, 0.05, 0.01, 7)                    # hyper_rbf_ref.CASES["perturbed-96"]
CASES = {
    # the POD family: pod_prom_burgers, and tests/hyper_ref.py on sampled rows
    "bg_rom_run": lambda: pod_case("bg_rom_run", PERTURBED, 17, "pod_prom_run_fused"),
    "bg_rom_run_wide-41": lambda: pod_case("bg_rom_run_wide", PERTURBED_WIDE, 41, "pod_prom_run_wide"),
    "bg_rom_run_wide-96": lambda: pod_case("bg_rom_run_wide", (512, 0.05, 0.0, None), 96, "pod_prom_run_wide",
                                           Phi=load_golden("committed_pod_r96.npz")["Phi"]),
    "bg_rom_run_blocked-120": lambda: pod_case("bg_rom_run_blocked", (200, 0.05, 0.01, 7), 120, "pod_prom_run_blocked"),
    "bg_rom_run_long": lambda: pod_case("bg_rom_run_long", (513, 0.05, 0.0, None), 17, "pod_prom_run_long"),
    "bg_rom_run_long_wide-41": lambda: pod_case("bg_rom_run_long_wide", (513, 0.05, 0.0, None), 41, "pod_prom_run_long_wide"),
    "bg_rom_run_long_wide-77": lambda: pod_case("bg_rom_run_long_wide", (513, 0.05, 0.0, None), 77, "pod_prom_run_long_wide"),
    "bg_hyper_rom_run": lambda: pod_case("bg_hyper_rom_run", PERTURBED, 17, None, left_out=LEFT_OUT),
    "bg_hyper_rom_run_wide-41": lambda: pod_case("bg_hyper_rom_run_wide", PERTURBED_WIDE, 41, None, left_out=LEFT_OUT + [158]),
    # sample 2 at step 70: at tol = 1e-9 a Galerkin count sits within 1.001 of the edge (test_rom_controls_gpu.py, condition 2)
    "bg_hyper_rom_run_wide-64": lambda: pod_case("bg_hyper_rom_run_wide", (200, 0.08, 0.0, None), 64, None, left_out=LEFT_OUT + [198],
                                                 steps=moved({2: 72})),
    # the quadratic manifold: pod_quadratic_manifold, and tests/hyper_quad_ref.py
    "bg_quad_rom_run": lambda: quad_case("bg_quad_rom_run", "perturbed-96", "fused"),
    "bg_quad_rom_run_long": lambda: quad_case("bg_quad_rom_run_long", (513, 0.05, 21, 0.0, None), "long"),
    "bg_hyper_quad_rom_run": lambda: quad_case("bg_hyper_quad_rom_run", "perturbed-96", "hyper", left_out=LEFT_OUT, steps=moved({3: 98})),
    # POD-ANN: pod_ann_prom, and tests/hyper_ann_ref.py
    # sample 5 at step 145 (both loops on perturbed-96): the LSPG run capped at two iterations amplifies a 1e-6 perturbation of
    # u0 by 130 (bg_hyper_ann_rom_run: 3200), the others by less than 1 (test_rom_controls_gpu.py, condition 3)
    "bg_ann_rom_run": lambda: ann_case("bg_ann_rom_run", "perturbed-96", "pod_ann_run_fused", steps=moved({5: 150})),
    "bg_ann_rom_run_wide": lambda: ann_case("bg_ann_rom_run_wide", ANN_WIDE, "pod_ann_run_wide", steps=moved({3: 98})),
    "bg_hyper_ann_rom_run": lambda: ann_case("bg_hyper_ann_rom_run", "perturbed-96", None, left_out=LEFT_OUT,
                                                 steps=moved({0: 25, 4: 125, 5: 150})),
    # POD-RBF, both kernels: pod_rbf_prom, and tests/hyper_rbf_ref.py
    "bg_rbf_rom_run-gaussian": lambda: rbf_case("bg_rbf_rom_run", RBF_96, "gaussian", "pod_rbf_run_fused", steps=moved({3: 90})),
    "bg_rbf_rom_run-imq": lambda: rbf_case("bg_rbf_rom_run", RBF_96, "imq", "pod_rbf_run_fused"),
    "bg_rbf_rom_run_long-gaussian": lambda: rbf_case("bg_rbf_rom_run_long", (513, 0.05, 0.0, None), "gaussian", "pod_rbf_run_long", fitted=True),
    # sample 1: 52, not the 50 that cleared this file's conditions: at 50 an LSPG count at tol = 1e-9 sits on the edge
    # (test_rom_controls_gpu.py, condition 2)
    "bg_rbf_rom_run_long-imq": lambda: rbf_case("bg_rbf_rom_run_long", (513, 0.05, 0.0, None), "imq", "pod_rbf_run_long", fitted=True,
                                                steps=moved({1: 52})),
    "bg_hyper_rbf_rom_run-gaussian": lambda: rbf_case("bg_hyper_rbf_rom_run", RBF_96, "gaussian", None, left_out=LEFT_OUT,
                                                      steps=moved({3: 90, 5: 150})),
    "bg_hyper_rbf_rom_run-imq": lambda: rbf_case("bg_hyper_rbf_rom_run", RBF_96, "imq", None, left_out=LEFT_OUT),
    # local POD: local_prom_burgers, and tests/hyper_local_ref.py
    "bg_local_rom_run": lambda: local_case("bg_local_rom_run", LOCAL_96, "local_prom_run_fused"),
    "bg_local_rom_run_long": lambda: local_case("bg_local_rom_run_long", (513, 0.05, 0.0, None), "local_prom_run_long"),
    "bg_hyper_local_rom_run": lambda: local_case("bg_hyper_local_rom_run", LOCAL_96, None, left_out=LEFT_OUT),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---- the reference's side: its runs from u0, with the conditions under which the comparison means something -------------------------
@functools.lru_cache(maxsize=None)
def reference(name, proj):
    """[(U, iters, extra, gate)] of the B samples.  Everything asserted here is asserted of the reference's own output."""
    c = case(name)
    out, first = [], []
    for b in range(B):
        u = c.u0[b]
        span = min(np.linalg.norm(u - P @ (P.T @ u)) / np.linalg.norm(u) for P in c.span)
        assert span >= 1e-4, (name, b, span)                                                       # 1: out of span
        U, it, extra = c.ref(proj, b, u)
        assert it.max() < c.cap, (name, proj, b, it.tolist())                                      # 2: below the cap in every step
        for f in (1.001, 1.0 / 1.001):
            assert np.array_equal(c.ref(proj, b, u, f)[1], it), (name, proj, b, f)                 # 3: no decision on the edge
        gate, d = c.gate, 0.0
        if c.rows is not None and c.family != "POD-ANN":                                           # (float32-limited: its gate is fixed)
            Ub, itb, _ = c.ref(proj, b, u, backwards=True)
            assert itb.max() < c.cap
            d = rel_l2(Ub[:, 1:], U[:, 1:])
            gate = max(c.gate, 10.0 * d)
        if c.family == "local":
            first.append(int(extra["clusters"][0]))
            assert first[-1] != 0 and extra["margin"] >= 1e-8, (name, proj, b, first, extra["margin"])      # 4
        moves = [rel_l2(c.ref(proj, b, v)[0][:, 1:], U[:, 1:]) for v in (shifted(u), c.u0[(b + 1) % B], c.projected(proj, b, u))]
        print(f"{name} {proj} sample {b}: out of span {span:.1e}, iterations {it.tolist()}, spread {d:.1e}, moves under a shift "
              f"{moves[0]:.1e}, the next sample's u0 {moves[1]:.1e}, the projected u0 {moves[2]:.1e}"
              + (f", first cluster {first[-1]}, tie margin {extra['margin']:.1e}" if first else ""))
        assert min(moves) >= 10.0 * gate, (name, proj, b, moves, gate)                             # 5: the test would notice
        out.append((U, it, extra, gate))
    if first:
        assert len(set(first)) > 1, first                                                          # 4: not the same for all samples
    return out


# ---- the loops --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_route_from_its_own_initial_states(hip, name, proj):
    c = case(name)
    refs = reference(name, proj)
    res = c.launch(proj, c.u0)
    torch.cuda.synchronize()
    assert res is not None and res.path == c.entry
    hist, iters = to_np(res.hist), to_np(res.iters)
    assert not bool(res.flags.any()) and bool((res.info == 0).all())
    assert np.array_equal(hist[:, 0], c.u0)                                                        # column 0 is u0, bit for bit
    if getattr(res, "redone", 0):
        print(f"{name} {proj}: {res.redone} samples redone on the host side")
    for b, (U, it, extra, gate) in enumerate(refs):
        err = rel_l2(hist[b].T[:, 1:], U[:, 1:]) if c.rows is not None else rel_l2(hist[b].T, U)
        print(f"{name} {proj} sample {b}: rel-L2 {err:.2e} (gate {gate:.1e}), iterations {iters[b].tolist()} / {it.tolist()}")
        assert err < gate, (name, proj, b, err, gate)
        if c.family == "POD-ANN":
            assert np.abs(iters[b] - it).max() <= 1, (name, proj, b)
        else:
            assert np.array_equal(iters[b], it), (name, proj, b)
        if c.family == "local":
            assert np.array_equal(to_np(res.clusters[b]), extra["clusters"]), (name, proj, b)
        if c.rows is not None:
            q = to_np(res.q[b])
            if c.family == "local":
                P = c.bases[int(extra["clusters"][0])]
                w = P.shape[1]
                assert rel_l2(q[0, :w], P.T @ c.u0[b]) < 1e-14 and not q[0, w:].any()              # entry 0 is Phi_c0^T u0
            else:
                assert rel_l2(q[0], c.q0(c.u0[b])) < 1e-14                                         # row 0 of q is Phi^T u0
                assert rel_l2(q.T, extra["Q"]) < gate
    if c.family == "POD" and c.rows is None:
        check_pod_vs_oracle(res, c.X, c.dt, NT, MU1, MU2, c.Phi, proj, E=c.E, u0=c.u0)                # the shared check, with its u0


# ---- a (N,) start is the same start for every sample -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bg_rom_run", "bg_hyper_rom_run"])
def test_a_shared_start_is_broadcast(hip, name):
    c = case(name)
    one = c.launch("LSPG", c.u0[2])
    tiled = c.launch("LSPG", np.tile(c.u0[2], (B, 1)))
    torch.cuda.synchronize()
    assert one.path == c.entry and bool((one.info == 0).all()) and np.array_equal(to_np(one.hist[:, 0]), np.tile(c.u0[2], (B, 1)))
    for k in ("hist", "iters", "flags", "info") + (("q",) if c.rows is not None else ()):
        assert torch.equal(getattr(one, k), getattr(tiled, k)), k
    assert not torch.equal(one.hist[0, 1:], one.hist[1, 1:])                                       # the samples do differ: by mu


# ---- slot != sample: the raw entry points with a reversed ``order`` ---------------------------------------------------------------
def _outputs(B_, nT, cols, dev):
    return (torch.full((B_, nT + 1, cols), -7.0, dtype=torch.float64, device=dev), torch.zeros((B_, nT), dtype=torch.int32, device=dev),
            torch.full((B_,), -3, dtype=torch.int32, device=dev), torch.zeros((B_,), dtype=torch.int32, device=dev))


def test_reversed_order_with_per_sample_starts_long(hip):
    """bg_rom_run_long: slot k works on sample B - 1 - k.  An ``order`` applied to mu but not to u0 (or the other way round)
    gives another sample's run."""
    from burgers_hip import lib, rom
    c = case("bg_rom_run_long")
    p = rom.PROJ["lspg"]
    ref = c.launch("LSPG", c.u0)
    torch.cuda.synchronize()
    N, dev, plan = len(c.X), ref.hist.device, ref.plan
    u0d, Xd = torch.as_tensor(c.u0, device=dev), torch.as_tensor(c.X, device=dev)
    mu1d, mu2d = torch.as_tensor(MU1, device=dev), torch.as_tensor(MU2, device=dev)
    got = {}
    for tag, order in (("identity", torch.arange(B, dtype=torch.int32, device=dev)),
                       ("reversed", torch.arange(B - 1, -1, -1, dtype=torch.int32, device=dev))):
        hist, iters, flags, info = _outputs(B, NT, N, dev)
        rc_ = lib.load().bg_rom_run_long(N, B, plan.r, NT, p, lib.ptr(Xd), lib.ptr(plan.PhiP), lib.ptr(u0d), lib.ptr(mu1d), lib.ptr(mu2d),
                                         c.dt, c.E, 1e-6, 20, lib.mesh_options(c.X, supg=True), lib.ptr(hist), lib.ptr(iters),
                                         lib.ptr(flags), lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
        assert rc_ == 0
        torch.cuda.synchronize()
        got[tag] = (hist, iters, flags, info)
    for a, b_, r_ in zip(got["identity"], got["reversed"], (ref.hist, ref.iters, ref.flags, ref.info)):
        assert torch.equal(a, b_) and torch.equal(a, r_)


def test_reversed_order_with_per_sample_starts_hyper(hip):
    """bg_hyper_rom_run: the same, where u0 reaches the kernel as q0 = Phi^T u0 and as its values at the stencil nodes."""
    from burgers_hip import lib, rom
    c = case("bg_hyper_rom_run")
    p = rom.PROJ["lspg"]
    ref = c.launch("LSPG", c.u0)
    torch.cuda.synchronize()
    N, dev, plan = len(c.X), ref.q.device, ref.plan
    u0d = torch.as_tensor(c.u0, device=dev)
    q0, u0s = (u0d @ plan.Phi).contiguous(), (u0d[:, plan.stencil] * plan.inside).contiguous()
    mu1d, mu2d = torch.as_tensor(MU1, device=dev), torch.as_tensor(MU2, device=dev)
    got = {}
    for tag, order in (("identity", torch.arange(B, dtype=torch.int32, device=dev)),
                       ("reversed", torch.arange(B - 1, -1, -1, dtype=torch.int32, device=dev))):
        qh, iters, flags, info = _outputs(B, NT, plan.r, dev)
        rc_ = lib.load().bg_hyper_rom_run(N, B, plan.r, plan.m, NT, p, lib.ptr(plan.rows), lib.ptr(plan.xi), lib.ptr(plan.xs),
                                          lib.ptr(plan.PhiS), lib.ptr(q0), lib.ptr(u0s), lib.ptr(mu1d), lib.ptr(mu2d), c.dt, c.E, 1e-6, 20,
                                          lib.mesh_options(c.X, supg=True), lib.ptr(qh), lib.ptr(iters), lib.ptr(flags), lib.ptr(info),
                                          lib.ptr(order), lib.stream_ptr(dev))
        assert rc_ == 0
        torch.cuda.synchronize()
        got[tag] = (qh, iters, flags, info)
    for a, b_, r_ in zip(got["identity"], got["reversed"], (ref.q, ref.iters, ref.flags, ref.info)):
        assert torch.equal(a, b_) and torch.equal(a, r_)
