"""Batched projection-ROM time-steppers (host orchestration over the C ABI).

Each Picard / Gauss-Newton iteration of the whole batch is two HIP launches,
    bg_rom_reduce[_lifted]  (assembly + fp64-MFMA projection, for POD also the lift u = Phi q)
    bg_lu_solve_update      (pivoted r x r solve + reduced-coordinate update + convergence bookkeeping)
plus the family-specific decode / tangent, which are plain dense contractions over the batch
(torch / rocBLAS).  Samples carry an ``active`` flag on the device; converged samples are
skipped by the kernels, so every sample follows exactly the reference's own loop:
  pod_prom_burgers        FEM/fem_burgers.py:709-785
  pod_quadratic_manifold  FEM/fem_burgers.py:1081-1175
  pod_ann_prom            FEM/fem_burgers.py:1177-1251
"""
from __future__ import annotations

import weakref
from dataclasses import dataclass
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn

from . import lib as _lib
from . import pod as _pod
from .fom import FomResult, _as_dev, check_mesh
from .fom import batch_inputs as _batch_inputs

PROJ = {"galerkin": _lib.BG_PROJ_GALERKIN, "lspg": _lib.BG_PROJ_LSPG}
_ACT_KINDS = {type(None): _lib.BG_ACT_NONE, nn.ELU: _lib.BG_ACT_ELU, nn.ReLU: _lib.BG_ACT_RELU, nn.Tanh: _lib.BG_ACT_TANH}
_NOT_AVAILABLE = "Projection method '{}' is not available. Please use 'Galerkin' or 'LSPG'."


def _projection(projection, message, exact=False):
    """The BG_PROJ_* code of ``projection`` or ValueError(``message``); ``exact``: spelt as the reference does (:754-764)."""
    if (projection not in ("Galerkin", "LSPG")) if exact else (projection.lower() not in PROJ):
        raise ValueError(message.format(projection))
    return PROJ[projection.lower()]


class _Route(NamedTuple):
    """One device-side time loop as the host sees it.  ``wg_per_cu``, ``max_n`` and ``max_r`` are ints or the names of the
    library's int() symbols that report them (_limit); the closure and local loops report theirs through ``*_limits``."""
    entry: str
    wg_per_cu: object        # persistent workgroups per compute unit
    max_r: object = None     # widest basis
    min_n: int = 2           # min_n <= N <= max_n: the meshes the entry point covers
    max_n: object = 512
    group: int = 1           # samples per slot of ``order``
    supg: bool = True
    redo: bool = False       # the wrapper redoes BG_INFO_NEEDS_PIVOTING samples on the host


_ROUTES = {r.entry: r for r in (
    _Route("bg_rom_run", 2, "bg_rom_run_max_r"),
    _Route("bg_rom_run_wide", 1, "bg_rom_run_wide_max_r", redo=True),
    _Route("bg_rom_run_blocked", 1, "bg_rom_run_blocked_max_r", min_n=3, redo=True),
    _Route("bg_rom_run_long", "bg_rom_run_long_workgroups_per_cu", "bg_rom_run_long_max_r", 3, "bg_rom_run_long_max_n"),
    _Route("bg_rom_run_long_wide", 1, "bg_rom_run_long_wide_max_r", 3, "bg_rom_run_long_wide_max_n", redo=True),
    _Route("bg_quad_rom_run", 1, "bg_quad_rom_max_n", group=4, supg=False),
    _Route("bg_quad_rom_run_long", "bg_quad_rom_run_long_workgroups_per_cu", "bg_quad_rom_run_long_max_r", 513,
           "bg_quad_rom_run_long_max_n", group=4, supg=False),
    _Route("bg_ann_rom_run", 2), _Route("bg_ann_rom_run_wide", 2), _Route("bg_rbf_rom_run", 2), _Route("bg_local_rom_run", 2),
    _Route("bg_local_rom_run_long", "bg_rom_run_long_workgroups_per_cu"),
    _Route("bg_rbf_rom_run_long", 1, min_n=513, max_n=1024),
    _Route("bg_hyper_rom_run", 2, min_n=3, max_n="bg_fom_max_n"),
    _Route("bg_hyper_rom_run_wide", 1, min_n=3, max_n="bg_fom_max_n", redo=True),
    _Route("bg_hyper_rom_run_blocked", 1, min_n=3, max_n="bg_fom_max_n", redo=True),
    _Route("bg_hyper_ann_rom_run", 2, min_n=3, max_n="bg_fom_max_n"),      # one per CU beyond 512 table nodes (HyperAnnPlan.wg_per_cu)
    _Route("bg_hyper_ann_rom_run_wide", 2, min_n=3, max_n="bg_fom_max_n"), # likewise (HyperAnnWidePlan.wg_per_cu)
    _Route("bg_hyper_rbf_rom_run", 2, min_n=3, max_n="bg_fom_max_n"),      # likewise (HyperRbfPlan.wg_per_cu)
    _Route("bg_hyper_quad_rom_run", 1, "bg_quad_rom_max_n", 3, "bg_fom_max_n", group=4, supg=False),
    _Route("bg_hyper_local_rom_run", 2, min_n=3, max_n="bg_fom_max_n"),
)}


def _limit(v):
    return v if isinstance(v, int) else getattr(_lib.load(), v)()


class SingularReducedSystem(np.linalg.LinAlgError):
    """np.linalg.solve raises LinAlgError('Singular matrix') at the same place (:767)."""


@dataclass
class _Common:
    L: object
    device: torch.device
    X: torch.Tensor
    N: int
    B: int
    mu1: torch.Tensor
    mu2: torch.Tensor
    u0: torch.Tensor
    fdt: torch.Tensor
    hfs: torch.Tensor
    dt: float
    E: float
    mesh_opt: int = 0
    Un: torch.Tensor = None          # state at the start of the time step (library path only)

    def stream(self):
        return _lib.stream_ptr(self.device)


def _setup(X, u0, mu1, mu2, dt, E, device, max_n=None):
    L = _lib.load()
    device = _lib.require_device(device)
    mesh_opt = _lib.mesh_options(check_mesh(X), supg=False)
    Xd = _as_dev(X, device)
    N = Xd.numel()
    max_n = L.bg_fom_max_n() if max_n is None else max_n
    if N > max_n:
        raise NotImplementedError(f"ROM steppers cover N <= {max_n} (got {N})")
    u0d, mu1d, mu2d = _batch_inputs(u0, mu1, mu2, N, device)
    B = mu1d.numel()
    fdt = torch.empty((B, N), dtype=torch.float64, device=device)
    hfs = torch.empty((B, N), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        _lib.check(L.bg_forcing_setup(N, B, _lib.ptr(Xd), _lib.ptr(mu2d), float(dt), mesh_opt, _lib.ptr(fdt),
                                      _lib.ptr(hfs), _lib.stream_ptr(device)), "bg_forcing_setup")
    return _Common(L, device, Xd, N, B, mu1d, mu2d, u0d, fdt, hfs, float(dt), float(E), mesh_opt)


def _mass_rhs(c, Un, out):
    c.Un = Un.clone()
    with torch.cuda.device(c.device):
        _lib.check(c.L.bg_mass_rhs(c.N, c.B, _lib.ptr(c.X), _lib.ptr(Un), _lib.ptr(c.fdt), c.mesh_opt, _lib.ptr(out),
                                   c.stream()), "bg_mass_rhs")
    return out


def rom_reduce(c, W, U, G, proj, supg, active, Ar, br, wtu=None, colmajor=False, w_index=None, extra_opts=0):
    """Ar, br (and optionally W^T u) of every active sample.  W: (N, r) shared or (B, N, r);
    with ``colmajor`` the transposed blocks (r, N) / (B, r, N); with ``w_index`` (B,) int32 a stack
    (C, N, r) of bases of which sample b uses block w_index[b]."""
    r = W.shape[-2] if colmajor else W.shape[-1]
    if r > c.L.bg_rom_max_r() or c.N > c.L.bg_rom_max_n():
        Wl = W if w_index is None else W[w_index.long()]
        return _rom_reduce_library(c, Wl.transpose(-1, -2) if colmajor else Wl, U, proj, supg, active, Ar, br, wtu)
    stride = 0 if W.dim() == 2 else c.N * r
    opts = (1 if supg else 0) | c.mesh_opt | (_lib.BG_OPT_W_COLMAJOR if colmajor else 0) | extra_opts
    if w_index is not None:
        _reduce_call(c, "bg_rom_reduce_indexed", r, proj, (_lib.ptr(W), stride, _lib.ptr(w_index), _lib.ptr(U)), G, opts,
                     active, Ar, br, wtu)
    else:
        _reduce_call(c, "bg_rom_reduce", r, proj, (_lib.ptr(W), stride, _lib.ptr(U)), G, opts, active, Ar, br, wtu,
                     r_limit=True)


def _reduce_call(c, entry, r, proj, mid, G, opts, active, Ar, br, wtu, r_limit=False):
    """One checked call of a bg_rom_reduce* entry point.  ``mid``: what its signature has between x and G (the basis or
    tangent with its stride or index, and u or q).  ``r_limit``: BG_ERR_UNSUPPORTED_R raises the NotImplementedError that
    names the kernels' limit on r."""
    with torch.cuda.device(c.device):
        rc = getattr(c.L, entry)(c.N, c.B, r, proj, _lib.ptr(c.X), *mid, _lib.ptr(G), _lib.ptr(c.hfs), _lib.ptr(c.mu1),
                                 c.dt, c.E, opts, _lib.ptr(active), _lib.ptr(Ar), _lib.ptr(br), _lib.ptr(wtu), c.stream())
    if r_limit and rc == _lib.BG_ERR_UNSUPPORTED_R:
        raise NotImplementedError(f"ROM kernels cover r <= {c.L.bg_rom_max_r()} (got {r})")
    _lib.check(rc, entry)


def _rom_reduce_library(c, W, U, proj, supg, active, Ar, br, wtu):
    """Same outputs as bg_rom_reduce for sizes beyond the register-resident MFMA kernels
    (r > 47 or N > 512): HIP assembly (bg_fom_assemble), then A W, the projection and W^T u as
    library GEMMs over the batch.  Inactive samples keep their previous outputs."""
    from . import fom as _fom
    lo, di, up, rhs = _fom.fom_assemble(c.X.cpu().numpy(), U, c.Un, c.mu1, c.mu2, c.dt, E=c.E, supg=supg,
                                        device=c.device)
    Wb = W if W.dim() == 3 else W.unsqueeze(0)
    z = torch.zeros_like(Wb[:, :1])
    Y = di.unsqueeze(-1) * Wb + lo.unsqueeze(-1) * torch.cat([z, Wb[:, :-1]], 1) + \
        up.unsqueeze(-1) * torch.cat([Wb[:, 1:], z], 1)                                   # A W, (B, N, r)
    L_ = Wb if proj == _lib.BG_PROJ_GALERKIN else Y
    Ar_new = torch.matmul(L_.transpose(1, 2), Y)
    br_new = -torch.matmul(L_.transpose(1, 2), rhs.unsqueeze(-1)).squeeze(-1)             # R = -rhs
    m = torch.ones((c.B,), dtype=torch.bool, device=c.device) if active is None else active.bool()
    Ar.copy_(torch.where(m[:, None, None], Ar_new, Ar))
    br.copy_(torch.where(m[:, None], br_new, br))
    if wtu is not None:
        wtu.copy_(torch.where(m[:, None], torch.matmul(Wb.transpose(1, 2), U.unsqueeze(-1)).squeeze(-1), wtu))


def lu_solve(A, b, sign=1.0, active=None, x=None, info=None):
    """x = solve(A, sign*b) for a batch of (n, n) systems on the device."""
    L = _lib.load()
    device = _lib.require_device(A.device)
    B, n, _ = A.shape
    x = torch.empty((B, n), dtype=torch.float64, device=device) if x is None else x
    info = torch.zeros((B,), dtype=torch.int32, device=device) if info is None else info
    with torch.cuda.device(device):
        rc = L.bg_lu_solve(n, B, _lib.ptr(A), _lib.ptr(b), float(sign), _lib.ptr(active), _lib.ptr(x), _lib.ptr(info),
                           _lib.stream_ptr(device))
    if rc == _lib.BG_ERR_UNSUPPORTED_R:
        raise NotImplementedError("bg_lu_solve covers n <= 64")
    _lib.check(rc, "bg_lu_solve")
    return x, info


def rom_reduce_lifted(c, Phi, q, U, G, proj, supg, active, Ar, br, wtu, extra_opts=0):
    """bg_rom_reduce with u = Phi q formed in-kernel (and stored to U)."""
    _reduce_call(c, "bg_rom_reduce_lifted", Phi.shape[1], proj, (_lib.ptr(Phi), _lib.ptr(q), _lib.ptr(U)), G,
                 (1 if supg else 0) | c.mesh_opt | extra_opts, active, Ar, br, wtu, r_limit=True)


def rom_lift(c, Phi, q, U, active=None):
    with torch.cuda.device(c.device):
        rc = c.L.bg_rom_lift(c.N, c.B, Phi.shape[1], _lib.ptr(c.X), _lib.ptr(Phi), _lib.ptr(q),
                             _lib.ptr(active), _lib.ptr(U), c.stream())
    _lib.check(rc, "bg_rom_lift")


class _IterState:
    """Per-time-step bookkeeping that lives on the device; one 8-byte readback per iteration."""

    def __init__(self, c, n):
        i32 = dict(dtype=torch.int32, device=c.device)
        self.c = c
        self.active = torch.ones((c.B,), **i32)
        self.k = torch.zeros((c.B,), **i32)
        self.flags = torch.zeros((c.B,), **i32)
        self.info = torch.zeros((c.B,), **i32)
        self.counter = torch.zeros((2, _lib.BG_COUNTER_SLOTS * _lib.BG_COUNTER_STRIDE), **i32)   # partial counts: still active | singular
        self.dq = torch.zeros((c.B, n), dtype=torch.float64, device=c.device)

    # Converged samples are skipped ON THE DEVICE (active mask), so the host does not have to
    # look after every batched iteration: it polls after POLL_FIRST iterations of a time step
    # and then every POLL_EVERY; an iteration launched on an all-converged batch is a no-op.
    POLL_FIRST = 4
    POLL_EVERY = 2

    def begin_step(self):
        self.active.fill_(1)
        self.k.zero_()
        self.launched = 0

    def _solve_update_library(self, mode, Ar, br, wtu, q, tol, max_it):
        """bg_lu_solve_update for n > 64: rocSOLVER LU through torch, same update rules."""
        act = self.active.bool()
        dq = _batched_solve(Ar, -br, act)
        qn = (wtu if mode == 1 else q) + dq
        q.copy_(torch.where(act[:, None], qn, q))
        nd, nq = torch.linalg.vector_norm(dq, dim=1), torch.linalg.vector_norm(qn, dim=1)
        self.k += self.active
        if mode == 1:
            err = nd / nq; more = (err > tol) & (self.k < max_it)
        elif mode == 2:
            err = nd / torch.clamp(nq, min=1e-14); more = ~(err < tol) & (self.k < max_it)
        else:
            err = nd / (nq + 1e-14); more = (err > tol) & (self.k < max_it)
        capped = (self.k >= max_it) & (~(err < tol) if mode == 2 else torch.ones_like(more))
        self.flags |= (act & ~torch.isfinite(err)).to(torch.int32) * _lib.BG_FLAG_NONFINITE
        self.flags |= (act & capped).to(torch.int32) * _lib.BG_FLAG_HIT_CAP
        self.active.copy_((act & more).to(torch.int32))
        return int(self.active.sum().item())

    def solve_update(self, mode, Ar, br, wtu, q, tol, max_it):
        """dq = solve(Ar, -br); q, iteration counters and the active mask updated on the device.
        Returns the number of samples that need another iteration (-1: not polled this time)."""
        c = self.c
        self.launched += 1
        self.active_before = self.active.bool()        # samples whose q this call updates
        if q.shape[1] > 64:
            return self._solve_update_library(mode, Ar, br, wtu, q, tol, max_it)
        poll = (self.launched >= max_it or self.launched == self.POLL_FIRST or
                (self.launched > self.POLL_FIRST and (self.launched - self.POLL_FIRST) % self.POLL_EVERY == 0))
        if poll:
            self.counter[0].zero_()         # row 1 (singular systems) keeps accumulating until read
        with torch.cuda.device(c.device):
            rc = c.L.bg_lu_solve_update(q.shape[1], c.B, _lib.ptr(Ar), _lib.ptr(br), mode,
                                        _lib.ptr(wtu), _lib.ptr(q), _lib.ptr(self.dq),
                                        float(tol), int(max_it), _lib.ptr(self.active), _lib.ptr(self.k),
                                        _lib.ptr(self.flags), _lib.ptr(self.counter), _lib.ptr(self.info), c.stream())
        if rc == _lib.BG_ERR_UNSUPPORTED_R:
            raise NotImplementedError("bg_lu_solve covers n <= 64")
        _lib.check(rc, "bg_lu_solve_update")
        if not poll:
            return -1
        n_active, n_singular = self.counter.cpu().sum(1).tolist()      # 4 KB readback, summed on the host
        if n_singular:
            raise SingularReducedSystem("Singular matrix")
        return n_active


def _alloc_hist(c, nsteps):
    hist = torch.empty((c.B, nsteps + 1, c.N), dtype=torch.float64, device=c.device)
    hist[:, 0] = c.u0
    iters = torch.zeros((c.B, nsteps), dtype=torch.int32, device=c.device)
    flags = torch.zeros((c.B,), dtype=torch.int32, device=c.device)
    return hist, iters, flags


def _host_loop(c, nsteps, n, step):
    """The frame of the host-driven loops for ``n`` reduced unknowns; ``step(k, U, st, Ar, br, wtu, G)`` iterates time
    step k from the state U (B, N), with G = M u^n + dt F and all samples active, and returns the new state."""
    hist, iters, flags = _alloc_hist(c, nsteps)
    f64 = dict(dtype=torch.float64, device=c.device)     # the reduced system Ar | br, W^T u and G = M u^n + dt F
    Ar, br, wtu = torch.zeros((c.B, n, n), **f64), torch.zeros((c.B, n), **f64), torch.zeros((c.B, n), **f64)
    G = torch.empty((c.B, c.N), **f64)
    st = _IterState(c, n)
    U = c.u0.clone()
    for k in range(nsteps):
        _mass_rhs(c, U, G)
        st.begin_step()
        U = step(k, U, st, Ar, br, wtu, G)
        iters[:, k] = st.k
        hist[:, k + 1] = U
    flags |= st.flags
    return FomResult(hist, iters, flags, path="host")


# --------------------------------------------------------------------------- POD
def _device_loop(route, Xh, u0, mu1, mu2, nsteps, device, options, balance, launch, keep=(), slots=None, cols=None):
    """What the device-side time loops (_ROUTES) share: the batched inputs, the outputs, the sample order over the grid
    (``slots``, or the route's workgroups per CU on every compute unit; ``route.group`` samples per slot), the launch and its
    FomResult.  ``Xh``: the mesh as check_mesh returned it.  ``launch(f, N, B, x, inputs, opts, outputs)`` calls the C
    entry point ``f`` with its own argument list; ``inputs`` are the pointers u0, mu1, mu2 and ``outputs`` hist, iters,
    flags, info, order, stream.  Nothing is synchronised: ``res.info`` is checked lazily by the caller, and the operands
    live in ``res._keep`` (inputs first, then ``keep``) as long as the result, since the launch is asynchronous.
    ``cols``: the entries per row of ``hist`` where the loop does not write mesh rows (bg_hyper_rom_run: r)."""
    grid = slots if slots is not None else _limit(route.wg_per_cu) * _cu_count(device)
    opts = _lib.mesh_options(Xh, supg=route.supg) | options
    Xd = _as_dev(Xh, device)
    N = Xd.numel()
    u0d, mu1d, mu2d = _batch_inputs(u0, mu1, mu2, N, device)
    B = mu1d.numel()
    hist = torch.empty((B, nsteps + 1, N if cols is None else cols), dtype=torch.float64, device=device)
    iters = torch.zeros((B, nsteps), dtype=torch.int32, device=device)
    flags = torch.zeros((B,), dtype=torch.int32, device=device)
    info = torch.zeros((B,), dtype=torch.int32, device=device)
    order = sample_order(mu1d, grid, route.group) if balance else None
    outputs = (_lib.ptr(hist), _lib.ptr(iters), _lib.ptr(flags), _lib.ptr(info), _lib.ptr(order), _lib.stream_ptr(device))
    with torch.cuda.device(device):
        rc = launch(getattr(_lib.load(), route.entry), N, B, _lib.ptr(Xd), (_lib.ptr(u0d), _lib.ptr(mu1d), _lib.ptr(mu2d)), int(opts), outputs)
    _lib.check(rc, route.entry)
    res = FomResult(hist, iters, flags, path=route.entry)
    res.info = info
    res._keep = (Xd, u0d, mu1d, mu2d) + tuple(keep)
    return res


def pod_prom_run_fused(X, u0, mu1, mu2, dt, nsteps, Phi, proj, E=0.0, tol=1e-6, max_it=20, device=None, options=0, balance=True):
    """``pod_prom_burgers`` for a batch with the whole time loop on the device (bg_rom_run): one workgroup per
    sample, no host in the loop.  Covers N <= 512 and r <= bg_rom_run_max_r()."""
    device = _lib.require_device(device)
    Xh = check_mesh(X)
    Phid = _as_dev(Phi, device)
    if Phid.dim() != 2 or Phid.shape[0] != len(Xh):
        raise ValueError("Phi must have one row per mesh node")
    r = Phid.shape[1]
    return _device_loop(_ROUTES["bg_rom_run"], Xh, u0, mu1, mu2, nsteps, device, options, balance,
                        lambda f, N, B, x, inputs, opts, outputs: f(
                            N, B, r, int(nsteps), proj, x, _lib.ptr(Phid), *inputs, float(dt), float(E), float(tol),
                            int(max_it), opts, *outputs), keep=(Phid,))


def sample_order(mu1d, grid, group=1):
    """The ``order`` argument of the device-side time loops (bg_rom_run, bg_rom_run_wide, bg_quad_rom_run,
    bg_ann_rom_run): which sample each slot of the launch works on.  The samples are independent, so this is a pure
    scheduling decision -- the results are the same bit for bit -- but their cost is not uniform: the iteration count of
    a sample follows its convection parameter mu1 (correlation 0.99 on the bench sweep).  Workgroup k of ``grid``
    persistent workgroups takes the slots k, k + grid, ...; with ``group`` = 4 (bg_quad_rom_run) four consecutive slots
    share a workgroup and every pass lasts until the slowest of the four has converged.  So: sort by mu1, keep
    neighbours together inside a group, and deal the groups out in boustrophedon order (round 0 left to right, round 1
    right to left, ...) so that every workgroup gets the same mix of expensive and cheap ones.  Returns an int32
    device tensor, or None when there is nothing to balance."""
    B = mu1d.numel()
    units = B // group                                   # whole groups; a ragged tail keeps the last slots
    if B <= group or (group == 1 and B <= grid):
        return None
    rank = torch.argsort(mu1d, descending=True)
    u = torch.arange(units, device=mu1d.device)
    rnd, pos = u // grid, u % grid
    size = torch.clamp(units - rnd * grid, max=grid)      # units in this round (the last one may be short)
    slot = rnd * grid + torch.where(rnd % 2 == 0, pos, size - 1 - pos)
    order = torch.empty_like(rank)
    head = units * group
    order[:head].view(units, group)[slot] = rank[:head].view(units, group)
    order[head:] = rank[head:]
    return order.to(torch.int32)


def _cu_count(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def _padded_basis(Phi, N, r, row_multiple, cols):
    """The padded copy of the device basis ``Phi`` the streaming POD loops read: Phi at row offset 1 in a zero matrix of
    (N rounded up to ``row_multiple``) + 2 rows by ``cols`` columns."""
    NPAD = (N + row_multiple - 1) // row_multiple * row_multiple
    PhiP = torch.zeros((NPAD + 2, cols), dtype=torch.float64, device=Phi.device)
    PhiP[1:N + 1, :r] = Phi
    return PhiP


def _redo_marked(res, Xh, plan, dt, nsteps, proj, E, tol, max_it, device):
    """Redo the samples a device loop marked BG_INFO_NEEDS_PIVOTING (np.linalg.solve would have exchanged rows: rare)
    through the library path, LU with partial pivoting.  Reads ``info`` back, so it synchronises the host."""
    _, u0d, mu1d, mu2d = res._keep[:4]
    redo = (res.info == _lib.BG_INFO_NEEDS_PIVOTING).nonzero().squeeze(1)
    if redo.numel():
        rr = _pod_prom_run_library(Xh, u0d[redo], mu1d[redo], mu2d[redo], dt, nsteps, plan.Phi, proj, E, tol, max_it, device)
        res.hist[redo], res.iters[redo], res.flags[redo] = rr.hist, rr.iters, rr.flags
        res.info[redo] = 0
    res.redone = int(redo.numel())


class _PaddedPodPlan:
    """What the streaming POD loops read, built once per basis on the device: the basis and its padded copy PhiP
    (_padded_basis: ``cols(r)`` columns), checked against the entry's own count ``elems(N, r)``.  What the shape alone
    decides is refused before the device is touched; every refusal is a ValueError."""
    slots = work = None           # BlockedPodPlan: its workgroups and their workspace, one slot each

    def __init__(self, route, Phi, device, row_multiple, cols, elems):
        shape = tuple(np.shape(Phi))
        if len(shape) != 2:
            raise ValueError("Phi must be (N, r)")
        N, r = shape
        max_r, max_n = _limit(route.max_r), _limit(route.max_n)
        if r < 1 or r > max_r:
            raise ValueError(f"Phi must be (N, r) with 1 <= r <= {max_r}")
        if N < route.min_n or N > max_n:
            raise ValueError(f"{route.entry} covers {route.min_n} <= N <= {max_n}, not N = {N}")
        device = _lib.require_device(device)
        self.Phi = _as_dev(Phi, device)
        self.N, self.r = N, r
        self.PhiP = _padded_basis(self.Phi, N, r, row_multiple, cols(r))
        if self.PhiP.numel() != elems(N, r):
            raise ValueError(f"{route.entry} does not cover N = {N}, r = {r}")


def _check_plan(plan, Xh, device):
    if plan.N != len(Xh) or plan.Phi.device != device:
        raise ValueError("Phi must have one row per mesh node (and a plan must live on the device of the call)")


def _run_pod_route(route, plan_type, X, u0, mu1, mu2, dt, nsteps, Phi_or_plan, proj, E, tol, max_it, device, options, balance):
    """pod_prom_run_wide, _blocked, _long and _long_wide: the plan (or the basis to build one from), the launch, the redo on the host."""
    device = _lib.require_device(device)
    Xh = check_mesh(X)
    plan = Phi_or_plan if isinstance(Phi_or_plan, plan_type) else plan_type(Phi_or_plan, device)
    _check_plan(plan, Xh, device)
    work = () if plan.slots is None else (_lib.ptr(plan.work), plan.slots)
    res = _device_loop(route, Xh, u0, mu1, mu2, nsteps, device, options, balance,
                       lambda f, N, B, x, inputs, opts, outputs: f(
                           N, B, plan.r, int(nsteps), proj, x, _lib.ptr(plan.PhiP), *inputs, float(dt), float(E),
                           float(tol), int(max_it), opts, *work, *outputs), keep=(plan,), slots=plan.slots)
    if route.redo:
        _redo_marked(res, Xh, plan, dt, nsteps, proj, E, tol, max_it, device)
    res.plan = plan
    return res


class WidePodPlan(_PaddedPodPlan):
    """The operand bg_rom_run_wide reads, built once per basis on the device (include/burgers_hip.h): the padded copy
    PhiP [NPAD + 2][96] of ``Phi`` (row i at index i + 1, zero rows and columns around it), kept together with the basis
    it was built from, which the pivoting redo of pod_prom_run_wide uses."""

    def __init__(self, Phi, device):
        super().__init__(_ROUTES["bg_rom_run_wide"], Phi, device, 64, lambda r: 96,
                         lambda N, r: _lib.load().bg_rom_run_wide_phi_elems(N))


def pod_prom_run_wide(X, u0, mu1, mu2, dt, nsteps, Phi, proj, E=0.0, tol=1e-6, max_it=20, device=None, options=0,
                      balance=True):
    """``pod_prom_burgers`` for bases of 41 .. 96 modes with the whole time loop on the device (bg_rom_run_wide): the basis
    streams through LDS, the reduced system's accumulators are spread over the four waves of the sample's workgroup.
    Samples whose elimination would have needed a row exchange come back marked and are redone through the library
    path (LU with partial pivoting); finding them reads ``info`` back, so unlike the other device-side loops this wrapper
    synchronises the host.  ``Phi``: the basis, or a WidePodPlan of it to reuse across calls (``res.plan``; ``res.PhiP`` is
    its padded copy)."""
    res = _run_pod_route(_ROUTES["bg_rom_run_wide"], WidePodPlan, X, u0, mu1, mu2, dt, nsteps, Phi, proj, E, tol, max_it,
                         device, options, balance)
    res.PhiP = res.plan.PhiP                             # the padded copy the kernel read (what wide results carried before)
    return res


class BlockedPodPlan(_PaddedPodPlan):
    """What bg_rom_run_blocked reads and writes besides the batch, built once per basis on the device
    (include/burgers_hip.h): the padded copy PhiP [NPAD + 2][RP] of ``Phi`` (row i at index i + 1, zero rows and columns
    around it), the workspace of ``slots`` slots (one per workgroup; default: one per compute unit, the kernel's LDS
    admits one workgroup per CU) and the basis itself, which the pivoting redo of pod_prom_run_blocked uses."""

    def __init__(self, Phi, device, slots=None):
        super().__init__(_ROUTES["bg_rom_run_blocked"], Phi, device, 8, lambda r: (r + 15) // 16 * 16,
                         _lib.load().bg_rom_run_blocked_phi_elems)
        self.slots = int(slots) if slots is not None else _cu_count(self.Phi.device)
        if self.slots < 1:
            raise ValueError("slots must be positive")
        self.work = torch.empty((self.slots, _lib.load().bg_rom_run_blocked_work_elems(self.N, self.r)),
                                dtype=torch.float64, device=self.Phi.device)


def pod_prom_run_blocked(X, u0, mu1, mu2, dt, nsteps, Phi_or_plan, proj, E=0.0, tol=1e-6, max_it=20, device=None,
                         options=0, balance=True):
    """``pod_prom_burgers`` for bases of up to 256 modes with the whole time loop on the device (bg_rom_run_blocked): the
    reduced system lives in a per-workgroup workspace slot, projected and eliminated tile by tile on the matrix cores.
    Samples whose elimination would have needed a row exchange come back marked and are redone through the library
    path, as in pod_prom_run_wide (so this wrapper synchronises the host).  ``Phi_or_plan``: the basis, or a
    BlockedPodPlan of it to reuse across calls (``res.plan``)."""
    return _run_pod_route(_ROUTES["bg_rom_run_blocked"], BlockedPodPlan, X, u0, mu1, mu2, dt, nsteps, Phi_or_plan, proj, E,
                          tol, max_it, device, options, balance)


class LongPodPlan(_PaddedPodPlan):
    """The operand bg_rom_run_long reads, built once per basis on the device (include/burgers_hip.h): the padded copy
    PhiP [NPAD + 2][40] of ``Phi`` (row i at index i + 1, NPAD = N rounded up to 64, zero rows and columns around it)."""

    def __init__(self, Phi, device):
        super().__init__(_ROUTES["bg_rom_run_long"], Phi, device, 64, lambda r: 40, _lib.load().bg_rom_run_long_phi_elems)


def pod_prom_run_long(X, u0, mu1, mu2, dt, nsteps, Phi_or_plan, proj, E=0.0, tol=1e-6, max_it=20, device=None, options=0,
                      balance=True):
    """``pod_prom_burgers`` for meshes of up to bg_rom_run_long_max_n() = 1024 nodes and bases of up to 40 modes with the
    whole time loop on the device (bg_rom_run_long): the basis streams through LDS, the pivoting repair runs inside the
    call, nothing is synchronised.  ``Phi_or_plan``: the basis, or a LongPodPlan of it to reuse across calls (``res.plan``)."""
    return _run_pod_route(_ROUTES["bg_rom_run_long"], LongPodPlan, X, u0, mu1, mu2, dt, nsteps, Phi_or_plan, proj, E, tol,
                          max_it, device, options, balance)


class LongWidePodPlan(_PaddedPodPlan):
    """The operand bg_rom_run_long_wide reads, built once per basis on the device (include/burgers_hip.h): the padded copy
    PhiP [NPAD + 2][96] of ``Phi`` (WidePodPlan's layout on a mesh of up to 1024 nodes), kept together with the basis it
    was built from, which the pivoting redo of pod_prom_run_long_wide uses."""

    def __init__(self, Phi, device):
        super().__init__(_ROUTES["bg_rom_run_long_wide"], Phi, device, 64, lambda r: 96,
                         lambda N, r: _lib.load().bg_rom_run_long_wide_phi_elems(N))


def pod_prom_run_long_wide(X, u0, mu1, mu2, dt, nsteps, Phi_or_plan, proj, E=0.0, tol=1e-6, max_it=20, device=None,
                           options=0, balance=True):
    """``pod_prom_burgers`` for meshes of up to bg_rom_run_long_wide_max_n() = 1024 nodes and bases of up to 96 modes with
    the whole time loop on the device (bg_rom_run_long_wide): pod_prom_run_wide's loop and solve on pod_prom_run_long's
    meshes.  Samples whose elimination would have needed a row exchange come back marked and are redone through the
    library path, as in pod_prom_run_wide (so this wrapper synchronises the host).  ``Phi_or_plan``: the basis, or a
    LongWidePodPlan of it to reuse across calls (``res.plan``)."""
    return _run_pod_route(_ROUTES["bg_rom_run_long_wide"], LongWidePodPlan, X, u0, mu1, mu2, dt, nsteps, Phi_or_plan, proj,
                          E, tol, max_it, device, options, balance)


# ------------------------------------------------ the frame of the hyper-reduced loops
# A plan holds what its loop reads besides the batch, built once per operands, sampling and mesh: N, m, Xh, the sampling, its
# projection code, the weights xi, and one of two tables of the sampled rows -- the three-point stencil of every row
# (_put_stencil: the POD and local loops) or the sorted distinct stencil nodes (_put_table: the closure and quadratic loops).
_SAMPLING_PROJECTION = "the row sampling's projection must be 'galerkin' or 'lspg' (got '{}')"
_host64 = _pod._host64


def _sampling_rows(route, sampling, N, max_m):
    """(rows int64, xi float64) of a pod.RowSampling on the host, checked against a mesh of N nodes and the loop's ``max_m``:
    what every hyper plan refuses alike, each a ValueError."""
    rows = np.asarray(sampling.rows.cpu() if isinstance(sampling.rows, torch.Tensor) else sampling.rows).astype(np.int64).reshape(-1)
    xi = _host64(sampling.xi).reshape(-1)
    m = len(rows)
    if m < 1 or m > N or len(xi) != m or rows[0] < 0 or rows[-1] >= N or not np.all(np.diff(rows) > 0):
        raise ValueError("the sampled rows must be ascending, distinct and in [0, N), one weight each")
    if not (np.isfinite(xi).all() and (xi >= 0.0).all()):
        raise ValueError("the weights must be finite and >= 0")
    if m > max_m:
        raise ValueError(f"{route.entry} covers at most {max_m} sampled rows (got {m})")
    return rows, xi


def _stencil_nodes(route, rows, N, max_nodes):
    """The sorted distinct stencil nodes of the sampled rows (ValueError beyond ``max_nodes``)."""
    nodes = np.unique(np.clip(rows[:, None] + np.arange(-1, 2)[None, :], 0, N - 1))
    if len(nodes) > max_nodes:
        raise ValueError(f"{route.entry} covers at most {max_nodes} stencil nodes (got {len(nodes)})")
    return nodes


def _put_table(plan, nodes, rows, xi, sampling, Xh, device):
    """The table arguments the hyper-reduced closure and quadratic loops share, on ``device``: ``nodes`` (int64, for
    gathers), ``node``, ``pos``, ``xi``, ``xn``, with ``m``, ``n_nodes``, ``Xh`` and the ``sampling``."""
    plan.m, plan.n_nodes, plan.Xh, plan.sampling = len(rows), len(nodes), Xh.copy(), sampling
    plan.nodes = torch.as_tensor(nodes, dtype=torch.int64, device=device)
    plan.node = plan.nodes.to(torch.int32)
    plan.pos = torch.as_tensor(np.searchsorted(nodes, rows), dtype=torch.int32, device=device)
    plan.xi = torch.as_tensor(xi, dtype=torch.float64, device=device)
    plan.xn = _as_dev(Xh[nodes], device)


def _put_stencil(plan, rows, xi, sampling, Xh, device):
    """The stencil arguments the hyper-reduced POD and local loops share, on ``device``: the gather index ``stencil`` (m, 3)
    of the nodes i-1, i, i+1 of every sampled row, clipped to the mesh, with ``inside`` marking the slots that exist, their
    coordinates ``xs``, ``rows`` (int32) and ``xi``, with ``m``, ``Xh`` and the ``sampling``."""
    plan.m, plan.Xh, plan.sampling = len(rows), Xh.copy(), sampling
    idx = torch.as_tensor(rows, device=device)[:, None] + torch.arange(-1, 2, device=device)[None, :]      # (m, 3)
    plan.inside = (idx >= 0) & (idx < len(Xh))
    plan.stencil = idx.clamp(0, len(Xh) - 1)
    plan.xs = _as_dev(Xh, device)[plan.stencil].contiguous()
    plan.rows = torch.as_tensor(rows, dtype=torch.int32, device=device)
    plan.xi = torch.as_tensor(xi, dtype=torch.float64, device=device)


def _require_orthonormal(U, what, carried):
    """ValueError unless the host matrix ``U`` is finite with |U^T U - I|_max <= 1e-8: the hyper loops carry their reduced
    coordinates from step to step instead of re-projecting ``carried``, which is exact only for orthonormal columns."""
    if not np.isfinite(U).all() or np.abs(U.T @ U - np.eye(U.shape[1])).max() > 1e-8:
        raise ValueError(f"{what} must have orthonormal columns (to 1e-8): the loop does not re-project {carried}")


def _check_hyper_call(plan, Xh, device, proj):
    """A hyper plan against the call it serves: its device, mesh and projection, each a ValueError.  Returns the device."""
    device = _lib.require_device(device)
    if plan.xi.device != device:
        raise ValueError("the plan was built on another device")
    if not np.array_equal(plan.Xh, Xh):
        raise ValueError("the plan was built for another mesh")
    if plan.projection != proj:
        raise ValueError("the row sampling was trained for the other projection")
    return device


class _HyperResult:
    """What the results of the hyper-reduced loops share: the reduced coordinates ``q`` (B, nT+1, r), ``iters``, ``flags``,
    ``info``, the ``path`` and the ``plan``.  ``hist`` (B, nT+1, N) is decoded on demand by the subclass's ``_decode`` with u0
    itself in column 0 as in every other loop, and kept; ``snapshots()`` is its (B, N, nT+1) layout."""

    def __init__(self, res, plan, u0d):
        self.q, self.iters, self.flags, self.info, self.path = res.hist, res.iters, res.flags, res.info, res.path
        self.plan, self._keep, self._u0, self._hist = plan, res._keep, u0d, None

    @property
    def hist(self):
        if self._hist is None:
            self._hist = self._decode()
            self._hist[:, 0] = self._u0
        return self._hist

    def snapshots(self):
        return FomResult(self.hist, self.iters, self.flags).snapshots()

    @property
    def newton_steps(self):
        return int(self.iters.sum().item())


class HyperPodPlan:
    """What bg_hyper_rom_run reads besides the batch, built once per basis, sampling and mesh on the device
    (include/burgers_hip.h): the packed stencil table PhiS (rows Phi[i-1], Phi[i], Phi[i+1] of every sampled row, 42 doubles
    each, zero outside the mesh and beyond r) and _put_stencil's arguments: the stencil coordinates xs (m, 3), the rows and
    weights, and the gather index of the stencil nodes.  ``sampling``: a pod.RowSampling.  What the shapes and the sampling
    alone decide is refused before the device is touched; every refusal is a ValueError."""
    entry, limits, table_elems, slab_rows = "bg_hyper_rom_run", "bg_hyper_rom_limits", "bg_hyper_rom_table_elems", 32
    slots = work = None           # HyperBlockedPodPlan: its workgroups and their workspace, one slot each

    def __init__(self, Phi, sampling, X, device):
        shape = tuple(np.shape(Phi))
        if len(shape) != 2:
            raise ValueError("Phi must be (N, r)")
        N, r = shape
        route = _ROUTES[self.entry]
        max_r, max_m = _lib.limits(self.limits, 2)
        Xh = check_mesh(X)
        if r < 1 or r > max_r:
            raise ValueError(f"Phi must be (N, r) with 1 <= r <= {max_r}")
        if N < route.min_n or N > _limit(route.max_n) or len(Xh) != N:
            raise ValueError(f"{route.entry} covers {route.min_n} <= N <= {_limit(route.max_n)} with one row of Phi per mesh node")
        rows, xi = _sampling_rows(route, sampling, N, max_m)
        m = len(rows)
        elems = getattr(_lib.load(), self.table_elems)(m, r)
        if elems == 0:
            raise ValueError(f"{route.entry} covers at most {max_m} sampled rows (got {m})")
        self.projection = _projection(str(sampling.projection), _SAMPLING_PROJECTION)
        device = _lib.require_device(device)
        self.Phi = _as_dev(Phi, device)
        self.N, self.r = N, r
        _put_stencil(self, rows, xi, sampling, Xh, device)
        cols = elems // (3 * ((m + self.slab_rows - 1) // self.slab_rows * self.slab_rows))
        table = torch.zeros((elems // (3 * cols), 3, cols), dtype=torch.float64, device=device)
        table[:m, :, :r] = self.Phi[self.stencil] * self.inside[:, :, None]
        self.PhiS = table


class HyperWidePodPlan(HyperPodPlan):
    """What bg_hyper_rom_run_wide reads besides the batch: a HyperPodPlan against the wide loop's limits (r <= 96, m <= 512,
    bg_hyper_rom_wide_limits) with the table PhiS in its layout, 98 doubles per row and m rounded up to 16.  The basis, the
    rows and the weights it keeps also serve the redo of marked samples (_pod_prom_run_hyper_library)."""
    entry, limits, table_elems, slab_rows = "bg_hyper_rom_run_wide", "bg_hyper_rom_wide_limits", "bg_hyper_rom_wide_table_elems", 16


class HyperBlockedPodPlan(HyperPodPlan):
    """What bg_hyper_rom_run_blocked reads and writes besides the batch: a HyperPodPlan against the blocked loop's limits
    (r <= 256, m <= 1024, bg_hyper_rom_blocked_limits) with the table PhiS in its layout, r rounded up to 16 doubles per row and
    m rounded up to 8, and BlockedPodPlan's workspace of ``slots`` slots (one per workgroup; default: one per compute unit,
    the kernel's LDS admits one workgroup per CU).  The basis, the rows and the weights it keeps also serve the redo of marked
    samples (_pod_prom_run_hyper_library)."""
    entry, limits, table_elems, slab_rows = ("bg_hyper_rom_run_blocked", "bg_hyper_rom_blocked_limits",
                                             "bg_hyper_rom_blocked_table_elems", 8)

    def __init__(self, Phi, sampling, X, device, slots=None):
        if slots is not None and int(slots) < 1:
            raise ValueError("slots must be positive")
        super().__init__(Phi, sampling, X, device)
        self.slots = int(slots) if slots is not None else _cu_count(self.Phi.device)
        self.work = torch.empty((self.slots, _lib.load().bg_hyper_rom_blocked_work_elems(self.r)), dtype=torch.float64,
                                device=self.Phi.device)


class HyperRomResult(_HyperResult):
    """Result of pod_prom_run_hyper (_HyperResult); from the wide and the blocked loop also ``redone``, the number of samples redone on the
    host side.  The decode is U = Phi q as one batched product."""

    def _decode(self):
        return torch.matmul(self.q, self.plan.Phi.t())


def _pivot_on_device(pivot):
    """The ``pivot`` keyword of the hyper-reduced POD loops: True for "device", False for "host", anything else a ValueError."""
    if pivot not in ("host", "device"):
        raise ValueError(f'pivot must be "host" or "device" (got {pivot!r})')
    return pivot == "device"


def _run_hyper_pod(plan_type, X, u0, mu1, mu2, dt, nsteps, Phi, sampling_or_plan, proj, E, tol, max_it, device, options, balance,
                   pivot="host"):
    """pod_prom_run_hyper's narrow loop, pod_prom_run_hyper_wide and pod_prom_run_hyper_blocked: the plan (or the sampling to build one from) against the
    call, q0 and u0 at the stencil, the launch, and for a route with ``redo`` the marked samples again on the host side, or
    with ``pivot="device"`` by the entry point's own repair kernel (BG_OPT_PIVOT_ON_DEVICE; the narrow loop always has one)."""
    route = _ROUTES[plan_type.entry]
    on_device = _pivot_on_device(pivot) and route.redo
    if on_device:
        options |= _lib.BG_OPT_PIVOT_ON_DEVICE
    Xh = check_mesh(X)
    if isinstance(sampling_or_plan, HyperPodPlan) and type(sampling_or_plan) is not plan_type:
        raise ValueError(f"{route.entry} takes a {plan_type.__name__}")
    plan = sampling_or_plan if isinstance(sampling_or_plan, plan_type) else plan_type(Phi, sampling_or_plan, Xh, device)
    device = _check_hyper_call(plan, Xh, device, proj)
    u0d, _, mu2d = _batch_inputs(u0, mu1, mu2, plan.N, device)
    q0 = (u0d @ plan.Phi).contiguous()
    u0s = (u0d[:, plan.stencil] * plan.inside).contiguous()
    work = () if plan.slots is None else (_lib.ptr(plan.work), plan.slots)
    res = _device_loop(route, Xh, u0d, mu1, mu2, nsteps, device, options, balance,
                       lambda f, N, B, x, inputs, opts, outputs: f(
                           N, B, plan.r, plan.m, int(nsteps), proj, _lib.ptr(plan.rows), _lib.ptr(plan.xi), _lib.ptr(plan.xs),
                           _lib.ptr(plan.PhiS), _lib.ptr(q0), _lib.ptr(u0s), *inputs[1:], float(dt), float(E), float(tol),
                           int(max_it), opts, *work, *outputs), keep=(plan, q0, u0s), slots=plan.slots, cols=plan.r)
    out = HyperRomResult(res, plan, u0d)
    if on_device:
        out.redone = 0                          # nothing comes back marked: info is not read, nothing is synchronised
    elif route.redo:
        _redo_marked_hyper(out, plan, dt, nsteps, proj, E, tol, max_it)
    return out


def pod_prom_run_hyper(X, u0, mu1, mu2, dt, nsteps, Phi, sampling_or_plan, proj, E=0.0, tol=1e-6, max_it=20, device=None,
                       options=0, balance=True, pivot="host"):
    """``pod_prom_burgers`` HYPER-REDUCED, with the whole time loop on the device (bg_hyper_rom_run): the reduced system
    is assembled from the sampled mesh rows of a pod.RowSampling (pod.build_row_sampling) with their weights, so an
    iteration costs O(m r^2) whatever the mesh: N up to bg_fom_max_n(), r <= 40, m <= 256 (bg_hyper_rom_limits).  The
    pivoting repair runs inside the call, nothing is synchronised.  ``sampling_or_plan``: the sampling, or a HyperPodPlan
    of this basis, sampling and mesh to reuse across calls (``res.plan``; ``Phi`` is then not looked at).  A sampling trained
    for the other projection is refused.  Returns a HyperRomResult.
    A HyperWidePodPlan, or a sampling with a basis of more than bg_hyper_rom_limits' r modes, goes to the wide loop
    (pod_prom_run_hyper_wide: r <= 96, m <= 512, which does synchronise unless ``pivot="device"``; with a narrow plan the
    keyword is accepted and changes nothing).  A HyperBlockedPodPlan goes to pod_prom_run_hyper_blocked (r <= 256, m <= 1024);
    a sampling with a basis of more than 96 modes is refused here and taken there."""
    _pivot_on_device(pivot)
    if isinstance(sampling_or_plan, HyperBlockedPodPlan):
        return pod_prom_run_hyper_blocked(X, u0, mu1, mu2, dt, nsteps, Phi, sampling_or_plan, proj, E, tol, max_it, device, options,
                                          balance, pivot)
    if isinstance(sampling_or_plan, HyperWidePodPlan) or (
            not isinstance(sampling_or_plan, HyperPodPlan) and len(np.shape(Phi)) == 2
            and np.shape(Phi)[1] > _lib.limits(HyperPodPlan.limits, 2)[0]):
        return pod_prom_run_hyper_wide(X, u0, mu1, mu2, dt, nsteps, Phi, sampling_or_plan, proj, E, tol, max_it, device, options,
                                       balance, pivot)
    return _run_hyper_pod(HyperPodPlan, X, u0, mu1, mu2, dt, nsteps, Phi, sampling_or_plan, proj, E, tol, max_it, device, options,
                          balance, pivot)


def pod_prom_run_hyper_wide(X, u0, mu1, mu2, dt, nsteps, Phi, sampling_or_plan, proj, E=0.0, tol=1e-6, max_it=20, device=None,
                            options=0, balance=True, pivot="host"):
    """pod_prom_run_hyper for bases of up to 96 modes on up to 512 sampled rows (bg_hyper_rom_run_wide,
    bg_hyper_rom_wide_limits; meant for r > 40): the same loop with pod_prom_run_wide's 96 x 96 solve.  There is no repair
    kernel: samples whose elimination would have needed a row exchange come back marked and are redone by the weighted-row
    library iteration (_pod_prom_run_hyper_library) -- the full PROM's library path answers another question -- so unlike
    pod_prom_run_hyper this wrapper reads ``info`` back and synchronises the host.  ``sampling_or_plan``: the sampling, or a
    HyperWidePodPlan to reuse across calls.  Returns a HyperRomResult with ``redone``.
    ``pivot="device"`` (BG_OPT_PIVOT_ON_DEVICE): the entry point's repair kernel redoes those samples with a pivoted 96 x 96
    solve on the device instead; ``redone`` is 0, ``info`` is not read back and nothing is synchronised, and an exactly
    singular reduced system is left in ``info`` for check_singular, as by the narrow loop.  Any other value is a ValueError."""
    return _run_hyper_pod(HyperWidePodPlan, X, u0, mu1, mu2, dt, nsteps, Phi, sampling_or_plan, proj, E, tol, max_it, device,
                          options, balance, pivot)


def pod_prom_run_hyper_blocked(X, u0, mu1, mu2, dt, nsteps, Phi, sampling_or_plan, proj, E=0.0, tol=1e-6, max_it=20, device=None,
                               options=0, balance=True, pivot="host"):
    """pod_prom_run_hyper for bases of up to 256 modes on up to 1024 sampled rows (bg_hyper_rom_run_blocked,
    bg_hyper_rom_blocked_limits; meant for r > 96, the thesis' r = 160 and 227): pod_prom_run_blocked's projection and blocked
    elimination in a per-workgroup workspace slot, driven over the table of sampled rows.  With all rows and unit weights it
    is the full PROM, on any mesh of up to 1024 nodes.  Samples whose elimination would have needed a row exchange come back
    marked and are redone by the weighted-row library iteration (_pod_prom_run_hyper_library), so this wrapper reads ``info``
    back and synchronises the host.  ``sampling_or_plan``: the sampling, or a HyperBlockedPodPlan to reuse across calls
    (``res.plan``).  Returns a HyperRomResult with ``redone``.  The loop has no repair kernel: ``pivot="device"`` is a
    ValueError, as is any value but "host"."""
    if _pivot_on_device(pivot):
        raise ValueError('bg_hyper_rom_run_blocked has no repair kernel: pivot must be "host"')
    return _run_hyper_pod(HyperBlockedPodPlan, X, u0, mu1, mu2, dt, nsteps, Phi, sampling_or_plan, proj, E, tol, max_it, device,
                          options, balance)


def _redo_marked_hyper(out, plan, dt, nsteps, proj, E, tol, max_it):
    """_redo_marked for a HyperRomResult: the samples marked BG_INFO_NEEDS_PIVOTING again through the weighted-row library
    iteration (LU with partial pivoting).  Reads ``info`` back, so it synchronises the host."""
    _, u0d, mu1d, mu2d = out._keep[:4]
    redo = (out.info == _lib.BG_INFO_NEEDS_PIVOTING).nonzero().squeeze(1)
    if redo.numel():
        rr = _pod_prom_run_hyper_library(plan, u0d[redo], mu1d[redo], mu2d[redo], dt, nsteps, proj, E, tol, max_it)
        out.q[redo], out.iters[redo], out.flags[redo] = rr.q, rr.iters, rr.flags
        out.info[redo] = 0
    out.redone = int(redo.numel())


def check_singular(res):
    """np.linalg.solve raises LinAlgError('Singular matrix') at :767; the device loop records it per sample."""
    info = getattr(res, "info", None)
    if info is not None and bool(info.ne(0).any()):
        raise SingularReducedSystem("Singular matrix")
    return res


def _pod_route(N, r, fused=True, blocked=False, long_mesh=False, long_wide=False):
    """Which way pod_prom_run takes an (N, r) basis, by the library's limits alone: a device loop's entry point, "library"
    or "host"; the first test that applies wins (the table in DESIGN.md, "Host side of the device-side loops")."""
    run, wide, blk, long, lw = (_ROUTES["bg_rom_run" + k] for k in ("", "_wide", "_blocked", "_long", "_long_wide"))
    if long_mesh and fused and run.max_n < N <= _limit(long.max_n) and r <= _limit(long.max_r):
        return long.entry
    if long_wide and fused and run.max_n < N <= _limit(lw.max_n) and _limit(long.max_r) < r <= _limit(lw.max_r):
        return lw.entry
    if blocked and fused and _limit(wide.max_r) < r <= _limit(blk.max_r) and N <= blk.max_n:
        return blk.entry
    if fused and _limit(run.max_r) < r <= _limit(wide.max_r) and N <= wide.max_n:
        return wide.entry
    if r > _limit("bg_rom_max_r") or N > _limit("bg_rom_max_n"):
        return "library"
    if fused and r <= _limit(run.max_r):
        return run.entry
    return "host"


def pod_prom_run(X, u0, mu1, mu2, dt, nsteps, Phi, projection="Galerkin", E=0.0, tol=1e-6, max_it=20,
                 device=None, fused=True, blocked=False, long_mesh=False, long_wide=False, hyper=None, pivot="host"):
    """Batched ``pod_prom_burgers``; ``projection`` is case-sensitive like the reference (:754-764).
    ``fused`` (default): the device-side time loop bg_rom_run where it applies (N <= 512, r <= 40); otherwise, or
    with ``fused=False``, the batched iteration bg_rom_reduce -> bg_lu_solve_update driven from the host.
    ``blocked`` (opt-in, with ``fused``): bases of bg_rom_run_wide_max_r() < r <= bg_rom_run_blocked_max_r() on
    N <= 512 take the device-side loop bg_rom_run_blocked instead of the library path.
    ``long_mesh`` (opt-in, with ``fused``): meshes of 512 < N <= bg_rom_run_long_max_n() with r <= bg_rom_run_long_max_r()
    take the device-side loop bg_rom_run_long instead of the library path.
    ``long_wide`` (opt-in, with ``fused``): meshes of 512 < N <= bg_rom_run_long_wide_max_n() with bg_rom_run_long_max_r() < r
    <= bg_rom_run_long_wide_max_r() take the device-side loop bg_rom_run_long_wide instead of the library path.
    ``hyper`` (opt-in): a pod.RowSampling, a HyperPodPlan or a HyperWidePodPlan sends the call through the hyper-reduced loop
    pod_prom_run_hyper, which assembles the reduced system from the sampled mesh rows only (r <= 40: bg_hyper_rom_run;
    41 <= r <= 96: bg_hyper_rom_run_wide); sizes it does not cover are refused, not rerouted.  With ``blocked`` a sampling
    with a basis of more than 96 modes, and without it a HyperBlockedPodPlan, goes through pod_prom_run_hyper_blocked
    (97 <= r <= 256, at most 1024 rows: bg_hyper_rom_run_blocked); ``blocked`` with at most 96 modes changes nothing here.
    ``pivot`` (with ``hyper``): "device" has bg_hyper_rom_run_wide redo the samples that need row exchanges in its own repair
    kernel, where "host" (default) redoes them through the library; the narrow loop always repairs on the device, the
    blocked one never does and refuses "device"."""
    proj = _projection(projection, _NOT_AVAILABLE, exact=True)
    _pivot_on_device(pivot)
    if hyper is not None:
        if (blocked and not isinstance(hyper, HyperPodPlan) and len(np.shape(Phi)) == 2
                and np.shape(Phi)[1] > _lib.limits(HyperWidePodPlan.limits, 2)[0]):
            return check_singular(pod_prom_run_hyper_blocked(X, u0, mu1, mu2, dt, nsteps, Phi, hyper, proj, E, tol, max_it, device,
                                                             pivot=pivot))
        return check_singular(pod_prom_run_hyper(X, u0, mu1, mu2, dt, nsteps, Phi, hyper, proj, E, tol, max_it, device, pivot=pivot))
    route = _pod_route(np.shape(Phi)[0], np.shape(Phi)[1], fused, blocked, long_mesh, long_wide)
    if route == "library":
        return _pod_prom_run_library(X, u0, mu1, mu2, dt, nsteps, Phi, proj, E, tol, max_it, device)
    if route != "host":
        run = {"bg_rom_run": pod_prom_run_fused, "bg_rom_run_wide": pod_prom_run_wide,
               "bg_rom_run_blocked": pod_prom_run_blocked, "bg_rom_run_long": pod_prom_run_long,
               "bg_rom_run_long_wide": pod_prom_run_long_wide}[route]
        return check_singular(run(X, u0, mu1, mu2, dt, nsteps, Phi, proj, E, tol, max_it, device))
    c = _setup(X, u0, mu1, mu2, dt, E, device)
    Phid = _as_dev(Phi, c.device)
    if Phid.shape[0] != c.N:
        raise ValueError("Phi must have one row per mesh node")
    r = Phid.shape[1]
    q = torch.zeros((c.B, r), dtype=torch.float64, device=c.device)

    def step(n, U0, st, Ar, br, wtu, G):
        first = n == 0                      # u0 is not in span(Phi): the very first assembly reads it from HBM
        while True:
            if first:
                rom_reduce(c, Phid, U0, G, proj, True, st.active, Ar, br, wtu)
                first = False
            else:                           # u_k = Phi q formed in-kernel                 (:773)
                rom_reduce_lifted(c, Phid, q, U0, G, proj, True, st.active, Ar, br, wtu)
            if st.solve_update(1, Ar, br, wtu, q, tol, max_it) == 0:     # q = Phi^T U0 + dq (:767-776)
                break
        rom_lift(c, Phid, q, U0)            # U[:, n+1] = Phi q                            (:779)
        return U0

    return _host_loop(c, nsteps, r, step)


def _batched_solve(A, b, considered):
    """x = solve(A, b) over a batch (rocSOLVER LU).  Like numpy (:767), an exactly singular FINITE system of a
    sample that is still iterating raises; a system that already holds NaN/Inf (a diverged sample) does not --
    its solution is simply non-finite, which the caller flags -- and neither does a sample that is masked out.
    The batch goes through in chunks: hipblasDgetrfBatched fails to allocate its workspace beyond about
    n^2 * batch = 1e7 (n = 160: 256 systems pass, 512 do not; tools/probe_solve.py)."""
    B, n, _ = A.shape
    chunk = max(16, int(6.0e6 / (n * n)))
    x = torch.empty_like(b)
    info = torch.empty((B,), dtype=torch.int32, device=A.device)
    for b0 in range(0, B, chunk):
        xs, inf = torch.linalg.solve_ex(A[b0:b0 + chunk], b[b0:b0 + chunk], check_errors=False)
        x[b0:b0 + chunk] = xs
        info[b0:b0 + chunk] = inf
    bad = (info != 0) & considered & torch.isfinite(A).all(dim=2).all(dim=1)
    if bool(bad.any()):
        raise SingularReducedSystem("Singular matrix")
    return x


def _pod_prom_run_library(X, u0, mu1, mu2, dt, nsteps, Phi, proj, E, tol, max_it, device):
    """POD PROM for bases beyond the register-resident MFMA kernels (r > 47 or N > 512; the thesis
    also runs r = 96, 160, 227): bg_fom_assemble (HIP) for A(u), R(u), then the projection and
    the reduced solve as plain library calls over the batch (rocBLAS GEMMs, rocSOLVER LU).
    Same loop and stopping rule as the fused path; slower, but it keeps the API total."""
    from . import fom as _fom
    L = _lib.load()
    c = _setup(X, u0, mu1, mu2, dt, E, device, max_n=L.bg_fom_max_n())
    Xh = c.X.cpu().numpy()
    Phid = _as_dev(Phi, c.device)
    if Phid.shape[0] != c.N:
        raise ValueError("Phi must have one row per mesh node")
    PhiT = Phid.t().contiguous()
    zrow = torch.zeros((1, Phid.shape[1]), dtype=torch.float64, device=c.device)
    PhiT_dn = torch.cat([zrow, Phid[:-1]], 0).t().contiguous()     # column i holds Phi[i-1]
    PhiT_up = torch.cat([Phid[1:], zrow], 0).t().contiguous()      # column i holds Phi[i+1]
    hist, iters, flags = _alloc_hist(c, nsteps)
    U0 = c.u0.clone()
    for n in range(nsteps):
        Un = U0.clone()
        active = torch.ones((c.B,), dtype=torch.bool, device=c.device)
        k = torch.zeros((c.B,), dtype=torch.int32, device=c.device)
        while True:
            lo, di, up, rhs = _fom.fom_assemble(Xh, U0, Un, c.mu1, c.mu2, c.dt, E=c.E, supg=True, device=c.device)
            # (A Phi)^T as (B, r, N): the Galerkin projection is then ONE GEMM over B r rows against Phi
            YT = di.unsqueeze(1) * PhiT + lo.unsqueeze(1) * PhiT_dn + up.unsqueeze(1) * PhiT_up
            if proj == _lib.BG_PROJ_GALERKIN:
                Ar = torch.matmul(YT, Phid).transpose(1, 2)                  # Phi^T A Phi       (:756)
                br = -(rhs @ Phid)                                           # Phi^T R, R = -rhs (:757)
            else:
                Ar = torch.matmul(YT, YT.transpose(1, 2))                    # (A Phi)^T (A Phi) (:761)
                br = -torch.matmul(YT, rhs.unsqueeze(-1)).squeeze(-1)
            dq = _batched_solve(Ar, -br, active)                            # np.linalg.solve (:767)
            q = U0 @ Phid + dq
            U1 = q @ PhiT
            err = torch.linalg.vector_norm(dq, dim=1) / torch.linalg.vector_norm(q, dim=1)
            U0 = torch.where(active[:, None], U1, U0)
            k += active.to(torch.int32)
            flags |= (active & ~torch.isfinite(err)).to(torch.int32) * _lib.BG_FLAG_NONFINITE
            active = active & (err > tol) & (k < max_it)
            if not bool(active.any()):
                break
        flags |= (k >= max_it).to(torch.int32) * _lib.BG_FLAG_HIT_CAP
        iters[:, n] = k
        hist[:, n + 1] = U0
    return FomResult(hist, iters, flags, path="library")


# ------------------------------------------------------------ quadratic manifold
def _pod_prom_run_hyper_library(plan, u0, mu1, mu2, dt, nsteps, proj, E, tol, max_it):
    """_pod_prom_run_library with the two projections restricted to the rows of ``plan`` (a HyperPodPlan or HyperWidePodPlan)
    and weighted by its xi (any r) -- bg_hyper_rom_run's iteration as library calls: bg_fom_assemble on the full state, the sampled
    rows gathered, the rows of Y = A Phi from the stencil, rocSOLVER LU, q <- q + dq, the first assembly at u0 itself.  It
    redoes the samples bg_hyper_rom_run_wide and bg_hyper_rom_run_blocked hand back and is the baseline of
    tools/time_hyper_wide_rom.py and tools/time_hyper_blocked_rom.py.  Returns a
    namespace with ``q`` (B, nT+1, r), ``iters``, ``flags`` and ``path``."""
    from . import fom as _fom
    c = _setup(plan.Xh, u0, mu1, mu2, dt, E, plan.Phi.device, max_n=_lib.load().bg_fom_max_n())
    rows = plan.rows.long()
    P3 = plan.Phi[plan.stencil] * plan.inside[:, :, None]            # (m, 3, r): Phi[i-1], Phi[i], Phi[i+1] of every sampled row
    gal = proj == _lib.BG_PROJ_GALERKIN
    w = plan.xi if gal else plan.xi.sqrt()                            # the weight goes into lo, di, up and R, as in the kernel
    PhiT = plan.Phi.t().contiguous()
    qhist = torch.empty((c.B, nsteps + 1, plan.r), dtype=torch.float64, device=c.device)
    iters = torch.zeros((c.B, nsteps), dtype=torch.int32, device=c.device)
    flags = torch.zeros((c.B,), dtype=torch.int32, device=c.device)
    q = c.u0 @ plan.Phi
    qhist[:, 0] = q
    U0 = c.u0.clone()
    for n in range(nsteps):
        Un = U0.clone()
        active = torch.ones((c.B,), dtype=torch.bool, device=c.device)
        k = torch.zeros((c.B,), dtype=torch.int32, device=c.device)
        while True:
            lo, di, up, rhs = _fom.fom_assemble(plan.Xh, U0, Un, c.mu1, c.mu2, c.dt, E=c.E, supg=True, device=c.device)
            lo, di, up, rhs = (v[:, rows] * w for v in (lo, di, up, rhs))
            Y = lo.unsqueeze(2) * P3[:, 0] + di.unsqueeze(2) * P3[:, 1] + up.unsqueeze(2) * P3[:, 2]      # (B, m, r), weighted
            W = P3[:, 1].expand(c.B, -1, -1) if gal else Y
            Ar = torch.matmul(W.transpose(1, 2), Y)                         # sum_j xi_j w_j^T y_j
            br = -torch.matmul(W.transpose(1, 2), rhs.unsqueeze(2)).squeeze(2)      # sum_j xi_j w_j R_j, R = -rhs
            dq = _batched_solve(Ar, -br, active)
            qn = q + dq
            err = torch.linalg.vector_norm(dq, dim=1) / torch.linalg.vector_norm(qn, dim=1)
            q = torch.where(active[:, None], qn, q)
            U0 = torch.where(active[:, None], q @ PhiT, U0)
            k += active.to(torch.int32)
            flags |= (active & ~torch.isfinite(err)).to(torch.int32) * _lib.BG_FLAG_NONFINITE
            active = active & (err > tol) & (k < max_it)
            if not bool(active.any()):
                break
        flags |= (k >= max_it).to(torch.int32) * _lib.BG_FLAG_HIT_CAP
        iters[:, n] = k
        qhist[:, n + 1] = q
    return SimpleNamespace(q=qhist, iters=iters, flags=flags, path="library")


def sym_index_tables(n, device):
    """Row-major upper-triangle pair order of get_sym (:263-273) and the (n, n) lookup of
    the pair index, with the factor (1 + delta_ab) of get_dQ_dq (:292-312)."""
    I, J = np.triu_indices(n)
    idx = np.zeros((n, n), dtype=np.int64)
    idx[I, J] = np.arange(len(I))
    idx[J, I] = np.arange(len(I))
    fac = np.ones((n, n)) + np.eye(n)
    return (torch.as_tensor(I, device=device), torch.as_tensor(J, device=device),
            torch.as_tensor(idx, device=device), torch.as_tensor(fac, device=device))


def quad_tangent_tensor(Phid, Hd):
    """H3[i][a][c] = H[i][pair(a, c)] (1 + delta_ac), (N, n, n): tangent = Phi + H3 . q (:1120-1123 with get_dQ_dq
    :292-312 folded in)."""
    n = Phid.shape[1]
    _, _, idx, fac = sym_index_tables(n, Phid.device)
    return (Hd[:, idx] * fac).contiguous()


def _quad_operand_copies(Phid, Hd):
    """PhiT, Phif, H3f of bg_quad_rom_run and bg_quad_rom_run_long (layouts: include/burgers_hip.h) from Phi (N, n) and
    H (N, n(n+1)/2) on the device, n <= 40."""
    device = Phid.device
    N, n = Phid.shape
    f64 = dict(dtype=torch.float64, device=device)
    NG, NPAD = (N + 3) // 4, (N + 63) // 64 * 64
    PhiT = torch.zeros((40, NPAD), **f64)
    PhiT[:n, :N] = Phid.t()
    Pp = torch.zeros((4 * NG, 40), **f64)
    Pp[:N, :n] = Phid
    # accumulator seeds of the tangent tiles: (rg, blk, c, i) -> [rg][c][4 i + blk]
    Phif = Pp.reshape(NG, 4, 10, 4).permute(0, 2, 3, 1).contiguous()
    H3p = torch.zeros((4 * NG, 40, 40), **f64)
    H3p[:N, :n, :n] = quad_tangent_tensor(Phid, Hd)
    # H3 of a mesh row is symmetric: only its upper 4 x 4 blocks (a <= b, row-major) travel.  Block (a, b), lane 16 k + 4 blk + i
    # = H3[4 rg + blk][4 a + i][4 b + k]; two blocks per 16-byte slot: [rg][slot (28)][lane][2] (block 55 = zero padding)
    Hb = H3p.reshape(NG, 4, 10, 4, 10, 4).permute(0, 2, 4, 5, 1, 3)           # (rg, a, b, k, blk, i)
    A_, B_ = np.triu_indices(10)
    Hu = Hb[:, torch.as_tensor(A_, device=device), torch.as_tensor(B_, device=device)].reshape(NG, 55, 64)
    Hu = torch.cat([Hu, torch.zeros((NG, 1, 64), **f64)], 1)
    H3f = Hu.reshape(NG, 28, 2, 64).permute(0, 1, 3, 2).contiguous()
    return PhiT, Phif, H3f


class _QuadPlan:
    """What QuadFusedPlan and QuadLongPlan share: the H-shape check (before the device is touched), (Phi, H) on the device
    and, for a basis the loop covers (``covers(N, n)``, which may raise instead; ``ok``), _quad_operand_copies."""

    def __init__(self, Phi, H, device, covers):
        N, n = self.N, self.n = tuple(np.shape(Phi))
        self.ok = covers(N, n)
        if tuple(np.shape(H)) != (N, n * (n + 1) // 2):
            raise ValueError("Phi must be (N, n) and H (N, n(n+1)/2)")
        device = _lib.require_device(device)
        self.Phi, self.H = _as_dev(Phi, device), _as_dev(np.ascontiguousarray(H) if isinstance(H, np.ndarray) else H, device)
        if self.ok:
            self.PhiT, self.Phif, self.H3f = _quad_operand_copies(self.Phi, self.H)


def _run_quad_route(route, Xh, plan, u0, mu1, mu2, dt, nsteps, proj, E, newton_tol, newton_itmax, device, balance):
    return _device_loop(route, Xh, u0, mu1, mu2, nsteps, device, 0, balance,
                        lambda f, N, B, x, inputs, opts, outputs: f(
                            N, B, plan.n, int(nsteps), proj, x, _lib.ptr(plan.PhiT), _lib.ptr(plan.Phif), _lib.ptr(plan.H3f),
                            *inputs, float(dt), float(E), float(newton_tol), int(newton_itmax), opts, *outputs), keep=(plan,))


class QuadFusedPlan(_QuadPlan):
    """The operand copies bg_quad_rom_run reads, built once per (Phi, H) on the device (include/burgers_hip.h):
    Phi^T zero padded, the accumulator seeds of the tangent tiles, and H3 in the A-operand order of the matrix
    instruction.  None-like (``ok`` False) when the basis is beyond the kernel (N > 512 or n > 40)."""

    def __init__(self, Phi, H, device):
        L = _lib.load()
        super().__init__(Phi, H, device, lambda N, n: _quad_route(N, n) == "bg_quad_rom_run")
        assert not self.ok or (self.H3f.numel() == L.bg_quad_rom_h3f_elems(self.N)
                               and self.Phif.numel() == L.bg_quad_rom_phif_elems(self.N))


def quadratic_run_fused(X, u0, mu1, mu2, dt, nsteps, plan, proj, E=0.0, newton_tol=1e-6, newton_itmax=25, device=None,
                        balance=True):
    """``pod_quadratic_manifold`` for a batch with the whole time loop on the device (bg_quad_rom_run): four samples
    per workgroup, no host in the loop; the reduced solve pivots like np.linalg.solve."""
    device = _lib.require_device(device)
    Xh = check_mesh(X)
    if len(Xh) != plan.N:
        raise ValueError("Phi must be (N, n) and H (N, n(n+1)/2)")
    return _run_quad_route(_ROUTES["bg_quad_rom_run"], Xh, plan, u0, mu1, mu2, dt, nsteps, proj, E, newton_tol, newton_itmax,
                           device, balance)


class QuadLongPlan(_QuadPlan):
    """The operand copies bg_quad_rom_run_long reads, built once per (Phi, H) on the device (include/burgers_hip.h; the
    layouts of QuadFusedPlan).  Covers 512 < N <= bg_quad_rom_run_long_max_n() and n <= bg_quad_rom_run_long_max_r();
    anything else raises ValueError."""

    def __init__(self, Phi, H, device):
        L = _lib.load()
        if len(np.shape(Phi)) != 2:
            raise ValueError("Phi must be (N, n)")

        def covers(N, n):
            if n < 1 or n > L.bg_quad_rom_run_long_max_r():
                raise ValueError(f"Phi must be (N, n) with 1 <= n <= {L.bg_quad_rom_run_long_max_r()}")
            if N <= 512 or N > L.bg_quad_rom_run_long_max_n():
                raise ValueError(f"bg_quad_rom_run_long covers 512 < N <= {L.bg_quad_rom_run_long_max_n()}, not N = {N}")
            return True
        super().__init__(Phi, H, device, covers)
        N, n = self.N, self.n
        if (self.PhiT.numel(), self.Phif.numel(), self.H3f.numel()) != (
                L.bg_quad_rom_run_long_phit_elems(N), L.bg_quad_rom_run_long_phif_elems(N), L.bg_quad_rom_run_long_h3f_elems(N)):
            raise ValueError(f"bg_quad_rom_run_long does not cover N = {N}, n = {n}")


def quadratic_run_long(X, u0, mu1, mu2, dt, nsteps, Phi_H_or_plan, proj, E=0.0, newton_tol=1e-6, newton_itmax=25,
                       device=None, balance=True):
    """``pod_quadratic_manifold`` for meshes of 513 .. bg_quad_rom_run_long_max_n() = 1024 nodes and n <= 40 with the
    whole time loop on the device (bg_quad_rom_run_long): four samples per workgroup, nothing is synchronised.
    ``Phi_H_or_plan``: the pair (Phi, H), or a QuadLongPlan of it to reuse across calls (``res.plan``)."""
    device = _lib.require_device(device)
    Xh = check_mesh(X)
    plan = Phi_H_or_plan if isinstance(Phi_H_or_plan, QuadLongPlan) else QuadLongPlan(*Phi_H_or_plan, device)
    _check_plan(plan, Xh, device)
    res = _run_quad_route(_ROUTES["bg_quad_rom_run_long"], Xh, plan, u0, mu1, mu2, dt, nsteps, proj, E, newton_tol,
                          newton_itmax, device, balance)
    res.plan = plan
    return res


def _quad_decoder(Phid, Hd, rows):
    """decode(q) for q (rows, n) on the device: u = Phi q + H Q(q) (:1116-1118) as ONE GEMM [q | Q(q)] . [Phi^T; H^T]; the
    left operand comes from bg_quad_features."""
    L, device, n = _lib.load(), Phid.device, Phid.shape[1]
    I, J, _, _ = sym_index_tables(n, device)
    WT = torch.cat([Phid.t(), Hd.t()], 0).contiguous()       # (n + k, N)
    I32, J32 = I.to(torch.int32).contiguous(), J.to(torch.int32).contiguous()
    feat = torch.empty((rows, n + len(I)), dtype=torch.float64, device=device)

    def decode(q):
        with torch.cuda.device(device):
            _lib.check(L.bg_quad_features(rows, n, _lib.ptr(q), _lib.ptr(I32), _lib.ptr(J32), _lib.ptr(feat),
                                          _lib.stream_ptr(device)), "bg_quad_features")
        return feat @ WT
    return decode


class HyperQuadPlan:
    """What bg_hyper_quad_rom_run reads besides the batch, built once per manifold, sampling and mesh (include/burgers_hip.h):
    the table of the sorted distinct stencil nodes of the sampled rows (``nodes``, at most 3 m), their coordinates ``xn``,
    the table position ``pos`` of every sampled row, the weights ``xi``, and bg_quad_rom_run's operand copies Phif, H3f of
    Phi and H restricted to the table nodes.  ``sampling``: a pod.RowSampling (pod.build_quad_row_sampling).  Everything the
    shapes, the sampling and the manifold decide is refused with a ValueError before the device is touched -- also
    |Phi^T Phi - I|_max > 1e-8 or |Phi^T H|_max > 1e-8: the loop carries q from step to step instead of re-projecting
    Phi^T u^n, which is exact only for an orthonormal Phi and an H fitted on the residual of the projection."""

    def __init__(self, Phi, H, sampling, X, device):
        route = _ROUTES["bg_hyper_quad_rom_run"]
        max_n, max_m, max_nodes = _lib.limits("bg_hyper_quad_rom_limits", 3)
        Ph, Hh = _host64(Phi), _host64(H)
        if Ph.ndim != 2 or Ph.shape[1] < 1 or Hh.shape != (Ph.shape[0], Ph.shape[1] * (Ph.shape[1] + 1) // 2):
            raise ValueError("Phi must be (N, n) and H (N, n(n+1)/2)")
        N, n = Ph.shape
        Xh = check_mesh(X)
        if N < route.min_n or N > _limit(route.max_n) or len(Xh) != N:
            raise ValueError(f"{route.entry} covers {route.min_n} <= N <= {_limit(route.max_n)} with one row of Phi and H per mesh node")
        if n > max_n:
            raise ValueError(f"{route.entry} covers n <= {max_n} (got {n})")
        rows, xi = _sampling_rows(route, sampling, N, max_m)
        _require_orthonormal(Ph, "Phi", "Phi^T u^n")
        if not np.isfinite(Hh).all() or np.abs(Ph.T @ Hh).max() > 1e-8:
            raise ValueError("Phi^T H must vanish (to 1e-8): the loop does not re-project Phi^T u^n")
        nodes = _stencil_nodes(route, rows, N, max_nodes)
        self.projection = _projection(str(sampling.projection), _SAMPLING_PROJECTION)
        device = _lib.require_device(device)
        self.N, self.n = N, n
        self.Phi, self.H = _as_dev(Ph, device), _as_dev(Hh, device)
        _put_table(self, nodes, rows, xi, sampling, Xh, device)
        _, self.Phif, self.H3f = _quad_operand_copies(self.Phi[self.nodes].contiguous(), self.H[self.nodes].contiguous())
        L = _lib.load()
        assert (self.Phif.numel(), self.H3f.numel()) == (L.bg_hyper_quad_rom_phif_elems(len(nodes)), L.bg_hyper_quad_rom_h3f_elems(len(nodes)))


class HyperQuadRomResult(_HyperResult):
    """Result of quadratic_run_hyper (_HyperResult; column 0 of ``q``: Phi^T u0).  The decode is U = Phi q + H Q(q), that of
    the host-driven route."""

    def _decode(self):
        B, cols, n = self.q.shape
        return _quad_decoder(self.plan.Phi, self.plan.H, B * cols)(self.q.reshape(B * cols, n)).reshape(B, cols, -1)


def quadratic_run_hyper(X, u0, mu1, mu2, dt, nsteps, Phi, H, sampling_or_plan, proj, E=0.0, newton_tol=1e-6, newton_itmax=25,
                        device=None, balance=True):
    """``pod_quadratic_manifold`` HYPER-REDUCED, with the whole time loop on the device (bg_hyper_quad_rom_run): both
    projections are assembled from the sampled mesh rows of a pod.RowSampling (pod.build_quad_row_sampling) with their
    weights, on the table of their stencil nodes, so a pass streams a few hundred rows of the tangent tensor whatever the
    mesh: N up to bg_fom_max_n(), n <= 40, m <= 256, at most 768 table nodes (bg_hyper_quad_rom_limits).  q carries over from
    step to step (no Phi^T u^n: Phi must be orthonormal and Phi^T H = 0).  ``sampling_or_plan``: the sampling, or a
    HyperQuadPlan of this manifold, sampling and mesh to reuse across calls (``res.plan``; ``Phi`` and ``H`` are then not
    looked at).  A plan built for another mesh or device and a sampling trained for the other projection are refused.
    Nothing is synchronised.  Returns a HyperQuadRomResult."""
    Xh = check_mesh(X)
    plan = sampling_or_plan if isinstance(sampling_or_plan, HyperQuadPlan) else HyperQuadPlan(Phi, H, sampling_or_plan, Xh, device)
    device = _check_hyper_call(plan, Xh, device, proj)
    u0d, _, _ = _batch_inputs(u0, mu1, mu2, plan.N, device)
    q0 = _project_rows(u0d, plan.Phi)
    u0n = u0d[:, plan.nodes].contiguous()
    res = _device_loop(_ROUTES["bg_hyper_quad_rom_run"], Xh, u0d, mu1, mu2, nsteps, device, 0, balance,
                       lambda f, N, B, x, inputs, opts, outputs: f(
                           N, B, plan.n, plan.m, plan.n_nodes, int(nsteps), proj, _lib.ptr(plan.xn), _lib.ptr(plan.node),
                           _lib.ptr(plan.pos), _lib.ptr(plan.xi), _lib.ptr(plan.Phif), _lib.ptr(plan.H3f), _lib.ptr(q0),
                           _lib.ptr(u0n), *inputs[1:], float(dt), float(E), float(newton_tol), int(newton_itmax), opts, *outputs),
                       keep=(plan, q0, u0n), cols=plan.n)
    return HyperQuadRomResult(res, plan, u0d)


def _quad_route(N, n, fused=True, long_mesh=False):
    """Which way quadratic_run takes an (N, n) manifold: a device-side loop's entry point, or "host"."""
    quad, long = _ROUTES["bg_quad_rom_run"], _ROUTES["bg_quad_rom_run_long"]
    if long_mesh and fused and quad.max_n < N <= _limit(long.max_n) and n <= _limit(long.max_r):
        return long.entry
    if fused and N <= quad.max_n and n <= _limit(quad.max_r):
        return quad.entry
    return "host"


def quadratic_run(X, u0, mu1, mu2, dt, nsteps, Phi, H, projection="LSPG", E=0.0, newton_tol=1e-6,
                  newton_itmax=25, device=None, fused=True, plan=None, long_mesh=False, hyper=None):
    """Batched ``pod_quadratic_manifold`` (no SUPG term in this variant, :1142).  ``fused`` (default): the device-side
    time loop bg_quad_rom_run where it applies (N <= 512, n <= 40); otherwise, or with ``fused=False``, the batched
    iteration (bg_quad_tangent -> bg_rom_reduce_frag -> bg_lu_solve_update -> decode GEMM) driven from the host.
    ``plan``: a QuadFusedPlan of (Phi, H) to reuse across calls.
    ``long_mesh`` (opt-in, with ``fused``): meshes of 512 < N <= bg_quad_rom_run_long_max_n() with n <=
    bg_quad_rom_run_long_max_r() take the device-side loop bg_quad_rom_run_long instead of the host-driven iteration
    (``plan`` may then be a QuadLongPlan).
    ``hyper`` (opt-in): a pod.RowSampling (pod.build_quad_row_sampling) or a HyperQuadPlan sends the call through the
    hyper-reduced loop quadratic_run_hyper, which assembles both projections from the sampled mesh rows only; manifolds and
    samplings it does not cover are refused, not rerouted."""
    proj = _projection(projection, "projection must be 'Galerkin' or 'LSPG'")
    if hyper is not None:
        return check_singular(quadratic_run_hyper(X, u0, mu1, mu2, dt, nsteps, Phi, H, hyper, proj, E, newton_tol, newton_itmax, device))
    if long_mesh and fused and _quad_route(np.shape(Phi)[0], np.shape(Phi)[1], long_mesh=True) == "bg_quad_rom_run_long":
        what = plan if isinstance(plan, QuadLongPlan) else (Phi, H)
        return check_singular(quadratic_run_long(X, u0, mu1, mu2, dt, nsteps, what, proj, E, newton_tol, newton_itmax, device))
    if isinstance(plan, QuadLongPlan):
        plan = None
    if fused:
        dev = _lib.require_device(device)
        if plan is None:
            plan = QuadFusedPlan(Phi, H, dev)
        if plan.ok:                                      # _quad_route(N, n) of the plan's own basis
            return check_singular(quadratic_run_fused(X, u0, mu1, mu2, dt, nsteps, plan, proj, E, newton_tol, newton_itmax, dev))
    c = _setup(X, u0, mu1, mu2, dt, E, device)
    Phid, Hd = _as_dev(Phi, c.device), _as_dev(np.ascontiguousarray(H) if isinstance(H, np.ndarray) else H, c.device)
    n = Phid.shape[1]
    kk = n * (n + 1) // 2
    if Hd.shape != (c.N, kk) or Phid.shape[0] != c.N:
        raise ValueError("Phi must be (N, n) and H (N, n(n+1)/2)")
    _, _, idx, fac = sym_index_tables(n, c.device)
    # H3[i, a, b] = H[i, pair(a, b)] * (1 + delta_ab):  tangent = Phi + H3 . q   (:1120-1123)
    H3 = (Hd[:, idx] * fac).reshape(c.N * n, n).contiguous()

    decode = _quad_decoder(Phid, Hd, c.B)
    H3t = H3.t().contiguous()
    Phi_flat = Phid.reshape(1, c.N * n)
    per = int(c.L.bg_rom_frag_elems(c.N, n))
    Wf = torch.zeros((c.B, per), dtype=torch.float64, device=c.device) if per > 0 else None
    if Wf is not None:                                   # zero-padded operands of bg_quad_tangent
        NP = int(c.L.bg_rom_frag_pad(n))
        H3p = torch.nn.functional.pad(H3.reshape(c.N, n, n), (0, NP - n)).contiguous()
        qpad = torch.zeros((c.B, NP), dtype=torch.float64, device=c.device)

    def step(m, Un, st, Ar, br, _, G):
        q = (Un @ Phid).contiguous()                         # first guess            (:1129)
        u = decode(q).contiguous()
        while True:
            if Wf is not None:                               # fused HIP tangent -> fragment-major W -> MFMA reduce
                if NP != n:
                    qpad[:, :n] = q                          # (n = 40 needs no padding: q itself is the operand)
                with torch.cuda.device(c.device):
                    _lib.check(c.L.bg_quad_tangent(c.N, c.B, n, _lib.ptr(Phid), _lib.ptr(H3p), _lib.ptr(qpad if NP != n else q),
                                                   _lib.ptr(st.active), _lib.ptr(Wf), c.stream()), "bg_quad_tangent")
                _reduce_call(c, "bg_rom_reduce_frag", n, proj, (_lib.ptr(Wf), _lib.ptr(u)), G, c.mesh_opt, st.active, Ar, br, None)
            else:                                            # sizes beyond the fused kernels: library GEMM
                T = torch.addmm(Phi_flat, q, H3t).reshape(c.B, c.N, n)
                rom_reduce(c, T, u, G, proj, False, st.active, Ar, br, None)
            left = st.solve_update(2, Ar, br, None, q, newton_tol, newton_itmax)     # q += dq (:1161-1169)
            u = decode(q).contiguous()                       # inactive samples keep their q, hence their u
            if left == 0:
                return u

    return _host_loop(c, nsteps, n, step)                    # HIT_CAP = "Newton did not converge" (:1171)


# ----------------------------------------------------------------------- POD-ANN
def _mlp_layers(model):
    """Recognise a plain MLP: nn.Sequential of Linear / ELU|ReLU|Tanh, or the reference's POD_ANN
    class (fc1..fcK + self.elu, POD-ANN/pod_ann.py:38-56).  Returns [(Linear, act-or-None)] or None."""
    acts = (nn.ELU, nn.ReLU, nn.Tanh)
    if isinstance(model, nn.Sequential):
        mods = list(model)
        out, i = [], 0
        while i < len(mods):
            if not isinstance(mods[i], nn.Linear):
                return None
            act = None
            if i + 1 < len(mods) and isinstance(mods[i + 1], acts):
                act = mods[i + 1]; i += 1
            out.append((mods[i - (1 if act is not None else 0)], act))
            i += 1
        return out if out else None
    fcs = []
    while isinstance(getattr(model, f"fc{len(fcs) + 1}", None), nn.Linear):
        fcs.append(getattr(model, f"fc{len(fcs) + 1}"))
    elu = getattr(model, "elu", None)
    if len(fcs) >= 2 and isinstance(elu, nn.ELU):
        return [(fc, elu if i < len(fcs) - 1 else None) for i, fc in enumerate(fcs)]
    return None


def _mlp_forward_jacobian(layers, x, want_jac=True):
    """Forward pass and forward-mode input-Jacobian of a recognised MLP as batched GEMMs."""
    J = None
    for lin, act in layers:
        z = torch.addmm(lin.bias, x, lin.weight.t()) if lin.bias is not None else x @ lin.weight.t()
        if want_jac:
            J = lin.weight.unsqueeze(0).expand(x.shape[0], -1, -1) if J is None else torch.matmul(lin.weight, J)
        if act is None:
            x = z
            continue
        if isinstance(act, nn.ELU):
            x = torch.nn.functional.elu(z, alpha=act.alpha)
            d = torch.where(z > 0, torch.ones_like(z), act.alpha * torch.exp(z))
        elif isinstance(act, nn.ReLU):
            x = torch.relu(z); d = (z > 0).to(z.dtype)
        else:
            x = torch.tanh(z); d = 1.0 - x * x
        if want_jac:
            J = d.unsqueeze(-1) * J
    return x, J


class AnnEvaluator:
    """model(q) and d model / d q for a batch, in the model's dtype.  A recognised MLP runs as a
    few batched GEMMs (checked against the module itself on a probe); anything else falls back
    to torch.func (vmap of jacfwd), the batched stand-in for the reference's per-sample
    torch.autograd.functional.jacobian (:1254-1275)."""

    _live = weakref.WeakSet()         # evaluators that currently own a captured graph

    def __init__(self, model, n, dtype):
        self.model, self.dtype = model, dtype
        self.layers = _mlp_layers(model)
        if self.layers is not None:
            dev = next(model.parameters()).device
            probe = torch.linspace(-1.0, 1.0, 4 * n, device=dev, dtype=dtype).reshape(4, n)
            with torch.no_grad():
                ok = torch.allclose(model(probe), _mlp_forward_jacobian(self.layers, probe, False)[0],
                                    rtol=1e-3 if dtype != torch.float32 else 1e-5, atol=1e-5)
            if not ok:
                self.layers = None

    def forward(self, q):
        with torch.no_grad():
            return self.model(q.to(self.dtype)).to(torch.float64)

    def jacobian(self, q):
        with torch.no_grad():
            x = q.to(self.dtype)
            if self.layers is not None:
                return _mlp_forward_jacobian(self.layers, x)[1].to(torch.float64)
            return ann_jacobian(self.model, x).to(torch.float64)

    # ---- value and Jacobian in one pass (recognised fp32 MLP on the device): the value and the n tangent
    # directions are the 1 + n rows of one matrix per sample, every linear layer is ONE GEMM over B (1 + n)
    # rows, every activation one bg_mlp_act_jvp launch.  Captured in a hipGraph and replayed.
    def bind(self, B, n, device, jt_out, qs_out):
        """jt_out (B, n, nbar) and qs_out (B, nbar): fp64 destinations of dN^T and N(q)."""
        self.jt_out, self.qs_out = jt_out, qs_out
        self._graph = None
        self.fused = self.layers is not None and self.dtype == torch.float32 and device.type == "cuda"
        if not self.fused:
            return
        L = _lib.load()
        self.q_in = torch.zeros((B, n), dtype=torch.float64, device=device)
        x0 = torch.zeros((B, 1 + n, n), dtype=torch.float32, device=device)
        x0[:, 1:, :] = torch.eye(n, dtype=torch.float32, device=device)
        plan = [(lin.weight.detach().t().contiguous(), None if lin.bias is None else lin.bias.detach().contiguous(),
                 _ACT_KINDS[type(act)], float(getattr(act, "alpha", 1.0))) for lin, act in self.layers]

        def run():
            x0[:, 0, :] = self.q_in                                           # fp64 -> fp32 like q.to(float32)
            x = x0
            for wt, bias, kind, alpha in plan:
                z = torch.matmul(x, wt)                                       # (B, 1+n, h): one GEMM
                with torch.cuda.device(device):
                    _lib.check(L.bg_mlp_act_jvp(B, 1 + n, wt.shape[1], _lib.ptr(z), _lib.ptr(bias),
                                                kind, alpha, _lib.stream_ptr(device)), "bg_mlp_act_jvp")
                x = z
            self.qs_out.copy_(x[:, 0, :])
            self.jt_out.copy_(x[:, 1:, :])

        self._run = run
        self._device = device
        import os
        if os.environ.get("BG_ANN_GRAPH", "1") == "0":        # eager launches: the capture is an optimisation only
            return
        # Graph lifetime is explicit ("AnnEvaluator graph lifetime"): no captured graph of an OLDER
        # evaluator is alive -- or still replaying -- while a new capture runs, and none is left to the garbage
        # collector, which may run at any point, also inside someone else's capture.
        for other in list(AnnEvaluator._live):
            if other is not self:
                other.release()
        try:
            side = torch.cuda.Stream(device=device)
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side):                      # warm-up outside capture (lazy inits, GEMM selection)
                run(); run()
            torch.cuda.current_stream(device).wait_stream(side)
            torch.cuda.synchronize(device)
            g = torch.cuda.CUDAGraph()
            import gc
            was_enabled = gc.isenabled()
            gc.disable()           # no finaliser (of anything holding device memory or a graph) runs inside the capture
            try:
                with torch.cuda.graph(g):
                    run()
            finally:
                if was_enabled:
                    gc.enable()
            self._graph = g
            AnnEvaluator._live.add(self)
        except Exception:                                      # capture is an optimisation only
            self._graph = None

    def release(self):
        """Destroy the captured graph NOW: after the device has finished every replay of it, outside any capture --
        not whenever the collector gets to it."""
        if getattr(self, "_graph", None) is not None:
            torch.cuda.synchronize(self._device)
            self._graph = None
        AnnEvaluator._live.discard(self)

    def eval(self, q):
        """N(q) into qs_out and (dN/dq)^T into jt_out for the batch q (B, n), float64 in and out."""
        if not self.fused:
            self.qs_out.copy_(self.forward(q))
            self.jt_out.copy_(self.jacobian(q).transpose(1, 2))
            return
        self.q_in.copy_(q)
        if self._graph is not None:
            self._graph.replay()
        else:
            self._run()


def ann_jacobian(model, q32):
    """Batched input-Jacobian (B, nbar, n) of ``model`` in fp32; forward mode, since n << nbar.
    Stand-in for the per-sample torch.autograd.functional.jacobian of :1254-1275."""
    from torch.func import jacfwd, vmap
    return vmap(jacfwd(lambda z: model(z.unsqueeze(0)).squeeze(0)))(q32)


class _ClosureTangent:
    """(U_p + U_s dN)^T for a batch, as ONE GEMM: [dN^T | I] (B n x (nbar+n)) . [U_s^T ; U_p^T] ((nbar+n) x N).
    The output is the column-major per-sample tangent bg_rom_reduce reads with BG_OPT_W_COLMAJOR; the batch of
    B small (N x nbar) . (nbar x n) GEMMs it replaces ran at 2 TFLOP/s.  reference: :1224, :1361."""

    def __init__(self, Up, Us, B):
        n, self.nbar = Up.shape[1], Us.shape[1]
        self.rhs = torch.cat([Us.t(), Up.t()], 0).contiguous()              # (nbar + n, N)
        self.lhs = torch.zeros((B, n, self.nbar + n), dtype=torch.float64, device=Up.device)
        self.lhs[:, :, self.nbar:] = torch.eye(n, dtype=torch.float64, device=Up.device)

    @property
    def jt(self):
        """The (B, n, nbar) slot for dN^T."""
        return self.lhs[:, :, :self.nbar]

    def gemm(self):
        return torch.matmul(self.lhs, self.rhs)

    def __call__(self, dN):
        """dN: (B, nbar, n) -> (B, n, N)."""
        self.jt.copy_(dN.transpose(1, 2))
        return self.gemm()


def _ann_fused_plan(model, n, nbar, N, dtype, device, limits="bg_ann_rom_limits"):
    """The closure as bg_ann_rom_run and bg_ann_rom_run_wide want it (``args``: its part of the argument list; ``keep``:
    the device copies those pointers refer to), or None when the device-side loop does not apply (not a plain fp32 MLP
    the evaluator recognises, or beyond ``limits``, the entry point's own ``*_limits`` symbol)."""
    if dtype != torch.float32 or N > 512:
        return None
    layers = _ann_model_layers(model, n, nbar, limits)
    return None if layers is None else _ann_model_pack(layers, device)


def _ann_model_layers(model, n, nbar, limits, count=4):
    """The [(Linear, activation)] of a float32 ``model`` the evaluator recognises as a plain MLP (n) -> (nbar) inside the
    first four of the ``count`` ints of the ``limits`` symbol (n, nbar, width, layers), or None.  Touches no device but
    the model's own."""
    ann = AnnEvaluator(model, n, torch.float32)
    if ann.layers is None:
        return None
    max_n, max_nbar, max_w, max_l = _lib.limits(limits, count)[:4]
    widths = [ann.layers[0][0].in_features] + [lin.out_features for lin, _ in ann.layers]
    if (n > max_n or nbar > max_nbar or len(ann.layers) > max_l or max(widths[1:]) > max_w or widths[0] != n
            or widths[-1] != nbar or any(type(act) not in _ACT_KINDS for _, act in ann.layers)):
        return None
    return ann.layers


def _ann_model_pack(layers, device):
    """``args`` and ``keep`` of _ann_fused_plan for the layers _ann_model_layers returned, packed on ``device``."""
    import ctypes
    widths = [layers[0][0].in_features] + [lin.out_features for lin, _ in layers]
    f32 = dict(dtype=torch.float32, device=device)
    # W^T zero-padded to [in rounded up to 4][out rounded up to 8]: a thread fetches the weights of 8 outputs of one input
    # as two 16-byte loads, four inputs at a time, with no bounds checks in the kernel
    wts = [torch.nn.functional.pad(lin.weight.detach().to(**f32).t(), (0, -lin.out_features % 8, 0, -lin.in_features % 4)).contiguous()
           for lin, _ in layers]
    biases = [None if lin.bias is None else lin.bias.detach().to(**f32).contiguous() for lin, _ in layers]
    nl = len(wts)
    return SimpleNamespace(keep=(wts, biases), args=(
        nl, (ctypes.c_int * (nl + 1))(*widths),
        (ctypes.c_void_p * nl)(*[w.data_ptr() for w in wts]),
        (ctypes.c_void_p * nl)(*[None if b is None else b.data_ptr() for b in biases]),
        (ctypes.c_int * nl)(*[_ACT_KINDS[type(act)] for _, act in layers]),
        (ctypes.c_float * nl)(*[float(getattr(act, "alpha", 1.0)) for _, act in layers])))


def _ann_device_loop(route, limits, ut_rows, X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, proj, E, tol, max_it, device,
                     options, plan, balance):
    """What pod_ann_run_fused (bg_ann_rom_run) and pod_ann_run_wide (bg_ann_rom_run_wide) share: the basis checks, the
    plan, UT = [U_p^T; U_s^T] in the entry point's layout (``ut_rows(n, nbar, N)``: its shape), the launch, the result.
    Returns None when the model is outside ``limits``."""
    device = _lib.require_device(device)
    Xh = check_mesh(X)
    N = len(Xh)
    Up, Us = _as_dev(U_p, device), _as_dev(U_s, device)
    if Up.dim() != 2 or Us.dim() != 2 or Up.shape[0] != N or Us.shape[0] != N:
        raise ValueError("U_p and U_s must have one row per mesh node")
    n, nbar = Up.shape[1], Us.shape[1]
    if plan is None:
        plan = _ann_fused_plan(model.to(device=device, dtype=torch.float32).eval(), n, nbar, N, torch.float32, device, limits)
    if plan is None:
        return None
    UT = torch.zeros(ut_rows(n, nbar, N), dtype=torch.float64, device=device)
    UT[:n, :N] = Up.t()
    UT[n:n + nbar, :N] = Us.t()
    return _device_loop(route, Xh, u0, mu1, mu2, nsteps, device, options, balance,
                        lambda f, N, B, x, inputs, opts, outputs: f(
                            N, B, n, nbar, int(nsteps), proj, x, _lib.ptr(UT), *inputs, *plan.args, float(dt), float(E),
                            float(tol), int(max_it), opts, *outputs), keep=(plan, UT))


def pod_ann_run_fused(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, proj, E=0.0, tol=1e-6, max_it=50, device=None,
                      options=0, plan=None, balance=True):
    """``pod_ann_prom`` for a batch with the whole time loop on the device (bg_ann_rom_run): one workgroup per sample,
    the closure MLP evaluated in-kernel in float32, the reduced solve with partial pivoting.  Returns None when the model
    is outside what that kernel covers.  ``plan``: an _ann_fused_plan of the model to reuse across calls."""
    return _ann_device_loop(_ROUTES["bg_ann_rom_run"], "bg_ann_rom_limits",
                            lambda n, nbar, N: (-(-(n + nbar) // 8) * 8, N),       # zero rows up to a multiple of 8
                            X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, proj, E, tol, max_it, device, options, plan, balance)


def pod_ann_run_wide(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, proj, E=0.0, tol=1e-6, max_it=50, device=None,
                     options=0, plan=None, balance=True):
    """pod_ann_run_fused for models of up to 20 primary modes (bg_ann_rom_run_wide): the closure MLP of bg_ann_rom_run on
    the mesh side of bg_rbf_rom_run.  Runs any model inside bg_ann_rom_run_wide_limits, the n <= 8 ones included; returns
    None outside them.  ``plan``: an _ann_fused_plan(..., limits="bg_ann_rom_run_wide_limits") to reuse across calls."""
    return _ann_device_loop(_ROUTES["bg_ann_rom_run_wide"], "bg_ann_rom_run_wide_limits",
                            lambda n, nbar, N: (n + nbar, 512),                    # zero columns from N
                            X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, proj, E, tol, max_it, device, options, plan, balance)


class _HyperClosurePlan:
    """What HyperAnnPlan and HyperRbfPlan share: the checks of bases, mesh and sampling on the host, and the table of the
    sorted distinct stencil nodes of the sampled rows on the device (include/burgers_hip.h, bg_hyper_ann_rom_run)."""

    def _check_sizes(self, route, U_p, U_s, sampling, X, max_n, max_nbar, max_m):
        """Bases, mesh and sampling against each other and the limits; returns the host copies (Up, Us, Xh, rows, xi)."""
        Up, Us = _host64(U_p), _host64(U_s)
        if Up.ndim != 2 or Us.ndim != 2 or Up.shape[0] != Us.shape[0] or Up.shape[1] < 1 or Us.shape[1] < 1:
            raise ValueError("U_p and U_s must be (N, n) and (N, nbar)")
        N, n, nbar = Up.shape[0], Up.shape[1], Us.shape[1]
        Xh = check_mesh(X)
        if N < route.min_n or N > _limit(route.max_n) or len(Xh) != N:
            raise ValueError(f"{route.entry} covers {route.min_n} <= N <= {_limit(route.max_n)} with one row of U_p and U_s per mesh node")
        if n > max_n or nbar > max_nbar:
            raise ValueError(f"{route.entry} covers n <= {max_n} and nbar <= {max_nbar} (got {n}, {nbar})")
        rows, xi = _sampling_rows(route, sampling, N, max_m)
        return Up, Us, Xh, rows, xi

    def _pack_table(self, route, Up, Us, Xh, rows, xi, sampling, max_nodes, device, workgroups_per_cu, ut_shape):
        """The remaining refusals (orthonormal bases, the table's size, the sampling's projection), then the device: the
        table, ``wg_per_cu`` from ``workgroups_per_cu(nodes)`` and UTn of shape ``ut_shape(nodes)``, zero outside
        [n + nbar][nodes].  Returns the device."""
        N, n, nbar = Up.shape[0], Up.shape[1], Us.shape[1]
        U = np.concatenate([Up, Us], axis=1)
        _require_orthonormal(U, "[U_p U_s]", "U_p^T u^n")
        nodes = _stencil_nodes(route, rows, N, max_nodes)
        self.projection = _projection(str(sampling.projection), _SAMPLING_PROJECTION)
        device = _lib.require_device(device)
        self.N, self.n, self.nbar = N, n, nbar
        self.wg_per_cu = workgroups_per_cu(len(nodes))
        self.Up, self.Us = _as_dev(Up, device), _as_dev(Us, device)
        _put_table(self, nodes, rows, xi, sampling, Xh, device)
        UTn = np.zeros(ut_shape(len(nodes)))
        UTn[:n + nbar, :len(nodes)] = U[nodes].T
        self.UTn = _as_dev(UTn, device)
        return device

    def _build_ann(self, entry, limits, U_p, U_s, model, sampling, X, device, workgroups_per_cu, ut_shape):
        """HyperAnnPlan and HyperAnnWidePlan: the checks against the six ``limits`` of ``entry``, the model, the table and the
        packed closure.  ``workgroups_per_cu(L, nodes)``, ``ut_shape(L, n + nbar, nodes)``: the entry point's own."""
        route = _ROUTES[entry]
        max_n, max_nbar, max_w, max_l, max_m, max_nodes = _lib.limits(limits, 6)
        Up, Us, Xh, rows, xi = self._check_sizes(route, U_p, U_s, sampling, X, max_n, max_nbar, max_m)
        n, nbar = Up.shape[1], Us.shape[1]
        if not isinstance(model, nn.Module) or any(p.dtype != torch.float32 for p in model.parameters()):
            raise ValueError("the closure must be a plain float32 MLP (torch.nn.Module)")
        layers = _ann_model_layers(model, n, nbar, limits, 6)
        if layers is None:
            raise ValueError(f"the closure must be a plain float32 MLP ({n}) -> ({nbar}) of Linear / ELU / ReLU / Tanh layers with "
                             f"widths <= {max_w} and at most {max_l} layers")
        device = self._pack_table(route, Up, Us, Xh, rows, xi, sampling, max_nodes, device,
                                  lambda k: workgroups_per_cu(_lib.load(), k), lambda k: ut_shape(_lib.load(), n + nbar, k))
        self.model = _ann_model_pack(layers, device)


class HyperAnnPlan(_HyperClosurePlan):
    """What bg_hyper_ann_rom_run reads besides the batch, built once per bases, closure, sampling and mesh
    (include/burgers_hip.h): the table of the sorted distinct stencil nodes of the sampled rows (``nodes``, at most 3 m),
    their coordinates ``xn``, the table position ``pos`` of every sampled row, the weights ``xi``, UTn = [U_p^T; U_s^T]
    restricted to the table nodes, and the packed closure.  ``sampling``: a pod.RowSampling (pod.build_ann_row_sampling);
    ``model``: a plain float32 MLP.  Everything the shapes, the sampling, the model and the bases decide is refused with a
    ValueError before the device is touched -- also bases with |[U_p U_s]^T [U_p U_s] - I|_max > 1e-8: the loop carries q_p
    from step to step instead of re-projecting U_p^T u^n, which is exact only for orthonormal bases."""

    def __init__(self, U_p, U_s, model, sampling, X, device):
        self._build_ann("bg_hyper_ann_rom_run", "bg_hyper_ann_rom_limits", U_p, U_s, model, sampling, X, device,
                        lambda L, k: L.bg_hyper_ann_rom_workgroups_per_cu(k),
                        lambda L, rows, k: (-(-rows // 8) * 8, k))


class HyperAnnWidePlan(_HyperClosurePlan):
    """What bg_hyper_ann_rom_run_wide reads besides the batch: a HyperAnnPlan against the wide loop's limits (n <= 20,
    bg_hyper_ann_rom_wide_limits) with UTn in its layout, [n + nbar] rows of the stride bg_hyper_ann_rom_wide_ut_ld gives, zero
    from ``nodes``.  Takes any model inside those limits, the n <= 8 ones included.  The refusals are HyperAnnPlan's, each a
    ValueError before the device is touched."""

    def __init__(self, U_p, U_s, model, sampling, X, device):
        self._build_ann("bg_hyper_ann_rom_run_wide", "bg_hyper_ann_rom_wide_limits", U_p, U_s, model, sampling, X, device,
                        lambda L, k: L.bg_hyper_ann_rom_wide_workgroups_per_cu(k),
                        lambda L, rows, k: (rows, L.bg_hyper_ann_rom_wide_ut_ld(k)))


class HyperClosureRomResult(_HyperResult):
    """Result of pod_ann_run_hyper and pod_rbf_run_hyper (_HyperResult): ``q`` holds the primary coordinates (column 0:
    U_p^T u0) and ``q_s`` (B, nT+1, nbar) the closure values of every step's decode (column 0: zeros, no closure value belongs
    to u0).  The decode is U = U_p q + U_s q_s as one batched product -- the kernel's own decode, not a second evaluation of
    the closure."""

    def __init__(self, res, plan, u0d, q_s):
        super().__init__(res, plan, u0d)
        self.q_s = q_s

    def _decode(self):
        return torch.matmul(torch.cat([self.q, self.q_s], dim=2), torch.cat([self.plan.Up, self.plan.Us], dim=1).t())


HyperAnnRomResult = HyperClosureRomResult        # the name pod_ann_run_hyper's result has had
HyperRbfRomResult = HyperClosureRomResult


def _project_rows(u, P, chunk=256):
    """u (B, N) times P (N, n), every ``chunk`` rows as one product-and-sum of one fixed shape (the last chunk padded with
    zero rows): a row's result does not depend on the batch around it, which a GEMM over the whole batch does not promise."""
    B, N = u.shape
    out = torch.empty((B, P.shape[1]), dtype=u.dtype, device=u.device)
    for b0 in range(0, B, chunk):
        rows = u[b0:b0 + chunk]
        if rows.shape[0] < chunk:
            rows = torch.cat([rows, rows.new_zeros((chunk - rows.shape[0], N))])
        out[b0:b0 + chunk] = (rows[:, :, None] * P[None]).sum(dim=1)[:min(chunk, B - b0)]
    return out


def pod_ann_run_hyper(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, sampling_or_plan, proj, E=0.0, tol=1e-6, max_it=50,
                      device=None, options=0, balance=True):
    """``pod_ann_prom`` HYPER-REDUCED, with the whole time loop on the device (bg_hyper_ann_rom_run): both projections are
    assembled from the sampled mesh rows of a pod.RowSampling (pod.build_ann_row_sampling) with their weights, on the table
    of their stencil nodes, so an iteration costs the same whatever the mesh: N up to bg_fom_max_n(), n <= 8, m <= 256
    (bg_hyper_ann_rom_limits).  q_p carries over from step to step (no U_p^T u^n: the bases must be orthonormal).
    ``sampling_or_plan``: the sampling, or a HyperAnnPlan of these bases, closure, sampling and mesh to reuse across calls
    (``res.plan``; ``U_p``, ``U_s`` and ``model`` are then not looked at).  A sampling trained for the other projection is
    refused.  Nothing is synchronised.  Returns a HyperAnnRomResult.
    A HyperAnnWidePlan, or a sampling with a model of more than bg_hyper_ann_rom_limits' n primary modes inside
    bg_hyper_ann_rom_wide_limits (n <= 20), goes to the wide loop (pod_ann_run_hyper_wide)."""
    if isinstance(sampling_or_plan, HyperAnnWidePlan) or (
            not isinstance(sampling_or_plan, HyperAnnPlan) and len(np.shape(U_p)) == 2
            and _lib.limits("bg_hyper_ann_rom_limits", 6)[0] < np.shape(U_p)[1] <= _lib.limits("bg_hyper_ann_rom_wide_limits", 6)[0]):
        return pod_ann_run_hyper_wide(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, sampling_or_plan, proj, E, tol, max_it, device,
                                      options, balance)
    Xh = check_mesh(X)
    plan = sampling_or_plan if isinstance(sampling_or_plan, HyperAnnPlan) else HyperAnnPlan(U_p, U_s, model, sampling_or_plan, Xh, device)
    return _hyper_closure_run(_ROUTES["bg_hyper_ann_rom_run"], plan, Xh, u0, mu1, mu2, nsteps, proj, device, options, balance,
                              lambda N, B, nsteps, proj, q0, u0n, inputs: (
                                  N, B, plan.n, plan.nbar, plan.m, plan.n_nodes, nsteps, proj, _lib.ptr(plan.node), _lib.ptr(plan.xn),
                                  _lib.ptr(plan.pos), _lib.ptr(plan.xi), _lib.ptr(plan.UTn), q0, u0n, *inputs[1:], *plan.model.args,
                                  float(dt), float(E), float(tol), int(max_it)))


def pod_ann_run_hyper_wide(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, sampling_or_plan, proj, E=0.0, tol=1e-6, max_it=50,
                           device=None, options=0, balance=True):
    """pod_ann_run_hyper for models of up to 20 primary modes (bg_hyper_ann_rom_run_wide, bg_hyper_ann_rom_wide_limits): the
    loop of bg_ann_rom_run_wide on the table of the sampled rows' stencil nodes.  Runs any model inside those limits, the
    n <= 8 ones included; what it does not cover is a ValueError.  ``sampling_or_plan``: the sampling, or a HyperAnnWidePlan to
    reuse across calls (``res.plan``).  Nothing is synchronised.  Returns a HyperClosureRomResult."""
    Xh = check_mesh(X)
    if isinstance(sampling_or_plan, HyperAnnPlan):
        raise ValueError("bg_hyper_ann_rom_run_wide takes a HyperAnnWidePlan")
    plan = (sampling_or_plan if isinstance(sampling_or_plan, HyperAnnWidePlan)
            else HyperAnnWidePlan(U_p, U_s, model, sampling_or_plan, Xh, device))
    return _hyper_closure_run(_ROUTES["bg_hyper_ann_rom_run_wide"], plan, Xh, u0, mu1, mu2, nsteps, proj, device, options, balance,
                              lambda N, B, nsteps, proj, q0, u0n, inputs: (
                                  N, B, plan.n, plan.nbar, plan.m, plan.n_nodes, nsteps, proj, _lib.ptr(plan.node), _lib.ptr(plan.xn),
                                  _lib.ptr(plan.pos), _lib.ptr(plan.xi), _lib.ptr(plan.UTn), q0, u0n, *inputs[1:], *plan.model.args,
                                  float(dt), float(E), float(tol), int(max_it)))


def _hyper_closure_run(route, plan, Xh, u0, mu1, mu2, nsteps, proj, device, options, balance, head):
    """What pod_ann_run_hyper and pod_rbf_run_hyper share: the plan against the call (device, mesh, projection), q0 and u0
    at the table nodes, the launch through _device_loop and the result.  ``head(N, B, nsteps, proj, q0, u0n, inputs)``: the
    entry point's argument list up to max_it; options, qhist, qshist and the other outputs follow it."""
    device = _check_hyper_call(plan, Xh, device, proj)
    u0d, mu1d, _ = _batch_inputs(u0, mu1, mu2, plan.N, device)
    q0 = _project_rows(u0d, plan.Up)
    u0n = u0d[:, plan.nodes].contiguous()
    q_s = torch.empty((mu1d.numel(), nsteps + 1, plan.nbar), dtype=torch.float64, device=device)
    res = _device_loop(route, Xh, u0d, mu1, mu2, nsteps, device, options, balance,
                       lambda f, N, B, x, inputs, opts, outputs: f(
                           *head(N, B, int(nsteps), proj, _lib.ptr(q0), _lib.ptr(u0n), inputs), opts, outputs[0], _lib.ptr(q_s),
                           *outputs[1:]), keep=(plan, q0, u0n, q_s), slots=plan.wg_per_cu * _cu_count(device), cols=plan.n)
    return HyperClosureRomResult(res, plan, u0d, q_s)


def _ann_route(n, fused=True, wide=False):
    """The device-side loops pod_ann_run tries, in order: bg_ann_rom_run_wide first only for an opted-in model with more
    primary modes than bg_ann_rom_run takes."""
    if not fused:
        return ()
    return (("bg_ann_rom_run_wide",) if wide and n > _lib.limits("bg_ann_rom_limits", 4)[0] else ()) + ("bg_ann_rom_run",)


def pod_ann_run(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, projection="LSPG", E=0.0, tol=1e-6, max_it=50,
                device=None, ann_dtype=torch.float32, fused=True, wide=False, hyper=None):
    """Batched ``pod_ann_prom``.  The MLP and its Jacobian are evaluated in ``ann_dtype`` (the
    reference uses float32, :1219,:1241); everything else is fp64.  ``fused`` (default): the device-side time loop
    bg_ann_rom_run when the closure is a plain float32 MLP within bg_ann_rom_limits; otherwise, or with
    ``fused=False``, the batched iteration driven from the host (MLP layers as GEMMs through PyTorch-ROCm).
    ``wide`` (opt-in, with ``fused`` and float32): a model with more primary modes than bg_ann_rom_limits allows that is
    inside bg_ann_rom_run_wide_limits (n <= 20) takes the device-side loop bg_ann_rom_run_wide instead of the host-driven
    iteration; every other model routes as without the flag.
    ``hyper`` (opt-in): a pod.RowSampling (pod.build_ann_row_sampling), a HyperAnnPlan or a HyperAnnWidePlan sends the call
    through the hyper-reduced loop pod_ann_run_hyper, which assembles both projections from the sampled mesh rows only
    (bg_hyper_ann_rom_run; a sampling with 9 <= n <= 20 primary modes and a HyperAnnWidePlan: bg_hyper_ann_rom_run_wide); models,
    bases and sizes it does not cover are refused, not rerouted."""
    proj = _projection(projection, "projection must be 'Galerkin' or 'LSPG'")
    if hyper is not None:
        if ann_dtype != torch.float32:
            raise ValueError("the hyper-reduced POD-ANN loop evaluates the closure in float32")
        return check_singular(pod_ann_run_hyper(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, hyper, proj, E, tol, max_it, device))
    if ann_dtype == torch.float32:
        for entry in _ann_route(np.shape(U_p)[1], fused, wide):
            run = pod_ann_run_wide if entry == "bg_ann_rom_run_wide" else pod_ann_run_fused
            res = run(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, proj, E, tol, max_it, device)
            if res is not None:
                return check_singular(res)
    c = _setup(X, u0, mu1, mu2, dt, E, device)
    Up, Us = _as_dev(U_p, c.device), _as_dev(U_s, c.device)
    n = Up.shape[1]
    UpT, UsT = Up.t().contiguous(), Us.t().contiguous()
    tangent = _ClosureTangent(Up, Us, c.B)
    model = model.to(device=c.device, dtype=ann_dtype).eval()
    ann = AnnEvaluator(model, n, ann_dtype)
    qs = torch.zeros((c.B, Us.shape[1]), dtype=torch.float64, device=c.device)
    ann.bind(c.B, n, c.device, tangent.jt, qs)

    def step(nt, U0, st, Ar, br, _, G):
        qp = (U0 @ Up).contiguous()                                         # (:1197)
        ann.eval(qp)                                                        # dN at the first guess (:1219)
        while True:
            rom_reduce(c, tangent.gemm(), U0, G, proj, True, st.active, Ar, br, None, colmajor=True)   # (:1224)
            left = st.solve_update(3, Ar, br, None, qp, tol, max_it)        # q_p += dq           (:1237-1244)
            ann.eval(qp)                            # q_s = N(q_p) for the decode (:1241) and dN for the next pass
            U0 = (qp @ UpT + qs @ UsT).contiguous()                         # (:1242)
            if left == 0:
                return U0

    try:
        return _host_loop(c, nsteps, n, step)
    finally:
        ann.release()               # also on an exception (SingularReducedSystem): never leave the graph to the collector


# ----------------------------------------------------------------------- POD-RBF
class RbfClosure:
    """Scaled RBF closure q_s = unscale(k(|x - x_i|) @ W), x = scale(q_p), and its full-chain Jacobian, batched
    over samples (FEM/fem_burgers.py:160-260).  bg_rbf_eval produces the kernel values phi (B, Ns) and the
    gradient factors d phi / d q_p already transposed, GT (B, n, Ns), in one pass; value and Jacobian are then
    ONE GEMM each against the output-scaled weights: q_s = phi Wd + (dy/2 + y_min), (dq_s/dq_p)^T = GT Wd."""

    def __init__(self, X_train, W, eps, kernel, x_min, x_max, y_min, y_max, device):
        self.kind = _pod._rbf_kind(kernel)                             # refuses an unknown name
        f = lambda a: _as_dev(np.asarray(a, dtype=np.float64), device)
        self.L = _lib.load()
        self.device = device
        Xt, Wm = f(X_train), f(W)
        self.eps = float(eps)
        self.x_min, y_min = f(x_min), f(y_min)
        self.dx, dy = _pod._rbf_range(self.x_min, f(x_max)), _pod._rbf_range(y_min, f(y_max))
        if Wm.shape != (Xt.shape[0], dy.numel()) or Xt.shape[1] != self.dx.numel():
            raise ValueError("X_train must be (Ns, n) and W (Ns, nbar)")
        self.Ns, self.n = Xt.shape
        self.XtT = Xt.t().contiguous()                                 # (n, Ns): centre index fastest
        self.Wd = (Wm * (0.5 * dy)).contiguous()                       # output scaling folded into the weights
        self.bias = (0.5 * dy + y_min).contiguous()
        self._buf = {}

    def _eval(self, qp, want_gt):
        B = qp.shape[0]
        if B not in self._buf:
            f64 = dict(dtype=torch.float64, device=self.device)
            self._buf[B] = (torch.empty((B, self.Ns), **f64), torch.empty((B, self.n, self.Ns), **f64))
        phi, GT = self._buf[B]
        qp = qp.contiguous()
        with torch.cuda.device(self.device):
            rc = self.L.bg_rbf_eval(B, self.n, self.Ns, self.kind, self.eps, _lib.ptr(qp), _lib.ptr(self.x_min),
                                    _lib.ptr(self.dx), _lib.ptr(self.XtT), _lib.ptr(phi),
                                    _lib.ptr(GT) if want_gt else None, _lib.stream_ptr(self.device))
        _lib.check(rc, "bg_rbf_eval")
        return phi, GT

    def value(self, qp):
        phi, _ = self._eval(qp, False)
        return torch.addmm(self.bias, phi, self.Wd)                    # (B, nbar)

    def jacobian_t(self, qp):
        _, GT = self._eval(qp, True)
        return torch.matmul(GT, self.Wd)                               # (B, n, nbar): one GEMM over B n rows

    def jacobian(self, qp):
        return self.jacobian_t(qp).transpose(1, 2)                     # (B, nbar, n) view


class RbfFusedPlan:
    """The operand copies bg_rbf_rom_run reads, built once per closure and basis on the device (include/burgers_hip.h):
    UT = [U_p^T; U_s^T] with row stride 512, the centres transposed, the output-scaled weights Wd and the bias padded to
    128 columns, x_min and dx (the closure's own scaling, RbfClosure).  ``ok`` is False when the closure or the mesh is
    beyond bg_rbf_rom_limits (N > 512, n > 20, nbar > 128 or too many centres).
    ``long_mesh``: the operands of bg_rbf_rom_run_long instead, UT with row stride 1024; ``ok`` only for 513 <= N <= 1024
    within the closure limits of bg_rbf_rom_run_long_limits, and shapes that do not fit together raise ValueError before
    anything is copied to the device."""

    def __init__(self, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max, kernel, device, long_mesh=False):
        self.long_mesh = bool(long_mesh)
        if self.long_mesh:
            up, us, xt, w = (tuple(np.shape(a)) for a in (U_p, U_s, X_train, W))
            if len(up) != 2 or len(us) != 2 or up[0] != us[0]:
                raise ValueError("U_p and U_s must be (N, n) and (N, nbar)")
            if len(xt) != 2 or len(w) != 2 or xt[1] != up[1] or w != (xt[0], us[1]):
                raise ValueError("X_train must be (Ns, n) and W (Ns, nbar) for the n, nbar of U_p, U_s")
            for name, v, k in (("x_min", x_min, up[1]), ("x_max", x_max, up[1]), ("y_min", y_min, us[1]), ("y_max", y_max, us[1])):
                if tuple(np.shape(v)) != (k,):
                    raise ValueError(f"{name} must have {k} entries")
            device = _lib.require_device(device)
        self.Up, self.Us = _as_dev(U_p, device), _as_dev(U_s, device)
        if self.Up.dim() != 2 or self.Us.dim() != 2 or self.Up.shape[0] != self.Us.shape[0]:
            raise ValueError("U_p and U_s must be (N, n) and (N, nbar)")
        self.N, self.n = self.Up.shape
        self.nbar = self.Us.shape[1]
        rbf = RbfClosure(X_train, W, epsilon, kernel, x_min, x_max, y_min, y_max, device)
        if rbf.n != self.n or rbf.Wd.shape[1] != self.nbar:
            raise ValueError("X_train must be (Ns, n) and W (Ns, nbar) for the n, nbar of U_p, U_s")
        self.Ns, self.kind, self.eps = rbf.Ns, rbf.kind, rbf.eps
        if self.long_mesh:
            ld, max_n, max_nbar, max_ns = _lib.limits("bg_rbf_rom_run_long_limits", 4)
            self.ok = 512 < self.N <= ld and self.n <= max_n and self.nbar <= max_nbar and self.Ns <= max_ns
        else:
            ld = 512
            max_n, max_nbar, max_ns = _lib.limits("bg_rbf_rom_limits", 3)
            self.ok = self.N <= 512 and self.n <= max_n and self.nbar <= max_nbar and self.Ns <= max_ns
        if not self.ok:
            return
        f64 = dict(dtype=torch.float64, device=device)
        self.UT = torch.zeros((self.n + self.nbar, ld), **f64)
        self.UT[:self.n, :self.N] = self.Up.t()
        self.UT[self.n:, :self.N] = self.Us.t()
        self.XtT, self.x_min, self.dx = rbf.XtT, rbf.x_min.contiguous(), rbf.dx.contiguous()
        self.Wd = torch.zeros((self.Ns, 128), **f64)
        self.Wd[:, :self.nbar] = rbf.Wd
        self.bias = torch.zeros((128,), **f64)
        self.bias[:self.nbar] = rbf.bias


def _rbf_device_loop(route, X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max,
                     projection, kernel, E, tol_newton, max_newton, device, plan, balance, options):
    """What pod_rbf_run_fused (bg_rbf_rom_run) and pod_rbf_run_long (bg_rbf_rom_run_long) share: the plan and its checks,
    the launch, the result.  Returns None when the plan's closure or mesh is outside what the entry point covers."""
    proj = _projection(projection, "projection must be 'LSPG' or 'Galerkin'.")
    long_mesh = route.entry == "bg_rbf_rom_run_long"
    device = _lib.require_device(device)
    Xh = check_mesh(X)
    if plan is None:
        plan = (RbfFusedPlan(U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max, kernel, device, long_mesh=True)
                if long_mesh else RbfFusedPlan(U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max, kernel, device))
    Up = U_p if isinstance(U_p, torch.Tensor) else np.asarray(U_p)
    if (plan.N != len(Xh) or tuple(Up.shape) != (plan.N, plan.n) or plan.Up.device != device
            or plan.long_mesh != long_mesh):
        raise ValueError("the plan must be built for this mesh, U_p and entry point (and live on the device of the call)")
    if not plan.ok:
        return None
    res = _device_loop(route, Xh, u0, mu1, mu2, nsteps, device, options, balance,
                       lambda f, N, B, x, inputs, opts, outputs: f(
                           N, B, plan.n, plan.nbar, plan.Ns, int(nsteps), proj, plan.kind, x, _lib.ptr(plan.UT),
                           _lib.ptr(plan.XtT), _lib.ptr(plan.Wd), _lib.ptr(plan.bias), _lib.ptr(plan.x_min),
                           _lib.ptr(plan.dx), float(plan.eps), *inputs, float(dt), float(E), float(tol_newton),
                           int(max_newton), opts, *outputs), keep=(plan,))
    res.plan = plan
    return res


def pod_rbf_run_fused(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max,
                      projection="LSPG", kernel="gaussian", E=0.0, tol_newton=1e-6, max_newton=30, device=None,
                      plan=None, balance=True, options=0):
    """``pod_rbf_prom`` for a batch with the whole time loop on the device (bg_rbf_rom_run): one workgroup per sample,
    the closure evaluated in-kernel in fp64, the reduced solve with partial pivoting.  Returns None when the closure is
    outside bg_rbf_rom_limits.  ``plan``: an RbfFusedPlan of the same closure and basis to reuse across calls
    (``res.plan``); the closure arguments are then not read again, U_p only for its shape."""
    return _rbf_device_loop(_ROUTES["bg_rbf_rom_run"], X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon, x_min,
                            x_max, y_min, y_max, projection, kernel, E, tol_newton, max_newton, device, plan, balance, options)


def pod_rbf_run_long(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max,
                     projection="LSPG", kernel="gaussian", E=0.0, tol_newton=1e-6, max_newton=30, device=None,
                     plan=None, balance=True, options=0):
    """pod_rbf_run_fused for meshes of 513 <= N <= 1024 nodes (bg_rbf_rom_run_long): the same loop on eight waves, one
    workgroup per compute unit.  Returns None when the mesh or the closure is outside bg_rbf_rom_run_long_limits.
    ``plan``: an RbfFusedPlan built with ``long_mesh=True`` (``res.plan``)."""
    return _rbf_device_loop(_ROUTES["bg_rbf_rom_run_long"], X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon,
                            x_min, x_max, y_min, y_max, projection, kernel, E, tol_newton, max_newton, device, plan, balance,
                            options)


class HyperRbfPlan(_HyperClosurePlan):
    """What bg_hyper_rbf_rom_run reads besides the batch, built once per bases, closure, sampling and mesh
    (include/burgers_hip.h): the table HyperAnnPlan holds (``nodes``, ``node``, ``pos``, ``xi``, ``xn``), UTn = [U_p^T; U_s^T]
    restricted to the table nodes with the row stride bg_hyper_rbf_rom_ut_ld gives, ``wg_per_cu`` from the library, and the
    closure operands of RbfFusedPlan: ``XtT``, ``Wd`` and ``bias`` padded to 128 columns, ``x_min``, ``dx``, ``kind``,
    ``eps``.  ``sampling``: a pod.RowSampling (pod.build_rbf_row_sampling).  Everything the shapes, the limits, the
    sampling, the kernel name and the bases decide is refused with a ValueError before the device is touched -- also bases
    with |[U_p U_s]^T [U_p U_s] - I|_max > 1e-8: the loop carries q_p over instead of re-projecting U_p^T U0, which is exact
    only for orthonormal bases."""

    def __init__(self, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max, kernel, sampling, X, device):
        route = _ROUTES["bg_hyper_rbf_rom_run"]
        max_n, max_nbar, max_ns, max_m, max_nodes = _lib.limits("bg_hyper_rbf_rom_limits", 5)
        Up, Us, Xh, rows, xi = self._check_sizes(route, U_p, U_s, sampling, X, max_n, max_nbar, max_m)
        n, nbar = Up.shape[1], Us.shape[1]
        Xt, Wm = _host64(X_train), _host64(W)
        if Xt.ndim != 2 or Wm.ndim != 2 or Xt.shape[1] != n or Wm.shape != (Xt.shape[0], nbar) or Xt.shape[0] < 1:
            raise ValueError("X_train must be (Ns, n) and W (Ns, nbar) for the n, nbar of U_p, U_s")
        scal = {}
        for name, v, k in (("x_min", x_min, n), ("x_max", x_max, n), ("y_min", y_min, nbar), ("y_max", y_max, nbar)):
            scal[name] = _host64(v)
            if scal[name].shape != (k,):
                raise ValueError(f"{name} must have {k} entries")
        if Xt.shape[0] > max_ns:
            raise ValueError(f"{route.entry} covers at most {max_ns} centres (got {Xt.shape[0]})")
        self.kind = _pod._rbf_kind(kernel)                             # refuses an unknown name
        self.Ns, self.eps = Xt.shape[0], float(epsilon)
        L = _lib.load()
        device = self._pack_table(route, Up, Us, Xh, rows, xi, sampling, max_nodes, device,
                                  L.bg_hyper_rbf_rom_workgroups_per_cu, lambda k: (n + nbar, L.bg_hyper_rbf_rom_ut_ld(k)))
        dx, dy = _pod._rbf_range(scal["x_min"], scal["x_max"]), _pod._rbf_range(scal["y_min"], scal["y_max"])
        self.XtT = _as_dev(np.ascontiguousarray(Xt.T), device)         # (n, Ns): centre index fastest
        Wd, bias = np.zeros((self.Ns, 128)), np.zeros(128)
        Wd[:, :nbar] = Wm * (0.5 * dy)                                 # output scaling folded into the weights (RbfClosure)
        bias[:nbar] = 0.5 * dy + scal["y_min"]
        self.Wd, self.bias = _as_dev(Wd, device), _as_dev(bias, device)
        self.x_min, self.dx = _as_dev(scal["x_min"], device), _as_dev(dx, device)


def pod_rbf_run_hyper(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max,
                      sampling_or_plan, proj, kernel="gaussian", E=0.0, tol_newton=1e-6, max_newton=30, device=None, options=0,
                      balance=True):
    """``pod_rbf_prom`` HYPER-REDUCED, with the whole time loop on the device (bg_hyper_rbf_rom_run): both projections are
    assembled from the sampled mesh rows of a pod.RowSampling (pod.build_rbf_row_sampling) with their weights, on the table
    of their stencil nodes, so the mesh side of an iteration costs the same whatever the mesh: N up to bg_fom_max_n(),
    n <= 20, nbar <= 128, m <= 256 (bg_hyper_rbf_rom_limits).  q_p carries over between iterations and steps (no U_p^T U0:
    the bases must be orthonormal).  ``sampling_or_plan``: the sampling, or a HyperRbfPlan of these bases, closure,
    sampling and mesh to reuse across calls (``res.plan``; the bases and the closure arguments are then not looked at).
    ``proj``: BG_PROJ_GALERKIN or BG_PROJ_LSPG (PROJ); a sampling trained for the other projection is refused.  Nothing is
    synchronised.  Returns a HyperRbfRomResult."""
    Xh = check_mesh(X)
    plan = sampling_or_plan if isinstance(sampling_or_plan, HyperRbfPlan) else HyperRbfPlan(
        U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max, kernel, sampling_or_plan, Xh, device)
    return _hyper_closure_run(_ROUTES["bg_hyper_rbf_rom_run"], plan, Xh, u0, mu1, mu2, nsteps, proj, device, options, balance,
                              lambda N, B, nsteps, proj, q0, u0n, inputs: (
                                  N, B, plan.n, plan.nbar, plan.Ns, plan.m, plan.n_nodes, nsteps, proj, plan.kind,
                                  _lib.ptr(plan.node), _lib.ptr(plan.xn), _lib.ptr(plan.pos), _lib.ptr(plan.xi), _lib.ptr(plan.UTn),
                                  _lib.ptr(plan.XtT), _lib.ptr(plan.Wd), _lib.ptr(plan.bias), _lib.ptr(plan.x_min),
                                  _lib.ptr(plan.dx), plan.eps, q0, u0n, *inputs[1:], float(dt), float(E), float(tol_newton),
                                  int(max_newton)))


def _rbf_route(N, fused=False, long_mesh=False):
    """The device loops pod_rbf_run tries for a mesh of N nodes, in this order; each is taken if the RbfFusedPlan of the
    closure for it is ``ok`` (inside its limits), and "host" is what is left."""
    if not fused:
        return ()
    return (("bg_rbf_rom_run_long",) if long_mesh and N > _ROUTES["bg_rbf_rom_run"].max_n else ()) + ("bg_rbf_rom_run",)


def pod_rbf_run(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max,
                projection="LSPG", kernel="gaussian", E=0.0, tol_newton=1e-6, max_newton=30, device=None, fused=False,
                long_mesh=False, hyper=None):
    """Batched ``pod_rbf_prom`` (FEM/fem_burgers.py:1278-1398).  Default: the batched iteration driven from the host.
    ``fused``: the device-side time loop bg_rbf_rom_run (pod_rbf_run_fused) when the closure is within bg_rbf_rom_limits,
    otherwise the host-driven iteration as well.
    ``long_mesh`` (opt-in, with ``fused``): meshes of 512 < N <= 1024 whose closure is inside bg_rbf_rom_run_long_limits
    take the device-side loop bg_rbf_rom_run_long (pod_rbf_run_long) instead of the host-driven iteration.
    ``hyper`` (opt-in): a pod.RowSampling (pod.build_rbf_row_sampling) or a HyperRbfPlan sends the call through the
    hyper-reduced loop pod_rbf_run_hyper, which assembles both projections from the sampled mesh rows only; closures, bases
    and sizes it does not cover are refused, not rerouted."""
    proj = _projection(projection, "projection must be 'LSPG' or 'Galerkin'.")
    if hyper is not None:
        return check_singular(pod_rbf_run_hyper(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min,
                                                y_max, hyper, proj, kernel, E, tol_newton, max_newton, device))
    tries = _rbf_route(np.shape(X)[0], fused, long_mesh)
    if "bg_rbf_rom_run_long" in tries:
        res = pod_rbf_run_long(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max,
                               projection, kernel, E, tol_newton, max_newton, device)
        if res is not None:
            return check_singular(res)
    if "bg_rbf_rom_run" in tries:
        res = pod_rbf_run_fused(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max,
                                projection, kernel, E, tol_newton, max_newton, device)
        if res is not None:
            return check_singular(res)
    c = _setup(X, u0, mu1, mu2, dt, E, device)
    rbf = RbfClosure(X_train, W, epsilon, kernel, x_min, x_max, y_min, y_max, c.device)
    Up, Us = _as_dev(U_p, c.device), _as_dev(U_s, c.device)
    n = Up.shape[1]
    UpT, UsT = Up.t().contiguous(), Us.t().contiguous()
    tangent = _ClosureTangent(Up, Us, c.B)
    q = torch.zeros((c.B, n), dtype=torch.float64, device=c.device)

    def step(nt, U0, st, Ar, br, _, G):
        while True:
            qp = (U0 @ Up).contiguous()                                     # q_p = U_p^T U0        (:1352)
            tangent.jt.copy_(rbf.jacobian_t(qp))
            rom_reduce(c, tangent.gemm(), U0, G, proj, True, st.active, Ar, br, None, colmajor=True)   # (:1361)
            left = st.solve_update(1, Ar, br, qp, q, tol_newton, max_newton)   # q_new = q_p + dq, err = |dq|/|q_new|
            act = st.active_before
            U1 = q @ UpT + rbf.value(q) @ UsT                               # (:1378-1381)
            U0 = torch.where(act[:, None], U1, U0).contiguous()
            if left == 0:
                return U0

    return _host_loop(c, nsteps, n, step)


# --------------------------------------------------------------------- local POD
class LocalPodPlan:
    """The operands bg_local_rom_run reads, built once per clustering on the device (include/burgers_hip.h): the local
    bases zero-padded into one stack [C][N][rmax] in centre order (slot = centre index), their widths (int32), UgT =
    U_global[:, :m]^T contiguous, and the centres [C][m].  Shapes that cannot be right raise ValueError; ``ok`` is False
    (with ``reason``) when the clustering is valid but the device loop does not cover it -- beyond bg_local_rom_limits,
    N > 512, or a centre 0 .. C-1 without a basis -- and the caller then takes the host path.
    ``long_mesh``: the operands of bg_local_rom_run_long instead, for 3 <= N <= 1024 (bg_local_rom_run_long_limits): the
    stack is [C][NPAD + 2][40], every block the padded copy of its basis that bg_rom_run_long reads (row i at index i + 1,
    NPAD = N rounded up to 64, zero rows and columns around it)."""

    def __init__(self, centres, local_bases, U_global, m, N, device, long_mesh=False):
        L = _lib.load()
        self.N, self.m = int(N), int(m)
        self.centres = _as_dev(centres, device)
        if self.centres.dim() != 2 or self.centres.shape[1] != self.m:
            raise ValueError(f"centres must be (C, m) with m = {self.m}")
        self.C = self.centres.shape[0]
        Ug = _as_dev(U_global, device)
        if Ug.dim() != 2 or Ug.shape[0] != self.N or Ug.shape[1] < self.m:
            raise ValueError(f"U_global must be (N, >= m) with N = {self.N}, m = {self.m}")
        for k, b in local_bases.items():
            if len(np.shape(b)) != 2 or np.shape(b)[0] != self.N:
                raise ValueError(f"local basis {k} must have one row per mesh node (N = {self.N})")
        self.long_mesh = bool(long_mesh)
        limits = "bg_local_rom_run_long_limits" if self.long_mesh else "bg_local_rom_limits"
        max_n, max_r, max_m, max_c = _lib.limits(limits, 4) if self.long_mesh else (512,) + _lib.limits(limits, 3)
        self.widths_host = [int(np.shape(local_bases[c])[1]) if c in local_bases else 0 for c in range(self.C)]
        self.rmax = max(self.widths_host)
        missing = [c for c in range(self.C) if c not in local_bases]
        if missing:
            self.reason = f"centre {missing[0]} has no local basis"
        elif self.N > max_n or (self.long_mesh and self.N < 3):
            self.reason = f"N = {self.N} > {max_n}" if self.N > max_n else f"N = {self.N} < 3"
        elif self.rmax > max_r or self.m > max_m or self.C > max_c:
            self.reason = (f"beyond {limits}: widths {self.rmax} (<= {max_r}), m {self.m} (<= {max_m}), "
                           f"{self.C} centres (<= {max_c})")
        elif min(self.widths_host) < 1:
            self.reason = "a local basis has no columns"
        else:
            self.reason = None
        self.ok = self.reason is None
        if not self.ok:
            return
        if self.long_mesh:
            self.stack = torch.stack([_padded_basis(_as_dev(local_bases[c], device), self.N, w_, 64, max_r)
                                      for c, w_ in enumerate(self.widths_host)])
            if self.stack.numel() != L.bg_local_rom_run_long_bases_elems(self.N, self.C):
                raise ValueError(f"bg_local_rom_run_long does not cover N = {self.N}, C = {self.C}")
        else:
            self.stack = torch.zeros((self.C, self.N, self.rmax), dtype=torch.float64, device=self.centres.device)
            for c, w_ in enumerate(self.widths_host):
                self.stack[c, :, :w_] = _as_dev(local_bases[c], device)
        self.widths = torch.as_tensor(self.widths_host, dtype=torch.int32, device=self.centres.device)
        self.UgT = Ug[:, :self.m].t().contiguous()


def _local_device_loop(route, X, u0, mu1, mu2, dt, nsteps, centers, local_bases, U_global,
                       num_global_modes, projection, E, tol, max_it, device, plan, balance, options):
    """What local_prom_run_fused (bg_local_rom_run) and local_prom_run_long (bg_local_rom_run_long) share: the plan and
    its checks, the launch with the ``clusters`` output, the result.  Returns None when the plan's clustering is outside
    what the entry point covers."""
    proj = _projection(projection, _NOT_AVAILABLE, exact=True)
    long_mesh = route.entry == "bg_local_rom_run_long"
    device = _lib.require_device(device)
    Xh = check_mesh(X)
    if plan is None:
        plan = LocalPodPlan(centers, local_bases, U_global, num_global_modes, len(Xh), device, long_mesh=long_mesh)
    if (plan.N != len(Xh) or plan.m != int(num_global_modes) or plan.centres.device != device
            or plan.long_mesh != long_mesh):
        raise ValueError("the plan must be built for this mesh, num_global_modes and entry point (and live on the device "
                         "of the call)")
    if not plan.ok:
        return None
    out = {}

    def launch(f, N, B, x, inputs, opts, outputs):
        out["clusters"] = torch.zeros((B, int(nsteps)), dtype=torch.int32, device=device)
        return f(N, B, plan.C, plan.rmax, plan.m, int(nsteps), proj, x, _lib.ptr(plan.stack), _lib.ptr(plan.widths),
                 _lib.ptr(plan.UgT), _lib.ptr(plan.centres), *inputs, float(dt), float(E), float(tol), int(max_it), opts,
                 *outputs[:4], _lib.ptr(out["clusters"]), *outputs[4:])

    res = _device_loop(route, Xh, u0, mu1, mu2, nsteps, device, options, balance, launch, keep=(plan,))
    res.plan = plan
    res.clusters = out["clusters"]
    return res


def local_prom_run_fused(X, u0, mu1, mu2, dt, nsteps, centers, local_bases, U_global, num_global_modes,
                         projection="Galerkin", E=0.0, tol=1e-6, max_it=20, device=None, plan=None, balance=True,
                         options=0):
    """``local_prom_burgers`` for a batch with the whole time loop on the device (bg_local_rom_run): one workgroup per
    sample, the nearest-centre pick at every step start, the cluster's basis reloaded into registers only when it
    changes.  Returns None when the clustering is outside what the kernel covers (LocalPodPlan.ok).  ``res.clusters``:
    (B, nsteps) int32, the centre index of every sample and step.  ``plan``: a LocalPodPlan of the same clustering to
    reuse across calls (``res.plan``); centres, bases and U_global are then not read again."""
    return _local_device_loop(_ROUTES["bg_local_rom_run"], X, u0, mu1, mu2, dt, nsteps, centers, local_bases, U_global,
                              num_global_modes, projection, E, tol, max_it, device, plan, balance, options)


def local_prom_run_long(X, u0, mu1, mu2, dt, nsteps, centers, local_bases, U_global, num_global_modes,
                        projection="Galerkin", E=0.0, tol=1e-6, max_it=20, device=None, plan=None, balance=True,
                        options=0):
    """``local_prom_burgers`` for meshes of up to 1024 nodes (bg_local_rom_run_long_limits; widths <= 40, m and C <= 64)
    with the whole time loop on the device (bg_local_rom_run_long): the picked cluster's basis streams through LDS, the
    pivoting repair runs inside the call, nothing is synchronised.  Raises ValueError when the clustering is outside the
    limits.  ``res.clusters`` and ``plan`` (a LocalPodPlan built with ``long_mesh=True``; ``res.plan``) as in
    local_prom_run_fused."""
    device = _lib.require_device(device)
    if plan is None:
        plan = LocalPodPlan(centers, local_bases, U_global, num_global_modes, len(check_mesh(X)), device, long_mesh=True)
    if not plan.ok:
        raise ValueError(f"bg_local_rom_run_long does not cover this clustering: {plan.reason}")
    return _local_device_loop(_ROUTES["bg_local_rom_run_long"], X, u0, mu1, mu2, dt, nsteps, None, None, None,
                              num_global_modes, projection, E, tol, max_it, device, plan, balance, options)


class HyperLocalPlan:
    """What bg_hyper_local_rom_run reads besides the batch, built once per clustering, sampling and mesh on the device
    (include/burgers_hip.h): the stack PhiS of HyperPodPlan's stencil tables, one per cluster; ``trans`` [C][C][40][40] =
    Phi_c^T Phi_p and ``pick`` [C][mg][40] = U_g^T Phi_p, zero padded; the widths and centres, and _put_stencil's
    arguments; the zero-padded bases ``stack`` (C, N, rmax) and ``UgT`` for the projections of u0 and the decode.
    ``sampling``: a pod.RowSampling (pod.build_local_row_sampling), one for all clusters, row 0 among its rows.  Everything the
    shapes, the sampling and the bases decide is refused with a ValueError before the device is touched -- also a basis with
    |Phi_c^T Phi_c - I|_max > 1e-8: the loop carries q from step to step and crosses from one basis to the next by
    Phi_c^T Phi_p q, which is the reference's Phi_c^T u^n only for orthonormal columns."""

    def __init__(self, centres, local_bases, U_global, num_global_modes, sampling, X, device):
        route = _ROUTES["bg_hyper_local_rom_run"]
        max_r, max_m, max_mg, max_c = _lib.limits("bg_hyper_local_rom_limits", 4)
        Xh = check_mesh(X)
        N, mg = len(Xh), int(num_global_modes)
        cen, bases, Ug = _pod._host_local_bases(centres, local_bases, U_global, mg, N, route.entry)
        C = len(cen)
        if C < 1 or mg < 1:
            raise ValueError(f"centres must be (C, m) with C >= 1 and m = {mg} >= 1")
        if N < route.min_n or N > _limit(route.max_n):
            raise ValueError(f"{route.entry} covers {route.min_n} <= N <= {_limit(route.max_n)}")
        for c, b in enumerate(bases):
            if b.shape[1] > max_r:
                raise ValueError(f"local basis {c} must have at most {max_r} columns (got {b.shape[1]})")
        if mg > max_mg or C > max_c:
            raise ValueError(f"beyond bg_hyper_local_rom_limits: m {mg} (<= {max_mg}), {C} centres (<= {max_c})")
        rows, xi = _sampling_rows(route, sampling, N, max_m)
        if rows[0] != 0:
            raise ValueError("row 0 (the Dirichlet row) must be among the sampled rows")
        self.projection = _projection(str(sampling.projection), _SAMPLING_PROJECTION)
        for c, b in enumerate(bases):
            _require_orthonormal(b, f"local basis {c}", "Phi^T u^n")
        if not (np.isfinite(cen).all() and np.isfinite(Ug).all()):
            raise ValueError("centres and U_global must be finite")
        m = len(rows)
        elems = _lib.load().bg_hyper_local_rom_table_elems(C, m)
        if elems == 0:
            raise ValueError(f"{route.entry} does not cover C = {C}, m = {m}")
        device = _lib.require_device(device)
        self.N, self.C, self.mg = N, C, mg
        _put_stencil(self, rows, xi, sampling, Xh, device)
        self.widths_host = [b.shape[1] for b in bases]
        self.rmax = max(self.widths_host)
        R = max_r                                                                # the padded width of trans and pick
        self.stack = torch.zeros((C, N, self.rmax), dtype=torch.float64, device=device)
        for c, b in enumerate(bases):
            self.stack[c, :, :b.shape[1]] = _as_dev(b, device)
        self.UgT = _as_dev(Ug, device).t().contiguous()
        self.centres = _as_dev(cen, device).contiguous()
        self.widths = torch.as_tensor(self.widths_host, dtype=torch.int32, device=device)
        mpad = (m + 31) // 32 * 32
        cols = elems // (C * 3 * mpad)
        self.PhiS = torch.zeros((C, mpad, 3, cols), dtype=torch.float64, device=device)
        self.PhiS[:, :m, :, :self.rmax] = self.stack[:, self.stencil] * self.inside[None, :, :, None]
        flat = self.stack.permute(1, 0, 2).reshape(N, C * self.rmax)              # all bases side by side
        self._proj = torch.cat([self.UgT.t(), flat], dim=1).contiguous()          # U_g | Phi_0 | ... | Phi_{C-1}
        self._chunk = max(1, min(256, (1 << 25) // self._proj.numel()))           # at most 256 MB per product of project()
        gram = (flat.t() @ flat).reshape(C, self.rmax, C, self.rmax).permute(0, 2, 1, 3)      # [c][p] = Phi_c^T Phi_p
        self.trans = torch.zeros((C, C, R, R), dtype=torch.float64, device=device)
        self.trans[:, :, :self.rmax, :self.rmax] = gram
        self.pick = torch.zeros((C, mg, R), dtype=torch.float64, device=device)
        self.pick[:, :, :self.rmax] = torch.matmul(self.UgT[None], self.stack)

    def project(self, u0d):
        """(qg0 (B, mg), pu0 (B, C, rmax)) = U_g^T u0 and Phi_c^T u0 for every cluster, by _project_rows in chunks of a size
        the plan fixes: a sample's bits do not depend on the batch around it."""
        out = _project_rows(u0d, self._proj, self._chunk)
        return out[:, :self.mg].contiguous(), out[:, self.mg:].reshape(u0d.shape[0], self.C, self.rmax).contiguous()


class HyperLocalRomResult(_HyperResult):
    """Result of local_prom_run_hyper (_HyperResult): entry n + 1 of ``q`` (B, nT+1, rmax) is in the basis of
    ``clusters[:, n]`` (B, nT) int32, entry 0 the projection of u0 on the first cluster's basis.  The decode is column n + 1 =
    Phi_{clusters[:, n]} q[:, n + 1]."""

    def __init__(self, res, plan, u0d, clusters):
        super().__init__(res, plan, u0d)
        self.clusters = clusters

    def _decode(self):
        B, cols, _ = self.q.shape
        hist = torch.empty((B, cols, self.plan.N), dtype=torch.float64, device=self.q.device)
        if cols > 1:
            cl = self.clusters.long()
            for c in range(self.plan.C):                                         # one product per cluster over its (sample, step) pairs
                b, n = (cl == c).nonzero(as_tuple=True)
                if b.numel():
                    hist[b, n + 1] = self.q[b, n + 1] @ self.plan.stack[c].t()
        return hist


def local_prom_run_hyper(X, u0, mu1, mu2, dt, nsteps, centers, local_bases, U_global, num_global_modes, sampling_or_plan, proj,
                         E=0.0, tol=1e-6, max_it=20, device=None, options=0, balance=True):
    """``local_prom_burgers`` HYPER-REDUCED, with the whole time loop on the device (bg_hyper_local_rom_run): every cluster's
    reduced system is assembled from the sampled mesh rows of ONE pod.RowSampling (pod.build_local_row_sampling) with their
    weights, so an iteration costs O(m r^2) whatever the mesh: N up to bg_fom_max_n(), orthonormal bases of at most 40
    modes, m <= 256, at most 64 centres and global modes (bg_hyper_local_rom_limits).  The cluster pick works from reduced
    coordinates and a switch crosses to the new basis by Phi_c^T Phi_p q.  The pivoting repair runs inside the call,
    nothing is synchronised.  ``sampling_or_plan``: the sampling, or a HyperLocalPlan of this clustering, sampling and mesh
    to reuse across calls (``res.plan``; centres, bases and U_global are then not looked at).  A plan built for another
    mesh or device and a sampling trained for the other projection are refused; what the loop does not cover is a
    ValueError, never rerouted.  Returns a HyperLocalRomResult."""
    Xh = check_mesh(X)
    plan = sampling_or_plan if isinstance(sampling_or_plan, HyperLocalPlan) else \
        HyperLocalPlan(centers, local_bases, U_global, num_global_modes, sampling_or_plan, Xh, device)
    device = _check_hyper_call(plan, Xh, device, proj)
    u0d, _, _ = _batch_inputs(u0, mu1, mu2, plan.N, device)
    B = u0d.shape[0]
    qg0, pu0 = plan.project(u0d)
    u0s = (u0d[:, plan.stencil] * plan.inside).contiguous()
    clusters = torch.zeros((B, int(nsteps)), dtype=torch.int32, device=device)
    res = _device_loop(_ROUTES["bg_hyper_local_rom_run"], Xh, u0d, mu1, mu2, nsteps, device, options, balance,
                       lambda f, N, B, x, inputs, opts, outputs: f(
                           N, B, plan.C, plan.rmax, plan.mg, plan.m, int(nsteps), proj, _lib.ptr(plan.rows), _lib.ptr(plan.xi),
                           _lib.ptr(plan.xs), _lib.ptr(plan.PhiS), _lib.ptr(plan.widths), _lib.ptr(plan.trans), _lib.ptr(plan.pick),
                           _lib.ptr(plan.centres), _lib.ptr(qg0), _lib.ptr(pu0), _lib.ptr(u0s), *inputs[1:], float(dt), float(E),
                           float(tol), int(max_it), opts, *outputs[:4], _lib.ptr(clusters), *outputs[4:]),
                       keep=(plan, qg0, pu0, u0s, clusters), cols=plan.rmax)
    return HyperLocalRomResult(res, plan, u0d, clusters)


def _local_route(N, fused=False, long_mesh=False):
    """The device loops local_prom_run tries for a mesh of N nodes, in this order; each is taken if the LocalPodPlan of the
    clustering for it is ``ok`` (inside its limits, a basis for every centre), and "host" is what is left."""
    if not fused:
        return ()
    return (("bg_local_rom_run_long",) if long_mesh and N > _ROUTES["bg_local_rom_run"].max_n else ()) + ("bg_local_rom_run",)


def local_prom_run(X, u0, mu1, mu2, dt, nsteps, centers, local_bases, U_global, num_global_modes,
                   projection="Galerkin", E=0.0, tol=1e-6, max_it=20, device=None, fused=False, long_mesh=False, hyper=None):
    """Batched ``local_prom_burgers`` (FEM/fem_burgers.py:979-1079): each sample picks, once per time
    step, the local basis of the cluster whose centre is nearest to ``U_global[:, :m]^T u^n``
    (= ``kmeans.predict``), then iterates like ``pod_prom_burgers`` in that basis.  The bases are
    zero-padded to a common width and travel as per-sample W; padded reduced unknowns get a unit
    diagonal so that their correction is exactly zero.  ``res.clusters``: (B, nsteps) int32, the
    centre index of every sample and step.
    ``fused``: the device-side time loop bg_local_rom_run (local_prom_run_fused) where it covers the clustering
    (N <= 512, widths <= 40, m and C <= 64, a basis for every centre); otherwise, and by default, the host-driven
    iteration.
    ``long_mesh`` (opt-in, with ``fused``): meshes of 512 < N <= 1024 whose clustering is inside
    bg_local_rom_run_long_limits take the device-side loop bg_local_rom_run_long instead of the host-driven iteration.
    ``hyper`` (opt-in): a pod.RowSampling (pod.build_local_row_sampling) or a HyperLocalPlan sends the call through the
    hyper-reduced loop local_prom_run_hyper, which assembles every cluster's reduced system from the sampled mesh rows only;
    what it does not cover is refused, not rerouted."""
    proj = _projection(projection, _NOT_AVAILABLE, exact=True)
    if hyper is not None:
        return check_singular(local_prom_run_hyper(X, u0, mu1, mu2, dt, nsteps, centers, local_bases, U_global, num_global_modes,
                                                   hyper, proj, E, tol, max_it, device))
    tries = _local_route(np.shape(X)[0], fused, long_mesh)
    if "bg_local_rom_run_long" in tries:
        dev = _lib.require_device(device)
        plan = LocalPodPlan(centers, local_bases, U_global, num_global_modes, len(check_mesh(X)), dev, long_mesh=True)
        if plan.ok:
            return check_singular(local_prom_run_long(X, u0, mu1, mu2, dt, nsteps, None, None, None, num_global_modes,
                                                      projection, E, tol, max_it, dev, plan=plan))
    if "bg_local_rom_run" in tries:
        res = local_prom_run_fused(X, u0, mu1, mu2, dt, nsteps, centers, local_bases, U_global, num_global_modes,
                                   projection, E, tol, max_it, device)
        if res is not None:
            return check_singular(res)
    c = _setup(X, u0, mu1, mu2, dt, E, device)
    ids = sorted(local_bases.keys())
    widths = [int(np.shape(local_bases[i])[1]) for i in ids]
    rmax = max(widths)          # beyond 47 modes rom_reduce / solve_update take their library paths
    stack = torch.zeros((len(ids), c.N, rmax), dtype=torch.float64, device=c.device)
    for s_, (i, w_) in enumerate(zip(ids, widths)):
        stack[s_, :, :w_] = _as_dev(local_bases[i], c.device)
    slot_of = torch.full((max(ids) + 1,), -1, dtype=torch.long, device=c.device)
    slot_of[torch.as_tensor(ids, device=c.device)] = torch.arange(len(ids), device=c.device)
    width_t = torch.as_tensor(widths, device=c.device)
    cen = _as_dev(centers, c.device)                                        # (n_clusters, m)
    Ug = _as_dev(U_global, c.device)[:, :num_global_modes].contiguous()
    col = torch.arange(rmax, device=c.device)
    stackT = stack.transpose(1, 2).contiguous()                              # (C, rmax, N)
    rows = torch.arange(c.B, device=c.device)
    clusters = torch.zeros((c.B, nsteps), dtype=torch.int32, device=c.device)
    q = torch.zeros((c.B, rmax), dtype=torch.float64, device=c.device)

    def step(n, U0, st, Ar, br, wtu, G):
        qg = U0 @ Ug                                                          # (:1011)
        cid = torch.cdist(qg, cen, compute_mode="donot_use_mm_for_euclid_dist").argmin(dim=1)   # kmeans.predict (:1012)
        slot = slot_of[cid]
        if bool((slot < 0).any()):
            raise KeyError("a predicted cluster has no local basis")
        clusters[:, n] = cid
        slot32 = slot.to(torch.int32)                                         # basis of each sample (:1013)
        pad = (col[None, :] >= width_t[slot][:, None]).to(torch.float64)      # 1 on padded reduced unknowns
        while True:
            rom_reduce(c, stack, U0, G, proj, True, st.active, Ar, br, wtu, w_index=slot32)
            Ar.diagonal(dim1=1, dim2=2).add_(pad * st.active[:, None].to(torch.float64))
            left = st.solve_update(1, Ar, br, wtu, q, tol, max_it)           # q = Phi^T U0 + dq
            act = st.active_before
            # U1 = Phi q: one GEMM per cluster over the whole batch against the SHARED bases, then each sample
            # picks its cluster's row (a bmm against the gathered per-sample copies streams B N r doubles)
            U1 = torch.matmul(q, stackT)[slot, rows]                         # (C, B, N) -> (B, N)
            U0 = torch.where(act[:, None], U1, U0).contiguous()
            if left == 0:
                return U0

    res = _host_loop(c, nsteps, rmax, step)
    res.clusters = clusters
    return res
