"""Batched FOM host API on torch device tensors (thin layer over the C ABI).

``fom_run`` is the batched form of the reference's ``FEMBurgers.fom_burgers``
(FEM/fem_burgers.py:646-707): B independent (mu1, mu2) samples, one wavefront each.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import lib as _lib


@dataclass
class FomResult:
    hist: torch.Tensor     # (B, nsteps+1, N) float64, time-major per sample
    iters: torch.Tensor    # (B, nsteps) int32, Picard iterations per step
    flags: torch.Tensor    # (B,) int32, BG_FLAG_* bits
    path: str | None = None  # ROM results: the C entry point of a device-side loop, "host" or "library"

    def snapshots(self):
        """(B, N, nsteps+1) C-contiguous: the reference's per-sample (N, nT+1) layout."""
        return transpose_batched(self.hist)

    @property
    def newton_steps(self):
        return int(self.iters.sum().item())


def _as_dev(a, device, shape=None):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
    t = t.to(device=device, dtype=torch.float64)
    if shape is not None:
        t = t.expand(shape)
    return t.contiguous()


def batch_inputs(u0, mu1, mu2, N, device):
    """Broadcast u0 (N,) | (B, N), mu1 and mu2 scalar | (B,) to one batch size B.  Returns contiguous device
    tensors u0 (B, N), mu1 (B,), mu2 (B,).  Sizes other than 1 and B are an error, not a silent broadcast."""
    mu1d = _as_dev(mu1, device).reshape(-1)
    mu2d = _as_dev(mu2, device).reshape(-1)
    u0d = _as_dev(u0, device)
    if u0d.dim() == 1:
        u0d = u0d.unsqueeze(0)
    if u0d.dim() != 2 or u0d.shape[-1] != N:
        raise ValueError(f"u0 has {u0d.shape[-1]} entries per sample, mesh has {N}")
    sizes = {"mu1": mu1d.numel(), "mu2": mu2d.numel(), "u0": u0d.shape[0]}
    B = max(sizes.values()) if min(sizes.values()) > 0 else 0
    for name, k in sizes.items():
        if k not in (1, B):
            raise ValueError(f"batch sizes do not agree: {sizes}")
    return u0d.expand(B, N).contiguous(), mu1d.expand(B).contiguous(), mu2d.expand(B).contiguous()


def check_mesh(X):
    """Validate the mesh and return it as host data (X is host data in the reference too)."""
    Xh = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float64)
    if Xh.ndim != 1 or len(Xh) < 2:
        raise ValueError("X must be a 1-D array of at least 2 nodes")
    if not np.all(np.diff(Xh) > 0):
        raise ValueError("mesh nodes must be strictly increasing")
    return Xh


def fom_run(X, u0, mu1, mu2, dt, nsteps, E=0.0, tol=1e-6, max_it=20, supg=True, device=None,
            out=None, validate_mesh=True, options=None, trace=False, form=None):
    """Run B samples through ``nsteps`` implicit-Euler steps on the current HIP stream.

    X (N,), u0 (N,) or (B, N), mu1/mu2 scalar or (B,).  Returns a :class:`FomResult` of
    device tensors; nothing is synchronised.  ``out``: a FomResult whose tensors are reused as the
    destination (shape, dtype, device and contiguity are checked: the kernel writes through raw pointers).
    ``trace``: also return ``res.errs`` (B, nsteps, max_it), the error of every Picard iteration (NaN where none ran).
    ``form``: None = the library's choice (one wavefront per sample up to N = 1536, one workgroup per sample beyond);
    "wide" asks for the workgroup form also for 64 < N <= 1536 on a uniform mesh (measured slower there), "wave" = default.
    """
    L = _lib.load()
    device = _lib.require_device(device)
    if options is None:
        # validate_mesh=False skips the host round trip of X (a device tensor in a timed loop) and therefore ASSUMES the
        # uniform mesh every driver of the reference builds (np.linspace); a caller with a graded mesh must pass
        # ``options`` (BG_OPT_SUPG | BG_OPT_NONUNIFORM) or leave validate_mesh on
        options = _lib.mesh_options(check_mesh(X), supg) if validate_mesh else (_lib.BG_OPT_SUPG if supg else 0)
    if form is not None:
        options |= {"wide": _lib.BG_OPT_FOM_WIDE, "wave": _lib.BG_OPT_FOM_WAVE}[form]
    Xd = _as_dev(X, device)
    N = Xd.numel()
    u0d, mu1d, mu2d = batch_inputs(u0, mu1, mu2, N, device)
    B = mu1d.numel()
    if out is None:
        hist = torch.empty((B, nsteps + 1, N), dtype=torch.float64, device=device)
        iters = torch.empty((B, nsteps), dtype=torch.int32, device=device)
        flags = torch.empty((B,), dtype=torch.int32, device=device)
    else:
        hist, iters, flags = out.hist, out.iters, out.flags
        for name, t, shape, dt_ in (("hist", hist, (B, nsteps + 1, N), torch.float64), ("iters", iters, (B, nsteps), torch.int32),
                                    ("flags", flags, (B,), torch.int32)):
            if tuple(t.shape) != shape or t.dtype != dt_ or t.device != device or not t.is_contiguous():
                raise ValueError(f"out.{name} must be a contiguous {dt_} tensor of shape {shape} on {device} "
                                 f"(got {tuple(t.shape)}, {t.dtype}, {t.device})")
    errs = None
    if trace:                          # error of every iteration (what the reference prints, :664); N <= 1536
        errs = torch.full((B, int(nsteps), int(max_it)), float("nan"), dtype=torch.float64, device=device)
        with torch.cuda.device(device):
            rc = L.bg_fom_run_traced(N, B, int(nsteps), _lib.ptr(Xd), _lib.ptr(u0d), _lib.ptr(mu1d), _lib.ptr(mu2d),
                                     float(dt), float(E), float(tol), int(max_it), int(options), _lib.ptr(hist),
                                     _lib.ptr(iters), _lib.ptr(flags), _lib.ptr(errs), _lib.stream_ptr(device))
        if rc == _lib.BG_ERR_UNSUPPORTED_N:
            trace, errs = False, None  # workgroup-per-sample sizes: no traced kernel
    if not trace:
        with torch.cuda.device(device):
            rc = L.bg_fom_run(N, B, int(nsteps), _lib.ptr(Xd), _lib.ptr(u0d), _lib.ptr(mu1d), _lib.ptr(mu2d),
                              float(dt), float(E), float(tol), int(max_it), int(options),
                              _lib.ptr(hist), _lib.ptr(iters), _lib.ptr(flags), _lib.stream_ptr(device))
    _lib.check(rc, "bg_fom_run")
    res = FomResult(hist, iters, flags)
    res.errs = errs
    return res


def fom_assemble(X, uk, un, mu1, mu2, dt, E=0.0, supg=True, device=None):
    """One Picard assembly: returns (lo, di, up, rhs), each (B, N); rhs = b - A(uk) uk."""
    L = _lib.load()
    device = _lib.require_device(device)
    options = _lib.mesh_options(check_mesh(X), supg)
    Xd = _as_dev(X, device)
    N = Xd.numel()
    ukd = _as_dev(uk, device).reshape(-1, N)
    B = ukd.shape[0]
    und = _as_dev(un, device).reshape(-1, N).expand(B, N).contiguous()
    mu1d = _as_dev(mu1, device).reshape(-1).expand(B).contiguous()
    mu2d = _as_dev(mu2, device).reshape(-1).expand(B).contiguous()
    outs = [torch.empty((B, N), dtype=torch.float64, device=device) for _ in range(4)]
    with torch.cuda.device(device):
        rc = L.bg_fom_assemble(N, B, _lib.ptr(Xd), _lib.ptr(ukd), _lib.ptr(und), _lib.ptr(mu1d),
                               _lib.ptr(mu2d), float(dt), float(E), int(options),
                               *[_lib.ptr(o) for o in outs], _lib.stream_ptr(device))
    _lib.check(rc, "bg_fom_assemble")
    return tuple(outs)


def tridiag_solve(lo, di, up, rhs):
    """Batched tridiagonal solve, one wavefront per system; inputs (B, N) device tensors."""
    L = _lib.load()
    device = _lib.require_device(lo.device)
    lo, di, up, rhs = [t.to(torch.float64).contiguous() for t in (lo, di, up, rhs)]
    B, N = lo.shape
    sol = torch.empty_like(rhs)
    with torch.cuda.device(device):
        rc = L.bg_tridiag_solve(N, B, _lib.ptr(lo), _lib.ptr(di), _lib.ptr(up), _lib.ptr(rhs),
                                _lib.ptr(sol), _lib.stream_ptr(device))
    _lib.check(rc, "bg_tridiag_solve")
    return sol


def transpose_batched(t):
    """(B, R, C) -> (B, C, R), contiguous, by the HIP transpose kernel."""
    L = _lib.load()
    device = _lib.require_device(t.device)
    t = t.contiguous()
    B, R, C = t.shape
    out = torch.empty((B, C, R), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        rc = L.bg_transpose_batched(B, R, C, _lib.ptr(t), _lib.ptr(out), _lib.stream_ptr(device))
    _lib.check(rc, "bg_transpose_batched")
    return out


def _fd_residual(U, Up, dt, dx, s_src):
    """compute_residual (FD/fd_burgers.py:28-35) on the last axis; nu = 0.25 dx max|U| per state."""
    nu = 0.25 * dx * U.abs().amax(dim=-1, keepdim=True)
    R = torch.zeros_like(U)
    conv = (0.5 * U[..., 2:] ** 2 - 0.5 * U[..., :-2] ** 2) / (2 * dx)
    diff = nu * (U[..., 2:] - 2 * U[..., 1:-1] + U[..., :-2]) / dx ** 2
    R[..., 1:-1] = (U[..., 1:-1] - Up[..., 1:-1]) / dt + conv - s_src[..., 1:-1] - diff
    return R


def _fd_run_fd_jacobian(a, b, N, u0d, mu1d, mu2d, dt, nsteps, max_iter, tol, device):
    """The reference's debugging variant (FD/fd_burgers.py:46-57, ``use_fd_jacobian=True``): the Jacobian is formed by
    one-sided differences of the residual (eps = 1e-8, the artificial viscosity re-evaluated per perturbed state), which
    makes it DENSE -- there is no tridiagonal kernel to write.  Library path on the device: batched residuals of the
    N - 2 perturbed states, one batched dense solve per Newton iteration, per-sample stopping as in :71-101."""
    B = mu1d.numel()
    dx = (b - a) / (N - 1)
    x = torch.linspace(a, b, N, dtype=torch.float64, device=device)
    s_src = 0.02 * torch.exp(mu2d[:, None] * x[None, :])                     # (B, N)
    hist = torch.empty((B, nsteps + 1, N), dtype=torch.float64, device=device)
    iters = torch.zeros((B, nsteps), dtype=torch.int32, device=device)
    flags = torch.zeros((B,), dtype=torch.int32, device=device)
    eye = 1e-8 * torch.eye(N, dtype=torch.float64, device=device)[1:N - 1]   # (N-2, N)

    def bc(U):
        U = U.clone(); U[:, 0] = mu1d; U[:, -1] = U[:, -2]
        return U

    Uc = bc(u0d)
    hist[:, 0] = Uc
    for step in range(nsteps):
        Up, Ug = Uc.clone(), Uc.clone()
        active = torch.ones((B,), dtype=torch.bool, device=device)
        singular = torch.zeros((B,), dtype=torch.bool, device=device)
        k = torch.zeros((B,), dtype=torch.int32, device=device)
        for _ in range(max_iter):
            Ug = torch.where(active[:, None], bc(Ug), Ug)
            R = _fd_residual(Ug, Up, dt, dx, s_src)
            active = active & ~(R[:, 1:-1].abs().amax(dim=1) < tol)          # "Converged." on the residual (:77)
            if not bool(active.any()):
                break
            # only the samples still iterating pay for a dense Jacobian and its (N-2)^3 solve
            ia = active.nonzero().squeeze(1)
            Ua, Upa, Ra, sa = Ug[ia], Up[ia], R[ia], s_src[ia]
            Rp = _fd_residual(Ua[:, None, :] + eye[None], Upa[:, None, :], dt, dx, sa[:, None, :])     # (Ba, N-2, N)
            J = ((Rp[:, :, 1:N - 1] - Ra[:, None, 1:N - 1]) / 1e-8).transpose(1, 2)                  # J[i, j] = dR_i/dU_j
            sol, info = torch.linalg.solve_ex(J, -Ra[:, 1:-1].unsqueeze(-1), check_errors=False)
            # "Jacobian is singular" (:88-93): that sample leaves its Newton loop with U_guess as it stands, no update
            # and no count for this iteration; the others go on
            good = info == 0
            ig = ia[good]
            dU = torch.zeros_like(Ua)
            dU[:, 1:-1] = sol.squeeze(-1)
            rel = dU[:, 1:-1].abs().amax(dim=1) / Ua[:, 1:-1].abs().amax(dim=1).clamp_min(1e-15)
            Ug[ig] = (Ua + dU)[good]
            k[ig] += 1
            active[ia] = good & ~(rel < tol)
            singular[ia[~good]] = True
        flags |= (active & ~singular).to(torch.int32) * _lib.BG_FLAG_HIT_CAP  # "did not converge within max_iter" (:97)
        iters[:, step] = k
        Uc = bc(Ug)
        hist[:, step + 1] = Uc
    return FomResult(hist, iters, flags)


def fd_run(a, b, N, u0, mu1, mu2, dt, nsteps, max_iter=30, tol=1e-8, device=None, use_fd_jacobian=False):
    """Batched ``FDBurgers.fom_burgers_newton`` (FD/fd_burgers.py:59-107) on the mesh linspace(a, b, N)."""
    L = _lib.load()
    device = _lib.require_device(device)
    Xd = _as_dev(np.linspace(a, b, N), device)
    try:
        u0d, mu1d, mu2d = batch_inputs(u0, mu1, mu2, N, device)
    except ValueError as e:
        raise ValueError(str(e).replace("u0 has", "U0 has")) from None
    B = mu1d.numel()
    if use_fd_jacobian:
        return _fd_run_fd_jacobian(float(a), float(b), int(N), u0d, mu1d, mu2d, float(dt), int(nsteps), int(max_iter),
                                   float(tol), device)
    hist = torch.empty((B, nsteps + 1, N), dtype=torch.float64, device=device)
    iters = torch.empty((B, nsteps), dtype=torch.int32, device=device)
    flags = torch.empty((B,), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        rc = L.bg_fd_run(N, B, int(nsteps), _lib.ptr(Xd), _lib.ptr(u0d), _lib.ptr(mu1d), _lib.ptr(mu2d), float(dt),
                         float(tol), int(max_iter), _lib.ptr(hist), _lib.ptr(iters), _lib.ptr(flags),
                         _lib.stream_ptr(device))
    _lib.check(rc, "bg_fd_run")
    return FomResult(hist, iters, flags)
