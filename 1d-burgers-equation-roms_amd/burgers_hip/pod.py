"""Offline basis builders on torch tensors (device or CPU) and the reference's .npy contracts.

  POD basis           POD/pod.py:8-14 (energy rule), :68-90 (thin SVD, file names)
  quadratic manifold  Quadratic_manifold/build_quadratic_manifold.py:25-48, quad_utils.py:63-81
  local POD           what FEMBurgers.local_prom_burgers consumes (FEM/fem_burgers.py:979-1079): k-means centres in global
                      POD coordinates and one overlapping basis per cluster (kmeans, build_local_bases)
  snapshot files      FEM/paper_training_stage.py:52-53
"""
from __future__ import annotations

import functools
import os

import numpy as np
import torch


def snapshot_matrix(hist):
    """(B, nT+1, N) time-major histories -> (N, B*(nT+1)) snapshot matrix, i.e. np.hstack of the
    per-sample (N, nT+1) arrays the reference stacks (POD/pod.py:80-82)."""
    B, T, N = hist.shape
    return hist.reshape(B * T, N).t()


def n_modes_for_tolerance(s, epsilon_squared):
    """K = argmax(1 - cumsum(s^2)/sum(s^2) <= eps^2) + 1   (POD/pod.py:8-14)."""
    s = torch.as_tensor(s, dtype=torch.float64)
    s_sorted = torch.sort(s, descending=True).values
    c = torch.cumsum(s_sorted ** 2, 0)
    loss = 1.0 - c / c[-1]
    hit = torch.nonzero(loss <= epsilon_squared)
    return int(hit[0]) + 1 if len(hit) else 1


@functools.lru_cache(maxsize=8)
def _round_robin(m):
    """(m' - 1, m'/2, 2) int32 pairs of a round-robin tournament over m rows (m' = m rounded up to even;
    the dummy player shows as -1)."""
    n = m + (m & 1)
    idx = np.arange(n)
    steps = np.empty((n - 1, n // 2, 2), dtype=np.int32)
    for r in range(n - 1):
        steps[r, :, 0] = idx[:n // 2]
        steps[r, :, 1] = idx[::-1][:n // 2]
        idx = np.concatenate([idx[:1], idx[-1:], idx[1:-1]])
    steps[steps >= m] = -1
    return torch.from_numpy(steps)


def _require_finite(A, who):
    """The reference's np.linalg.svd raises LinAlgError on NaN / Inf input; a NaN row would otherwise pass the
    kernel's skip test and come back as a NaN mode."""
    if not bool(torch.isfinite(A).all()):
        raise np.linalg.LinAlgError(f"{who}: the matrix holds NaN or Inf")


def jacobi_svd(R, tol=1e-15, max_sweeps=80, info=None):
    """SVD of a square device matrix by one-sided Jacobi on the HIP kernel bg_jacobi_sweep.
    Returns U, s, Vh with R = U diag(s) Vh, s descending.  The rotations act on the ROWS of R, i.e.
    on the columns of R^T: R^T J = W with orthogonal columns  =>  R = J (W^T): left vectors J, right W/|W|.

    Before every sweep, rows whose squared norm is at or below (eps |R|_F)^2 are set to zero: they hold rounding
    noise of the input, which rotations against the large rows keep regenerating above the relative tol, so a
    rank-deficient core otherwise rotates forever (N x 808 bench gather: ~4800 rotations in every sweep).  Their
    singular values come back 0 and their rows of Vh zero; the kernel skips every pair holding a zero row.  A
    floor of m eps |R|_F would also converge but moves the modes near sigma/sigma_1 = 1e-7 by 4e-7 (measured).
    Graded cores of condition 1e10 need up to ~46 sweeps at m = 512..777.  A sweep that still rotates at
    max_sweeps raises RuntimeError; NaN / Inf input raises LinAlgError.  ``info`` (a dict) receives the sweep
    count."""
    from . import lib as _lib
    L = _lib.load()
    _require_finite(R, "jacobi_svd")
    m = R.shape[0]
    G = R.contiguous().clone()
    Jt = torch.eye(m, dtype=torch.float64, device=R.device)
    pairs = _round_robin(m).to(R.device)
    rot = torch.zeros((1,), dtype=torch.int32, device=R.device)
    floor = (torch.finfo(torch.float64).eps * torch.linalg.matrix_norm(G)) ** 2
    n_rot = sweep = 0
    with torch.cuda.device(R.device):
        for sweep in range(1, max_sweeps + 1):
            G.masked_fill_((G * G).sum(1, keepdim=True) <= floor, 0.0)
            rot.zero_()
            _lib.check(L.bg_jacobi_sweep(m, m, _lib.ptr(G), _lib.ptr(Jt), _lib.ptr(pairs), pairs.shape[0], pairs.shape[1],
                                         float(tol), _lib.ptr(rot), _lib.stream_ptr(R.device)), "bg_jacobi_sweep")
            n_rot = int(rot.item())
            if n_rot == 0:
                break
    if n_rot:
        raise RuntimeError(f"jacobi_svd: not converged after {max_sweeps} sweeps (m = {m}, {n_rot} rotations in the last)")
    if info is not None:
        info["sweeps"] = sweep
    s = torch.linalg.vector_norm(G, dim=1)
    order = torch.argsort(s, descending=True)
    s, G, Jt = s[order], G[order], Jt[order]
    Vh = G / torch.clamp(s, min=torch.finfo(torch.float64).tiny)[:, None]
    return Jt.t().contiguous(), s, Vh


def jacobi_svd_batched(Rs, tol=1e-15, max_sweeps=80, info=None):
    """jacobi_svd of every matrix of the (count, m, m) device tensor ``Rs`` in the launches of one (bg_jacobi_sweep_batched):
    stacked U, s, Vh, each matrix finished and sorted as jacobi_svd does it, and bitwise what jacobi_svd returns for that
    matrix alone.  The rounding floor and the rotation count are per matrix; a matrix that has converged makes no rotation
    in the sweeps the others still need.  Raises RuntimeError naming the matrices that still rotate at ``max_sweeps``;
    NaN / Inf raises LinAlgError.  ``info`` (a dict) receives ``sweeps`` (per matrix, the sweep that made no rotation) and
    ``rotations`` (one list per sweep, one count per matrix)."""
    from . import lib as _lib
    L = _lib.load()
    _require_finite(Rs, "jacobi_svd_batched")
    if Rs.dim() != 3 or Rs.shape[1] != Rs.shape[2]:
        raise ValueError("jacobi_svd_batched takes a (count, m, m) tensor")
    count, m = Rs.shape[0], Rs.shape[1]
    G = Rs.contiguous().clone()
    Jt = torch.eye(m, dtype=torch.float64, device=Rs.device).repeat(count, 1, 1)
    pairs = _round_robin(m).to(Rs.device)
    rot = torch.zeros((count,), dtype=torch.int32, device=Rs.device)
    eps = torch.finfo(torch.float64).eps
    # (every per-matrix reduction runs on a copy of that matrix: the same shape and alignment as in jacobi_svd, hence its bits)
    floor = torch.stack([(eps * torch.linalg.matrix_norm(G[k].clone())) ** 2 for k in range(count)]).reshape(count, 1, 1)
    n_rot, sweeps, history = [0] * count, [0] * count, []
    with torch.cuda.device(Rs.device):
        for sweep in range(1, max_sweeps + 1):
            if count == 0:
                break
            G.masked_fill_((G * G).sum(2, keepdim=True) <= floor, 0.0)
            rot.zero_()
            _lib.check(L.bg_jacobi_sweep_batched(m, m, count, m * m, _lib.ptr(G), _lib.ptr(Jt), _lib.ptr(pairs), pairs.shape[0],
                                                 pairs.shape[1], float(tol), _lib.ptr(rot), _lib.stream_ptr(Rs.device)),
                       "bg_jacobi_sweep_batched")
            n_rot = rot.tolist()
            history.append(n_rot)
            sweeps = [sweep if (v == 0 and n == 0) else v for v, n in zip(sweeps, n_rot)]
            if not any(n_rot):
                break
    if any(n_rot):
        late = ", ".join(f"matrix {k}: {n} rotations in the last" for k, n in enumerate(n_rot) if n)
        raise RuntimeError(f"jacobi_svd_batched: not converged after {max_sweeps} sweeps (m = {m}; {late})")
    if info is not None:
        info["sweeps"], info["rotations"] = sweeps, history
    U, S, Vh = torch.empty_like(G), torch.empty((count, m), dtype=torch.float64, device=Rs.device), torch.empty_like(G)
    tiny = torch.finfo(torch.float64).tiny
    for k in range(count):
        Gk, Jk = G[k].clone(), Jt[k].clone()
        s = torch.linalg.vector_norm(Gk, dim=1)
        order = torch.argsort(s, descending=True)
        s, Gk, Jk = s[order], Gk[order], Jk[order]
        U[k], S[k], Vh[k] = Jk.t(), s, Gk / torch.clamp(s, min=tiny)[:, None]
    return U, S, Vh


def thin_svd(A, info=None):
    """U, s, Vh of a wide matrix A (m x M), M >> m (snapshot matrices are N x B (nT+1)), on A's device.

    A^T = Q R by Householder QR (O(M m^2), rocSOLVER), then the SVD of the m x m core by one-sided Jacobi
    (bg_jacobi_sweep), and A = R^T Q^T = Vr s (Q Ur)^T.  rocSOLVER's own SVD is a Jacobi eigensolver on the
    Gram matrix: measured absolute accuracy 1e-9 sigma_max (tools/time_pod.py), which loses the singular
    triplets a 1e-6 energy tolerance still keeps.  A tall A (m > M) works on A^T.  On CPU tensors (tests,
    fixtures) LAPACK does the lot.

    Triplets at the rounding level of the input, sigma <= eps |A|_F, come back as sigma = 0 with a zero column of U
    (wide A) or zero row of Vh (tall A), see jacobi_svd; every larger triplet is kept.  A device A holding NaN or
    Inf raises LinAlgError, as np.linalg.svd does; a core that does not converge raises RuntimeError.  ``info``
    (a dict) receives the Jacobi sweep count."""
    m, M = A.shape
    if not A.is_cuda:
        return torch.linalg.svd(A, full_matrices=False)
    if m > M:                                                     # tall: work on the transpose
        V, s, Uh = thin_svd(A.t(), info)
        return Uh.t().contiguous(), s, V.t().contiguous()
    _require_finite(A, "thin_svd")
    Q, R = torch.linalg.qr(A.t(), mode="reduced")                # (M, m), (m, m)
    Ur, s, VrT = jacobi_svd(R, info=info)
    return VrT.t().contiguous(), s, (Q @ Ur).t()


def pod_basis(S, epsilon_squared=None, n_modes=None):
    """Thin SVD of the snapshot matrix and truncation.  Returns (U[:, :K], s[:K], s_all)."""
    U, s, _ = thin_svd(S)
    K = n_modes if n_modes is not None else n_modes_for_tolerance(s, epsilon_squared)
    return U[:, :K].contiguous(), s[:K].contiguous(), s


def align_signs(U, U_ref):
    """Singular vectors are defined up to sign; flip columns of U to match U_ref."""
    sgn = torch.sign((U * U_ref).sum(0))
    sgn[sgn == 0] = 1
    return U * sgn


def build_Q(q):
    """(n, Ns) reduced coordinates -> (k, Ns) unique monomials q_i q_j, j >= i (quad_utils.py:21-31)."""
    n = q.shape[0]
    I, J = np.triu_indices(n)
    I = torch.as_tensor(I, device=q.device); J = torch.as_tensor(J, device=q.device)
    return q[I] * q[J]


def compute_H(Q, E, alpha):
    """Ridge fit min ||E - H Q||_F^2 + alpha^2 ||H||_F^2  (quad_utils.py:63-81).

    The reference writes the minimiser through the thin SVD of Q, H = (Uq diag(s^2/(s^2+alpha^2))) (Vq^T E^T / s)^T.
    The same minimiser is the least-squares solution of [Q^T; alpha I] H^T = [E^T; 0], solved here by Householder
    QR and a triangular solve on the device: backward stable at condition sigma_max/alpha, where the device SVD
    (see thin_svd) returned H with 2e-3 relative error.  Measured on the 9-sample training fit (N = 512, n = 21):
    agrees with the SVD formula to 3e-11 on CPU tensors (LAPACK QR) but to 1.9e-8 on the device, from the same Phi
    and snapshots, and with the committed H.npy to 1.9e-8 on the device (tests/test_offline_builders_gpu.py)."""
    k = Q.shape[0]
    A = torch.cat([Q.t(), alpha * torch.eye(k, dtype=Q.dtype, device=Q.device)], 0)      # (Ns + k, k)
    B = torch.cat([E.t(), torch.zeros((k, E.shape[0]), dtype=Q.dtype, device=Q.device)], 0)
    Qa, Ra = torch.linalg.qr(A, mode="reduced")
    return torch.linalg.solve_triangular(Ra, Qa.t() @ B, upper=True).t().contiguous()


def build_quadratic_manifold(S, n, alpha=1e-2):
    """Phi (N, n), H (N, n(n+1)/2), q (n, Ns) from snapshots S (build_quadratic_manifold.py:25-48)."""
    U, _, _ = thin_svd(S)
    Phi = U[:, :n].contiguous()
    q = Phi.t() @ S
    Q = build_Q(q)
    Em = S - Phi @ q
    return Phi, compute_H(Q, Em, alpha), q


# ---- local POD: clustering in global POD coordinates and one overlapping basis per cluster ------------------------------
def _assign(Q, centres, overlap=None, labels=None):
    """Nearest centre of every row of Q (Ns, m): labels (int32), the squared distance to it, the membership words (int64
    holding the 64 bits; with ``overlap``: bit c set iff c is the label or d2[i, c] < overlap d2min[i]) or None, and the
    number of labels that differ from ``labels`` (all of them when None).  Device tensors: bg_kmeans_assign, the arithmetic
    of the online pick.  CPU tensors: the direct sum in torch."""
    Ns, m = Q.shape
    C = centres.shape[0]
    if not Q.is_cuda:
        d2 = ((Q[:, None, :] - centres[None]) ** 2).sum(2)
        new = torch.argmin(d2, 1).to(torch.int32)
        d2min = d2.gather(1, new.long()[:, None])[:, 0]
        bits = None
        if overlap is not None:
            mask = (torch.arange(C)[None, :] == new[:, None]) | (d2 < overlap * d2min[:, None])
            words = (mask.numpy().astype(np.uint64) << np.arange(C, dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)
            bits = torch.from_numpy(words.view(np.int64).copy())
        changed = Ns if labels is None else int((new != labels).sum())
        return new, d2min, bits, changed
    from . import lib as _lib
    L = _lib.load()
    new = torch.full((Ns,), -1, dtype=torch.int32, device=Q.device) if labels is None else labels.to(torch.int32).clone()
    d2min = torch.empty((Ns,), dtype=torch.float64, device=Q.device)
    bits = torch.zeros((Ns,), dtype=torch.int64, device=Q.device) if overlap is not None else None
    changed = torch.zeros((1,), dtype=torch.int32, device=Q.device)
    with torch.cuda.device(Q.device):
        _lib.check(L.bg_kmeans_assign(Ns, m, C, _lib.ptr(Q), _lib.ptr(centres), float(overlap or 0.0), _lib.ptr(new),
                                      _lib.ptr(d2min), _lib.ptr(bits), _lib.ptr(changed), _lib.stream_ptr(Q.device)),
                   "bg_kmeans_assign")
    return new, d2min, bits, int(changed.item())


def _update(Q, labels, centres):
    """The centres moved to the means of their points, in place (a cluster without points keeps its centre), and the
    points per cluster (int32).  Device tensors: bg_kmeans_update, bitwise reproducible."""
    C, m = centres.shape
    if not Q.is_cuda:
        counts = torch.bincount(labels.long(), minlength=C)
        sums = torch.zeros_like(centres).index_add_(0, labels.long(), Q)
        full = counts > 0
        centres[full] = sums[full] / counts[full, None].to(torch.float64)
        return counts.to(torch.int32)
    from . import lib as _lib
    counts = torch.zeros((C,), dtype=torch.int32, device=Q.device)
    with torch.cuda.device(Q.device):
        _lib.check(_lib.load().bg_kmeans_update(Q.shape[0], m, C, _lib.ptr(Q), _lib.ptr(labels), _lib.ptr(centres),
                                                _lib.ptr(counts), _lib.stream_ptr(Q.device)), "bg_kmeans_update")
    return counts


def member_mask(member_bits, c):
    """Boolean (Ns,) mask of the snapshots whose membership word has bit ``c`` set (build_local_bases)."""
    return ((member_bits >> int(c)) & 1).bool()


class KMeansResult:
    """What kmeans returns.  ``centres`` (C, m) and ``labels`` (Ns,) int32 live on the device of the points;
    ``cluster_centers_`` is the host copy under scikit-learn's name, so that the object can be passed as the ``kmeans``
    argument of FEMBurgers.local_prom_burgers.  ``n_iter`` assignment passes were made, ``converged`` says whether the last
    of them changed no label, ``inertia`` is the sum of the squared distances to the nearest centre."""

    def __init__(self, centres, labels, n_iter, converged, inertia, changed=()):
        self.centres, self.labels = centres, labels
        self.cluster_centers_ = centres.detach().cpu().numpy()
        self.n_iter, self.converged, self.inertia = int(n_iter), bool(converged), float(inertia)
        self.changed = list(changed)                    # labels changed by every assignment pass

    @property
    def labels_(self):
        return self.labels.cpu().numpy()

    def predict(self, q):
        """Index of the nearest centre of every row of ``q`` ((m,) or (n, m)): a device tensor for a device tensor (labelled
        by bg_kmeans_assign on its device), otherwise a NumPy array."""
        if isinstance(q, torch.Tensor) and q.is_cuda:
            t = q.to(torch.float64).reshape(-1, self.centres.shape[1]).contiguous()
            return _assign(t, self.centres.to(t.device))[0]
        t = torch.as_tensor(np.atleast_2d(np.asarray(q.detach().cpu() if isinstance(q, torch.Tensor) else q, dtype=np.float64)))
        return _assign(t, torch.as_tensor(self.cluster_centers_))[0].numpy()


def kmeans(Q, n_clusters, init=None, seed=0, max_iter=100):
    """Lloyd iterations on the rows of ``Q`` (Ns, m), on Q's device: assign every point to its nearest centre
    (bg_kmeans_assign: the distance arithmetic and tie rule of the online pick of bg_local_rom_run), move every centre to
    the mean of its points (bg_kmeans_update; a cluster without points keeps its centre), until a pass changes no label or
    ``max_iter`` passes were made.  One integer comes back to the host per pass, as in jacobi_svd.
    ``init``: (C, m) starting centres; None takes the rows numpy.random.default_rng(seed).choice(Ns, C, replace=False)
    of Q, the recipe of the golden-fixture generator.  When the passes run out, one more assignment makes the labels and the
    inertia those of the returned centres.  NaN / Inf in Q or init raises LinAlgError; more centres or coordinates than
    bg_kmeans_limits allows raise ValueError on the device.  CPU tensors take a plain torch path (tests, fixtures).
    Returns a KMeansResult."""
    if Q.dim() != 2:
        raise ValueError("kmeans takes the points as the rows of a (Ns, m) tensor")
    Q = Q.to(torch.float64).contiguous()
    Ns, m = Q.shape
    C = int(n_clusters)
    if C < 1 or Ns < 1 or m < 1 or (init is None and C > Ns):
        raise ValueError(f"kmeans: {C} clusters of {Ns} points in {m} coordinates")
    _require_finite(Q, "kmeans")
    if init is None:
        rows = np.random.default_rng(seed).choice(Ns, C, replace=False)
        centres = Q[torch.as_tensor(rows, device=Q.device)].clone()
    else:
        centres = torch.as_tensor(init).to(device=Q.device, dtype=torch.float64).contiguous().clone()
        if centres.shape != (C, m):
            raise ValueError(f"init must be ({C}, {m}), got {tuple(centres.shape)}")
        _require_finite(centres, "kmeans (init)")
    if Q.is_cuda:
        from . import lib as _lib
        max_m, max_c = _lib.limits("bg_kmeans_limits", 2)
        if m > max_m or C > max_c:
            raise ValueError(f"kmeans: beyond bg_kmeans_limits: {m} coordinates (<= {max_m}), {C} centres (<= {max_c})")
    labels, d2min, n_iter, converged, history = None, None, 0, False, []
    for n_iter in range(1, int(max_iter) + 1):
        labels, d2min, _, changed = _assign(Q, centres, labels=labels)
        history.append(changed)
        if changed == 0:
            converged = True
            break
        _update(Q, labels, centres)
    if not converged:
        labels, d2min, _, _ = _assign(Q, centres, labels=labels)
    return KMeansResult(centres, labels, n_iter, converged, float(d2min.sum()), history)


class LocalBases:
    """What build_local_bases returns and save_local_bases stores: ``centres`` (C, m), ``local_bases`` {cluster id: (N, r_c)
    contiguous}, ``U_global``, ``num_global_modes``, ``labels`` (Ns,) int32, ``member_bits`` (Ns,) int64 (bit c: snapshot in
    cluster c's overlapping set, see member_mask), ``member_counts`` and ``singular_values`` per cluster, ``overlap`` and
    the KMeansResult ``kmeans``.  centres, local_bases, U_global and num_global_modes are the arguments of
    rom.local_prom_run; ``kmeans`` is the one FEMBurgers.local_prom_burgers takes."""

    def __init__(self, centres, local_bases, U_global, num_global_modes, labels, member_bits, member_counts, singular_values,
                 overlap, kmeans):
        self.centres, self.local_bases, self.U_global, self.num_global_modes = centres, local_bases, U_global, int(num_global_modes)
        self.labels, self.member_bits, self.member_counts = labels, member_bits, [int(v) for v in member_counts]
        self.singular_values, self.overlap, self.kmeans = singular_values, float(overlap), kmeans


def build_local_bases(S, n_clusters, num_global_modes, U_global=None, overlap=1.5, epsilon_squared=None, n_modes=None,
                      max_modes=None, init=None, seed=0, max_iter=100, batched=True, info=None):
    """Snapshots S (N, Ns) -> the clustering and the local bases the local POD PROM runs on, on S's device.

      1. U_global = thin_svd(S)[0] unless given;  2. Q = (U_global[:, :m]^T S)^T, m = num_global_modes;
      3. kmeans(Q, n_clusters, init, seed, max_iter);  4. one more assignment pass writes the membership words: snapshot i
      belongs to cluster c's set iff c is its label or d2[i, c] < overlap * d2min[i] -- the overlap rule of this project's
      golden-fixture generator (tests/golden/make_golden.py fx_local_pod);  5. the left singular vectors of every cluster's
      snapshot columns: S_c^T = Q_c R_c (library QR), the N x N cores of the clusters with at least N members through
      jacobi_svd_batched in one batch, the others through thin_svd;  6. truncation at ``n_modes`` (an int or one per
      cluster), else at n_modes_for_tolerance(s_c, epsilon_squared) capped at ``max_modes`` (the device loops take 40).

    ``batched=False`` sends every cluster through thin_svd: the same bits, one Jacobi core at a time.  More clusters or
    coordinates than bg_kmeans_limits (the limits of the device loops) and a cluster whose set is empty raise ValueError.
    ``info`` (a dict) receives the Jacobi sweep counts.  Returns a LocalBases."""
    from . import lib as _lib
    if S.dim() != 2:
        raise ValueError("build_local_bases takes the (N, Ns) snapshot matrix")
    N, Ns = S.shape
    C, m = int(n_clusters), int(num_global_modes)
    max_m, max_c = _lib.limits("bg_kmeans_limits", 2)
    if C > max_c or m > max_m:
        raise ValueError(f"build_local_bases: {C} clusters (<= {max_c}) in {m} global coordinates (<= {max_m}): beyond what "
                         "the local POD loops take")
    if C < 1 or m < 1 or not overlap >= 0.0:
        raise ValueError("build_local_bases: n_clusters and num_global_modes must be positive, overlap non-negative")
    if n_modes is None and epsilon_squared is None:
        raise ValueError("build_local_bases: give epsilon_squared or n_modes")
    widths = None if n_modes is None else ([int(n_modes)] * C if np.ndim(n_modes) == 0 else [int(v) for v in n_modes])
    if widths is not None and len(widths) != C:
        raise ValueError(f"n_modes must be an int or one per cluster ({C})")
    _require_finite(S, "build_local_bases")
    if U_global is None:
        U_global = thin_svd(S)[0]
    else:
        U_global = torch.as_tensor(U_global).to(device=S.device, dtype=torch.float64)
    if U_global.dim() != 2 or U_global.shape[0] != N or U_global.shape[1] < m:
        raise ValueError(f"U_global must be (N, >= num_global_modes) with N = {N}, num_global_modes = {m}")
    Q = (U_global[:, :m].t() @ S).t().contiguous()
    km = kmeans(Q, C, init=init, seed=seed, max_iter=max_iter)
    labels, _, bits, _ = _assign(Q, km.centres, overlap=overlap, labels=km.labels)
    columns = [torch.nonzero(member_mask(bits, c))[:, 0] for c in range(C)]
    counts = [int(ix.numel()) for ix in columns]
    for c, n in enumerate(counts):
        if n == 0:
            raise ValueError(f"build_local_bases: cluster {c} has no snapshots (no label and nothing within the overlap)")
    U_of, s_of, sweeps = {}, {}, {}
    big = [c for c in range(C) if counts[c] >= N] if (batched and S.is_cuda) else []
    if big:
        cores = torch.stack([torch.linalg.qr(S[:, columns[c]].t(), mode="reduced")[1] for c in big])
        inf = {}
        _, sb, Vhb = jacobi_svd_batched(cores, info=inf)
        for k, c in enumerate(big):
            U_of[c], s_of[c], sweeps[c] = Vhb[k].t().contiguous(), sb[k], inf["sweeps"][k]
    for c in range(C):
        if c not in U_of:
            inf = {}
            U_of[c], s_of[c], _ = thin_svd(S[:, columns[c]], info=inf)
            sweeps[c] = inf.get("sweeps")
    bases = {}
    for c in range(C):
        if widths is not None:
            K = widths[c]
        else:
            K = n_modes_for_tolerance(s_of[c], epsilon_squared)
            K = K if max_modes is None else min(K, int(max_modes))
        if K < 1 or K > U_of[c].shape[1] or not float(s_of[c][K - 1]) > 0.0:
            raise ValueError(f"build_local_bases: cluster {c} cannot give {K} modes ({counts[c]} snapshots, rank "
                             f"{int((s_of[c] > 0).sum())})")
        bases[c] = U_of[c][:, :K].contiguous()
    if info is not None:
        info["sweeps"], info["batched"] = sweeps, big
    return LocalBases(km.centres, bases, U_global, m, labels, bits, counts, s_of, overlap, km)


# ---- .npy contracts --------------------------------------------------------------------------
def snapshot_filename(mu1, mu2):
    return f"fem_simulation_mu1_{mu1:.3f}_mu2_{mu2:.4f}.npy"          # paper_training_stage.py:52


def save_snapshots(directory, snaps, mu1, mu2):
    """Write one C-ordered (N, nT+1) float64 .npy per sample, named like the reference."""
    os.makedirs(directory, exist_ok=True)
    snaps = snaps.detach().cpu().numpy() if isinstance(snaps, torch.Tensor) else np.asarray(snaps)
    paths = []
    for U, a, b in zip(snaps, np.atleast_1d(mu1), np.atleast_1d(mu2)):
        p = os.path.join(directory, snapshot_filename(float(a), float(b)))
        np.save(p, np.ascontiguousarray(U, dtype=np.float64))
        paths.append(p)
    return paths


def save_modes(directory, U, s, eps2):
    """U_modes_tol_{eps2:.0e}.npy and Singular_values_modes_tol_{eps2:.0e}.npy (POD/pod.py:73-76)."""
    os.makedirs(directory, exist_ok=True)
    pu = os.path.join(directory, f"U_modes_tol_{eps2:.0e}.npy")
    ps = os.path.join(directory, f"Singular_values_modes_tol_{eps2:.0e}.npy")
    np.save(pu, np.ascontiguousarray(U.detach().cpu().numpy(), dtype=np.float64))
    np.save(ps, np.ascontiguousarray(s.detach().cpu().numpy(), dtype=np.float64))
    return pu, ps


def save_local_bases(directory, result):
    """A LocalBases as .npy / .npz files (no pickles): centres.npy, U_global.npy, labels.npy, member_bits.npy,
    local_bases.npz and singular_values.npz (one array per cluster, named by its id) and clustering.npz (the scalars).
    Returns the directory."""
    os.makedirs(directory, exist_ok=True)
    host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())
    np.save(os.path.join(directory, "centres.npy"), host(result.centres))
    np.save(os.path.join(directory, "U_global.npy"), host(result.U_global))
    np.save(os.path.join(directory, "labels.npy"), host(result.labels))
    np.save(os.path.join(directory, "member_bits.npy"), host(result.member_bits))
    np.savez(os.path.join(directory, "local_bases.npz"), **{str(c): host(b) for c, b in result.local_bases.items()})
    np.savez(os.path.join(directory, "singular_values.npz"), **{str(c): host(v) for c, v in result.singular_values.items()})
    km = result.kmeans
    np.savez(os.path.join(directory, "clustering.npz"), num_global_modes=np.int64(result.num_global_modes),
             member_counts=np.asarray(result.member_counts, dtype=np.int64), overlap=np.float64(result.overlap),
             n_iter=np.int64(km.n_iter), converged=np.bool_(km.converged), inertia=np.float64(km.inertia),
             changed=np.asarray(km.changed, dtype=np.int64))
    return directory


def load_local_bases(directory, device="cpu"):
    """The LocalBases save_local_bases wrote, as tensors on ``device``."""
    load = lambda name: np.load(os.path.join(directory, name), allow_pickle=False)
    dev = lambda a: torch.as_tensor(a).to(device)
    with load("local_bases.npz") as z:
        bases = {int(k): dev(z[k]).contiguous() for k in z.files}
    with load("singular_values.npz") as z:
        svals = {int(k): dev(z[k]) for k in z.files}
    with load("clustering.npz") as z:
        meta = {k: z[k] for k in z.files}
    centres, labels = dev(load("centres.npy")), dev(load("labels.npy"))
    km = KMeansResult(centres, labels, int(meta["n_iter"]), bool(meta["converged"]), float(meta["inertia"]), meta["changed"].tolist())
    return LocalBases(centres, dict(sorted(bases.items())), dev(load("U_global.npy")), int(meta["num_global_modes"]), labels,
                      dev(load("member_bits.npy")), meta["member_counts"].tolist(), dict(sorted(svals.items())),
                      float(meta["overlap"]), km)
