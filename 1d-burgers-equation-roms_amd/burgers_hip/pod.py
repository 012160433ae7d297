"""Offline basis builders on torch tensors (device or CPU) and the reference's .npy contracts.

  POD basis           POD/pod.py:8-14 (energy rule), :68-90 (thin SVD, file names)
  quadratic manifold  Quadratic_manifold/build_quadratic_manifold.py:25-48, quad_utils.py:63-81
  local POD           what FEMBurgers.local_prom_burgers consumes (FEM/fem_burgers.py:979-1079): k-means centres in global
                      POD coordinates and one overlapping basis per cluster (kmeans, build_local_bases)
  POD-RBF closure     what FEMBurgers.pod_rbf_prom consumes (FEM/fem_burgers.py:1278-1398): scaled centres, ranges and the
                      ridge-fitted weights (rbf_kernel_matrix, spd_solve, fit_rbf_weights, build_rbf_closure)
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


def _jacobi(Rs, tol, max_sweeps, who, late):
    """One-sided Jacobi on the HIP kernel of bg_jacobi_sweep_batched: the SVD of every matrix of the finite (count, m, m)
    device tensor ``Rs``.  Returns stacked U, s, Vh with R = U diag(s) Vh, s descending, per matrix the sweep that made no
    rotation, and the rotation counts per sweep and matrix.  The rotations act on the ROWS of R, i.e. on the columns of
    R^T: R^T J = W with orthogonal columns  =>  R = J (W^T): left vectors J, right W/|W|.

    Before every sweep, rows whose squared norm is at or below (eps |R|_F)^2 are set to zero: they hold rounding
    noise of the input, which rotations against the large rows keep regenerating above the relative tol, so a
    rank-deficient core otherwise rotates forever (N x 808 bench gather: ~4800 rotations in every sweep).  Their
    singular values come back 0 and their rows of Vh zero; the kernel skips every pair holding a zero row.  A
    floor of m eps |R|_F would also converge but moves the modes near sigma/sigma_1 = 1e-7 by 4e-7 (measured).
    Graded cores of condition 1e10 need up to ~46 sweeps at m = 512..777.  The floor and the rotation count are per matrix;
    a matrix that has converged makes no rotation in the sweeps the others still need.  A sweep that still rotates at
    max_sweeps raises RuntimeError: ``who``, then ``late(counts)`` on the matrices at fault."""
    from . import lib as _lib
    L = _lib.load()
    count, m = Rs.shape[0], Rs.shape[1]
    G = Rs.contiguous().clone()
    Jt = torch.eye(m, dtype=torch.float64, device=Rs.device).repeat(count, 1, 1)
    pairs = _round_robin(m).to(Rs.device)
    rot = torch.zeros((count,), dtype=torch.int32, device=Rs.device)
    eps = torch.finfo(torch.float64).eps
    # (every per-matrix reduction runs on a copy of that matrix: one shape and alignment whatever the batch, hence one set of bits)
    floor = torch.stack([(eps * torch.linalg.matrix_norm(G[k].clone())) ** 2 for k in range(count)]).reshape(count, 1, 1)
    n_rot, sweeps, history = [0] * count, [0] * count, []
    with torch.cuda.device(Rs.device):
        for sweep in range(1, (max_sweeps if count else 0) + 1):
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
        raise RuntimeError(f"{who}: not converged after {max_sweeps} sweeps (m = {m}{late(n_rot)})")
    U, S, Vh = torch.empty_like(G), torch.empty((count, m), dtype=torch.float64, device=Rs.device), torch.empty_like(G)
    tiny = torch.finfo(torch.float64).tiny
    for k in range(count):
        Gk, Jk = G[k].clone(), Jt[k].clone()
        s = torch.linalg.vector_norm(Gk, dim=1)
        order = torch.argsort(s, descending=True)
        s, Gk, Jk = s[order], Gk[order], Jk[order]
        U[k], S[k], Vh[k] = Jk.t(), s, Gk / torch.clamp(s, min=tiny)[:, None]
    return U, S, Vh, sweeps, history


def jacobi_svd(R, tol=1e-15, max_sweeps=80, info=None):
    """SVD of a square device matrix by one-sided Jacobi (_jacobi on the batch of this one matrix): U, s, Vh with
    R = U diag(s) Vh, s descending.  A sweep that still rotates at max_sweeps raises RuntimeError; NaN / Inf input raises
    LinAlgError.  ``info`` (a dict) receives the sweep count."""
    _require_finite(R, "jacobi_svd")
    U, s, Vh, sweeps, _ = _jacobi(R[None], tol, max_sweeps, "jacobi_svd", lambda n: f", {n[0]} rotations in the last")
    if info is not None:
        info["sweeps"] = sweeps[0]
    return U[0], s[0], Vh[0]


def jacobi_svd_batched(Rs, tol=1e-15, max_sweeps=80, info=None):
    """jacobi_svd of every matrix of the (count, m, m) device tensor ``Rs`` in the launches of one: stacked U, s, Vh, bitwise
    what jacobi_svd returns for each matrix alone.  Raises RuntimeError naming the matrices that still rotate at
    ``max_sweeps``; NaN / Inf raises LinAlgError.  ``info`` (a dict) receives ``sweeps`` (per matrix, the sweep that made no
    rotation) and ``rotations`` (one list per sweep, one count per matrix)."""
    _require_finite(Rs, "jacobi_svd_batched")
    if Rs.dim() != 3 or Rs.shape[1] != Rs.shape[2]:
        raise ValueError("jacobi_svd_batched takes a (count, m, m) tensor")
    late = lambda n_rot: "; " + ", ".join(f"matrix {k}: {n} rotations in the last" for k, n in enumerate(n_rot) if n)
    U, s, Vh, sweeps, history = _jacobi(Rs, tol, max_sweeps, "jacobi_svd_batched", late)
    if info is not None:
        info["sweeps"], info["rotations"] = sweeps, history
    return U, s, Vh


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


# ---- what the builders below share ----------------------------------------------------------------------------------------
def _global_basis(S, U, cols, message):
    """The global basis of the snapshots ``S``: ``U`` on S's device as float64, or thin_svd(S)[0]; (N, >= cols) or ValueError."""
    U = thin_svd(S)[0] if U is None else torch.as_tensor(U).to(device=S.device, dtype=torch.float64)
    if U.dim() != 2 or U.shape[0] != S.shape[0] or U.shape[1] < cols:
        raise ValueError(message)
    return U


def _coordinates(Phi, S):
    """(Phi^T S)^T contiguous: the coordinates of the snapshots in the columns ``Phi`` of a basis, one row per snapshot."""
    return (Phi.t() @ S).t().contiguous()


def _check_ridge(ridge):
    if not (ridge >= 0.0 and np.isfinite(ridge)):
        raise ValueError("ridge must be a non-negative finite number")


def _check_solver(solver):
    if solver not in ("cholesky", "library"):
        raise ValueError("solver must be 'cholesky' or 'library'")


_host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())                          # a tensor as the array np.save gets
_host_matrix = lambda A: np.ascontiguousarray(_host64(A))


def _host64(A):
    """A tensor or an array as a float64 host array, its layout kept."""
    return np.asarray(A.detach().cpu() if isinstance(A, torch.Tensor) else A, dtype=np.float64)
_npy = lambda directory, name: np.load(os.path.join(directory, name), allow_pickle=False)  # .npy / .npz, never a pickle


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
        t = torch.as_tensor(np.atleast_2d(_host64(q)))
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
    U_global = _global_basis(S, U_global, m, f"U_global must be (N, >= num_global_modes) with N = {N}, num_global_modes = {m}")
    Q = _coordinates(U_global[:, :m], S)
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


# ---- POD-RBF: the closure's centres, scaling and ridge fit ---------------------------------------------------------------
RBF_KERNELS = ("gaussian", "imq")                          # index = BG_RBF_GAUSSIAN, BG_RBF_IMQ


def _rbf_kind(kernel):
    """BG_RBF_GAUSSIAN or BG_RBF_IMQ of a kernel name; the one place that knows the names (rom.RbfClosure asks here)."""
    if kernel not in RBF_KERNELS:
        raise ValueError("kernel must be 'gaussian' or 'imq'.")
    return RBF_KERNELS.index(kernel)


def _rbf_range(lo, hi):
    """hi - lo with entries below 1e-15 replaced by 1: the closure's scaling guard, in its fit and in rom.RbfClosure alike."""
    d = hi - lo
    d[d < 1e-15] = 1.0
    return d


def _chol_max_n():
    from . import lib as _lib
    return int(_lib.load().bg_chol_max_n())


def _check_order(Ns, who):
    if Ns > _chol_max_n():
        raise ValueError(f"{who}: {Ns} centres, beyond the {_chol_max_n()} of bg_chol_max_n (subsample with `centres`)")


def rbf_kernel_matrix(Xs, epsilon, kernel, ridge=0.0):
    """The (Ns, Ns) matrix k(eps |x_i - x_j|) + ridge I of the scaled centres ``Xs`` (Ns, n): gaussian exp(-eps^2 r^2) or imq
    (1 + eps^2 r^2)^(-1/2), r^2 summed over the coordinates in their order -- the forms of the closure's evaluation
    (csrc/rbf_device.hpp).  Device tensors: bg_rbf_gram (both triangles bit for bit equal, the diagonal 1 + ridge exactly).  CPU
    tensors: the same direct sum in torch."""
    kind = _rbf_kind(kernel)
    if Xs.dim() != 2 or Xs.shape[0] < 1 or Xs.shape[1] < 1:
        raise ValueError("rbf_kernel_matrix takes the scaled centres as the rows of a (Ns, n) tensor")
    _check_ridge(ridge)
    Xs = Xs.to(torch.float64)
    Ns, n = Xs.shape
    _check_order(Ns, "rbf_kernel_matrix")
    eps2 = float(epsilon) * float(epsilon)
    if not Xs.is_cuda:
        r2 = torch.zeros((Ns, Ns), dtype=torch.float64)
        for k in range(n):
            d = Xs[:, None, k] - Xs[None, :, k]
            r2 += d * d
        A = torch.exp(-eps2 * r2) if kind == 0 else 1.0 / torch.sqrt(1.0 + eps2 * r2)
        A.diagonal().fill_(1.0 + float(ridge))
        return A
    from . import lib as _lib
    XtT = Xs.t().contiguous()
    A = torch.empty((Ns, Ns), dtype=torch.float64, device=Xs.device)
    with torch.cuda.device(Xs.device):
        _lib.check(_lib.load().bg_rbf_gram(Ns, n, kind, float(epsilon), float(ridge), _lib.ptr(XtT), _lib.ptr(A), Ns,
                                           _lib.stream_ptr(Xs.device)), "bg_rbf_gram")
    return A


def _spd_solve(A, Y, info, overwrite):
    """spd_solve on a float64 matrix the caller gives up when ``overwrite`` (its lower triangle becomes the factor)."""
    if A.dim() != 2 or A.shape[0] != A.shape[1] or Y.shape[0] != A.shape[0] or Y.dim() not in (1, 2):
        raise ValueError("spd_solve takes an (n, n) matrix and an (n,) or (n, nrhs) right-hand side")
    if Y.device != A.device:
        raise ValueError(f"spd_solve: the matrix lives on {A.device}, the right-hand side on {Y.device}")
    _require_finite(Y, "spd_solve (right-hand side)")
    n = A.shape[0]
    B = Y.to(torch.float64).reshape(n, -1).contiguous().clone()
    if not A.is_cuda:
        L, bad = torch.linalg.cholesky_ex(A)
        bad = int(bad)
    else:
        from . import lib as _lib
        lib = _lib.load()
        _check_order(n, "spd_solve")
        L = A if (overwrite and A.is_contiguous()) else A.contiguous().clone()
        flag = torch.zeros((1,), dtype=torch.int32, device=A.device)
        with torch.cuda.device(A.device):
            _lib.check(lib.bg_chol_factor(n, _lib.ptr(L), n, _lib.ptr(flag), _lib.stream_ptr(A.device)), "bg_chol_factor")
            bad = int(flag.item()) if n else 0
    if info is not None:
        info["info"] = bad
    if bad:
        raise np.linalg.LinAlgError(f"spd_solve: pivot {bad - 1} of the Cholesky factorisation is not a positive finite number "
                                    f"(info = {bad}): the matrix is not positive definite to rounding; a larger ridge makes it so")
    if not A.is_cuda:
        X = torch.cholesky_solve(B, L)
    else:
        with torch.cuda.device(A.device):
            _lib.check(lib.bg_chol_solve(n, B.shape[1], _lib.ptr(L), n, _lib.ptr(B), B.shape[1], _lib.stream_ptr(A.device)),
                       "bg_chol_solve")
        X = B
    return X.reshape(Y.shape)


def spd_solve(A, Y, info=None):
    """W with A W = Y for a symmetric positive definite float64 ``A`` (n, n), of which only the lower triangle is read, and
    ``Y`` (n,) or (n, nrhs); A is left as it is.  Device tensors: the blocked Cholesky bg_chol_factor, one int read back after
    it (as jacobi_svd reads its rotation count), then bg_chol_solve -- no workspace beyond the copy of A, bitwise reproducible,
    and a column of W does not depend on the other columns of Y.  CPU tensors: torch.linalg.cholesky_ex + cholesky_solve.
    A pivot that is not a positive finite number raises LinAlgError naming it; NaN / Inf in Y raises LinAlgError; an order
    beyond bg_chol_max_n raises ValueError on the device.  ``info`` (a dict) receives LAPACK's ``info`` (0, or pivot + 1)."""
    return _spd_solve(A.to(torch.float64), Y, info, overwrite=False)


def backward_error(A, W, Y):
    """|A W - Y|_F / (|A|_2 |W|_F + |Y|_F) of a symmetric positive semi-definite ``A``.  |A|_2 is the Rayleigh quotient after
    30 power iterations from the vector of ones: at most the norm, so the figure errs upwards.  A kernel matrix has positive
    entries and a dominant Perron value, which the quotient meets to well below a percent."""
    W2, Y2 = W.reshape(A.shape[0], -1), Y.reshape(A.shape[0], -1)
    v = torch.ones((A.shape[0],), dtype=A.dtype, device=A.device)
    for _ in range(30):
        v = A @ (v / torch.linalg.vector_norm(v))
    v = v / torch.linalg.vector_norm(v)
    norm2 = float(torch.dot(v, A @ v))
    return float(torch.linalg.matrix_norm(A @ W2 - Y2)) / (norm2 * float(torch.linalg.matrix_norm(W2)) + float(torch.linalg.matrix_norm(Y2)))


def fit_rbf_weights(Xs, Ys, epsilon, kernel="gaussian", ridge=1e-8, solver="cholesky", info=None):
    """The closure weights W (Ns, nbar): (K + ridge I) W = Ys over the scaled centres ``Xs`` (Ns, n) and scaled targets ``Ys``
    (Ns, nbar), K = rbf_kernel_matrix(Xs, epsilon, kernel).  ``solver``: "cholesky" is spd_solve (in-tree on the device);
    "library" is torch.linalg.solve (LU) on the same matrix, kept for A/B runs and never the default.  ``info`` (a dict)
    receives ``backward_error`` (see backward_error; costs a copy of the matrix) and, from the Cholesky route, ``info``."""
    _check_solver(solver)
    if Xs.dim() != 2 or Ys.dim() != 2 or Ys.shape[0] != Xs.shape[0] or Ys.device != Xs.device:
        raise ValueError("fit_rbf_weights takes Xs (Ns, n) and Ys (Ns, nbar) on one device")
    Ys = Ys.to(torch.float64)
    A = rbf_kernel_matrix(Xs, epsilon, kernel, ridge)
    if solver == "library":
        _require_finite(Ys, "fit_rbf_weights (targets)")
        W = torch.linalg.solve(A, Ys)
    else:
        W = _spd_solve(A, Ys, info, overwrite=info is None)
    if info is not None:
        info["backward_error"] = backward_error(A, W, Ys)
    return W


class RbfFit:
    """What build_rbf_closure returns and save_rbf_closure stores: the bases ``U_p`` (N, n) and ``U_s`` (N, nbar), the scaled
    centres ``X_train`` (Ns, n), the weights ``W`` (Ns, nbar), ``epsilon``, ``kernel``, the scaling ranges ``x_min, x_max``
    (n,) and ``y_min, y_max`` (nbar,) over all snapshots, ``ridge``, ``centre_index`` (Ns,) int64 (the snapshot columns taken
    as centres) and ``backward_error`` of the ridge system (see backward_error).  Tensors live on the device of the snapshots."""

    def __init__(self, U_p, U_s, X_train, W, epsilon, kernel, x_min, x_max, y_min, y_max, ridge, centre_index, backward_error):
        self.U_p, self.U_s, self.X_train, self.W = U_p, U_s, X_train, W
        self.epsilon, self.kernel, self.ridge = float(epsilon), str(kernel), float(ridge)
        self.x_min, self.x_max, self.y_min, self.y_max = x_min, x_max, y_min, y_max
        self.centre_index, self.backward_error = centre_index, float(backward_error)

    def prom_args(self):
        """(U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max): the positional operands of
        FEMBurgers.pod_rbf_prom and rom.pod_rbf_run after the initial condition and parameters (pass ``kernel=fit.kernel``
        beside them).  The bases stay where they are; the closure's own operands go as host arrays, which is how
        rom.RbfClosure takes them."""
        return (self.U_p, self.U_s, _host(self.X_train), _host(self.W), self.epsilon, _host(self.x_min), _host(self.x_max),
                _host(self.y_min), _host(self.y_max))


def _centre_rows(centres, Ns_all):
    if centres is None:
        return np.arange(Ns_all)
    if np.ndim(centres) == 0:
        k = int(centres)
        if k < 1 or k > Ns_all:
            raise ValueError(f"build_rbf_closure: {k} centres of {Ns_all} snapshots")
        return np.linspace(0, Ns_all - 1, k).astype(int)
    idx = np.asarray(centres.detach().cpu() if isinstance(centres, torch.Tensor) else centres).astype(np.int64).reshape(-1)
    if idx.size < 1 or idx.min() < 0 or idx.max() >= Ns_all or len(np.unique(idx)) != idx.size:
        raise ValueError("build_rbf_closure: centre indices must be distinct snapshot columns")
    return idx


def build_rbf_closure(S, n, nbar, epsilon, kernel="gaussian", ridge=1e-8, centres=None, U=None, solver="cholesky"):
    """Snapshots S (N, Ns_all) -> the closure the POD-RBF PROM runs on, on S's device.

      1. U = thin_svd(S)[0] unless given; U_p its first n columns, U_s the next nbar;  2. Q = (U_p^T S)^T, Qbar = (U_s^T S)^T;
      3. x_min .. y_max: the column minima and maxima over ALL snapshots;  4. centres: every snapshot (None), the rows
      np.linspace(0, Ns_all - 1, k).astype(int) (an int k) or the given distinct indices;  5. Xs = 2 (Q[idx] - x_min)/dx - 1,
      Ys likewise with dy, ranges below 1e-15 replaced by 1 -- the guard and arithmetic of the closure's evaluation
      (rom.RbfClosure, csrc/rbf.hip);  6. W = fit_rbf_weights(Xs, Ys, epsilon, kernel, ridge, solver).
    This is the rule of this project's golden-fixture generator (tests/golden/make_golden.py fx_rbf), which solves the ridge
    system by LU; the matrix is symmetric positive definite and the builder factors it by Cholesky (bg_chol_factor).

    Any n and nbar are taken: the host-driven PROM has no limits of its own, while ``fused=True`` runs the device-side loop
    only within bg_rbf_rom_limits (N <= 512, n <= 20, nbar <= 128, 65536 centres) and otherwise the host-driven iteration.
    An unknown kernel or solver, n + nbar beyond the singular vectors at hand, an integer ``centres`` above Ns_all or indices
    with duplicates, a negative ridge and more centres than bg_chol_max_n raise ValueError; a ridge too small for the matrix
    to be positive definite to rounding raises LinAlgError.  Returns an RbfFit."""
    _rbf_kind(kernel)
    _check_solver(solver)
    if S.dim() != 2:
        raise ValueError("build_rbf_closure takes the (N, Ns) snapshot matrix")
    _check_ridge(ridge)
    n, nbar = int(n), int(nbar)
    N, Ns_all = S.shape
    if n < 1 or nbar < 1 or n + nbar > (min(N, Ns_all) if U is None else int(np.shape(U)[1])):
        raise ValueError(f"build_rbf_closure: n = {n} and nbar = {nbar} need {n + nbar} singular vectors")
    idx = _centre_rows(centres, Ns_all)
    _check_order(len(idx), "build_rbf_closure")
    S = S.to(torch.float64)
    _require_finite(S, "build_rbf_closure")
    U = _global_basis(S, U, n + nbar, f"U must be (N, >= n + nbar) with N = {N}")
    U_p, U_s = U[:, :n].contiguous(), U[:, n:n + nbar].contiguous()
    Q, Qb = _coordinates(U_p, S), _coordinates(U_s, S)
    x_min, x_max, y_min, y_max = Q.min(0).values, Q.max(0).values, Qb.min(0).values, Qb.max(0).values
    dx, dy = _rbf_range(x_min, x_max), _rbf_range(y_min, y_max)
    rows = torch.as_tensor(idx, device=S.device)
    Xs = (2.0 * ((Q[rows] - x_min) / dx) - 1.0).contiguous()
    Ys = (2.0 * ((Qb[rows] - y_min) / dy) - 1.0).contiguous()
    info = {}
    W = fit_rbf_weights(Xs, Ys, epsilon, kernel, ridge, solver, info=info)
    return RbfFit(U_p, U_s, Xs, W, epsilon, kernel, x_min, x_max, y_min, y_max, ridge, rows.to(torch.int64), info["backward_error"])


# ---- row sampling for the hyper-reduced POD PROM (rom.pod_prom_run_hyper, bg_hyper_rom_run) ----
class RowSampling:
    """What build_row_sampling returns and save_row_sampling stores: the sampled mesh ``rows`` (m,) int32, ascending, row 0
    among them; their weights ``xi`` (m,) float64 >= 0 (row 0: 1); the ``projection`` they were trained for ("galerkin" or
    "lspg"); ``residual`` = |G xi - d| / |d| on the training data, ``pairs`` the number of training pairs and ``tau`` the
    bound asked for.  The tensors live on the host."""

    def __init__(self, rows, xi, projection, residual, pairs, tau):
        self.rows, self.xi = torch.as_tensor(rows, dtype=torch.int32), torch.as_tensor(xi, dtype=torch.float64)
        self.projection, self.residual, self.pairs, self.tau = str(projection), float(residual), int(pairs), float(tau)

    @property
    def m(self):
        return int(self.rows.numel())


_GP_A, _GP_B = 0.5 * (1.0 + 1.0 / np.sqrt(3.0)), 0.5 * (1.0 - 1.0 / np.sqrt(3.0))      # P1 shape values at the two Gauss points


def picard_rows(X, U0, Un, mu1, mu2, dt, E=0.0, supg=True):
    """The three diagonals lo, di, up of the Picard matrix A(U0) = M + dt C(U0) + dt E K with the Dirichlet row 0, and
    R = A U0 - b, b = M Un + dt F - dt S(U0), b[0] = mu1 (FEM/fem_burgers.py:730-753), for one state on the host: the closed
    forms of the two-point Gauss rule on P1 elements, in numpy.  This is training arithmetic for build_row_sampling, not a
    stepper: the device kernels assemble their own rows."""
    X, U0, Un = (np.asarray(v, dtype=np.float64) for v in (X, U0, Un))
    N = len(X)
    h = np.diff(X)
    ul, ur = U0[:-1], U0[1:]
    a, b = (2.0 * ul + ur) / 6.0, (ul + 2.0 * ur) / 6.0         # int N_l u, int N_r u over the element, divided by h
    off, dd = h / 6.0 - dt * E / h, h / 3.0 + dt * E / h
    lo, di, up = np.zeros(N), np.zeros(N), np.zeros(N)
    di[:-1] += dd - dt * a
    di[1:] += dd + dt * b
    up[:-1] = off + dt * a
    lo[1:] = off - dt * b
    xl, xr = X[:-1], X[1:]
    f1 = 0.02 * np.exp(mu2 * (_GP_A * xl + _GP_B * xr))
    f2 = 0.02 * np.exp(mu2 * (_GP_B * xl + _GP_A * xr))
    rhs = np.zeros(N)
    rhs[:-1] += h / 6.0 * (2.0 * Un[:-1] + Un[1:]) + dt * (f1 * _GP_A + f2 * _GP_B) * (0.5 * h)
    rhs[1:] += h / 6.0 * (Un[:-1] + 2.0 * Un[1:]) + dt * (f1 * _GP_B + f2 * _GP_A) * (0.5 * h)
    if supg:
        ue = 0.5 * (ul + ur)
        tau_e = 0.5 * h / (2.0 * np.maximum(np.abs(ue), 1.0e-10))
        s = 0.5 * tau_e * ((ul + ur) * (ur - ul) / h - (f1 + f2))
        rhs[:-1] += dt * s
        rhs[1:] -= dt * s
    lo[0], di[0], up[0], rhs[0] = 0.0, 1.0, 0.0, mu1
    R = di * U0 - rhs
    R[1:] += lo[1:] * U0[:-1]
    R[:-1] += up[:-1] * U0[1:]
    return lo, di, up, R


def row_contributions(X, Phi, U0, Un, mu1, mu2, dt, projection, E=0.0, supg=True):
    """(r, N): column i is c_i = w_i R_i, the share of mesh row i in the reduced right-hand side br = sum_i c_i at the state
    U0 (previous step Un); w_i = Phi[i] for "galerkin", (A Phi)[i] for "lspg"."""
    lo, di, up, R = picard_rows(X, U0, Un, mu1, mu2, dt, E, supg)
    W = Phi
    if projection == "lspg":
        W = di[:, None] * Phi
        W[1:] += lo[1:, None] * Phi[:-1]
        W[:-1] += up[:-1, None] * Phi[1:]
    return (W * R[:, None]).T


def _no_column_left(count, rel, tau, min_cols, dependent=0):
    """``dependent``: the candidates nnls_rows_device found numerically dependent on the active columns, named when there are any."""
    why = "" if not dependent else (f"; {dependent} candidates were numerically dependent on the active columns: ``min_rows`` is "
                                    f"beyond the numerical rank of the training matrix, ask for fewer rows or use solver='host'")
    return ValueError(f"row sampling: no column left to add at {count} columns, residual {rel:.2e} "
                      f"(asked: {tau:.1e}, at least {min_cols} columns){why}")


def _too_many_rows(rel, tau, min_cols, max_cols):
    return ValueError(f"row sampling: more than max_rows = {max_cols + 1} rows needed (residual {rel:.2e} at that "
                      f"point, asked: {tau:.1e} with at least {min_cols + 1} rows)")


def nnls_rows(G, d, tau, min_cols, max_cols):
    """Active-set NNLS (Lawson-Hanson) for min |G x - d|, x >= 0, stopped as soon as |G x - d| <= tau |d|; after that the
    same greedy rule (the column with the largest gradient G^T (d - G x)) goes on adding columns until ``min_cols`` are
    active.  ValueError when ``max_cols`` would be exceeded or no column is left to add.  Returns (x, relative residual)."""
    n = G.shape[1]
    x = np.zeros(n)
    active = np.zeros(n, dtype=bool)
    tabu = np.zeros(n, dtype=bool)                 # fill phase: columns the least-squares fit threw out again
    dn = float(np.linalg.norm(d))
    res = d.copy()
    for _ in range(3 * n + 10):
        rel = float(np.linalg.norm(res)) / dn if dn > 0.0 else 0.0
        fit_done = rel <= tau
        if fit_done and int(active.sum()) >= min_cols:
            return x, rel
        w = G.T @ res
        w[active | tabu] = -np.inf
        j = int(np.argmax(w))
        if not np.isfinite(w[j]) or (not fit_done and w[j] <= 0.0):
            raise _no_column_left(int(active.sum()), rel, tau, min_cols)
        if int(active.sum()) + 1 > max_cols:
            raise _too_many_rows(rel, tau, min_cols, max_cols)
        active[j] = True
        while True:
            idx = np.flatnonzero(active)
            s = np.linalg.lstsq(G[:, idx], d, rcond=None)[0]
            if s.min() > 0.0:
                x[:] = 0.0
                x[idx] = s
                break
            neg = s <= 0.0                            # step towards s as far as x stays non-negative, drop what reaches 0
            xa = x[idx]
            ratio = np.where(neg, xa / np.where(neg, xa - s, 1.0), np.inf)
            xa = xa + float(ratio.min()) * (s - xa)
            xa[ratio <= ratio.min()] = 0.0
            x[:] = 0.0
            x[idx] = np.maximum(xa, 0.0)
            active[idx[x[idx] <= 0.0]] = False
        if active[j] and not fit_done:
            tabu[:] = False
        elif not active[j]:
            tabu[j] = True                             # the fit threw the new column out again: not this one next time
        res = d - G[:, active] @ x[active]
    raise ValueError("row sampling: the active-set iteration did not end")


class NnlsWorkspace:
    """The device-resident state of nnls_rows_device and the entry points of csrc/nnls.hip on it (layouts:
    include/burgers_hip.h, bg_nnls_pick): ``At`` (n, ld) the columns of G, ``b``, ``res``, the thin QR ``Q`` (kmax, ld),
    ``R`` (kmax, kmax) stored by columns, ``z``, the weights ``x`` and the columns ``order`` in insertion order, the masks
    ``active`` and ``tabu`` and the 64-byte ``status``.  ``G`` (rows, n): a host array (uploaded once and transposed on the
    device) or a device tensor; ``kmax``: the most columns that may become active.  Every method queues its kernels on the
    current stream of the device; read() alone waits, and brings back the status record as a numpy record."""

    def __init__(self, G, d, kmax, device=None):
        from . import lib as _lib
        self._lib, self.L = _lib, _lib.load()
        self.device = G.device if isinstance(G, torch.Tensor) and G.is_cuda else _lib.require_device(device)
        dev, f64, i32 = self.device, torch.float64, torch.int32
        self.rows, self.n = int(G.shape[0]), int(G.shape[1])
        self.kmax = int(kmax)
        self.ld = ld = max(8, (self.rows + 7) // 8 * 8)
        self.At = torch.zeros((max(self.n, 1), ld), dtype=f64, device=dev)
        if self.n:
            self.At[:self.n, :self.rows] = torch.as_tensor(G).to(device=dev, dtype=f64).t()
        self.b = torch.zeros((ld,), dtype=f64, device=dev)
        self.b[:self.rows] = torch.as_tensor(d).to(device=dev, dtype=f64)
        self.res = self.b.clone()
        self.Q = torch.zeros((self.kmax, ld), dtype=f64, device=dev)
        self.R = torch.zeros((self.kmax, self.kmax), dtype=f64, device=dev)
        self.z = torch.zeros((self.kmax,), dtype=f64, device=dev)
        self.x = torch.zeros((self.kmax,), dtype=f64, device=dev)
        self.order = torch.zeros((self.kmax,), dtype=i32, device=dev)
        self.active = torch.zeros((max(self.n, 1),), dtype=i32, device=dev)
        self.tabu = torch.zeros((max(self.n, 1),), dtype=i32, device=dev)
        self.w = torch.zeros((max(self.n, 1),), dtype=f64, device=dev)
        self.work = torch.zeros((int(self.L.bg_nnls_work_elems(ld)),), dtype=f64, device=dev)
        self.status = torch.zeros((_lib.NNLS_STATUS.itemsize,), dtype=torch.uint8, device=dev)

    def _call(self, name, *args):
        with torch.cuda.device(self.device):
            self._lib.check(getattr(self.L, name)(*args, self._lib.stream_ptr(self.device)), name)

    def residual(self, k):
        p = self._lib.ptr
        self._call("bg_nnls_residual", self.rows, self.ld, int(k), p(self.At), p(self.b), p(self.x), p(self.order), p(self.res))

    def pick(self, dnorm, tau, min_cols, max_cols):
        p = self._lib.ptr
        self._call("bg_nnls_pick", self.rows, self.n, self.ld, p(self.At), p(self.res), p(self.active), p(self.tabu), float(dnorm),
                   float(tau), int(min_cols), int(max_cols), p(self.w), p(self.status))

    def append(self, k, rebuild=False):
        p = self._lib.ptr
        self._call("bg_nnls_append", self.rows, self.ld, int(k), int(bool(rebuild)), p(self.At), p(self.b), p(self.Q), p(self.R),
                   self.kmax, p(self.z), p(self.x), p(self.order), p(self.active), p(self.tabu), p(self.work), p(self.status))

    def solve(self, k):
        p = self._lib.ptr
        self._call("bg_nnls_solve", int(k), p(self.R), self.kmax, p(self.z), p(self.x), p(self.order), p(self.active), p(self.status))

    def mark(self, j, value):
        self._call("bg_nnls_mark", self.n, self._lib.ptr(self.tabu), int(j), int(value))

    def read(self):
        return np.frombuffer(self.status.cpu().numpy().tobytes(), dtype=self._lib.NNLS_STATUS)[0]


def nnls_rows_device(G, d, tau, min_cols, max_cols, device=None, info=None):
    """nnls_rows on the device (csrc/nnls.hip): the same active-set iteration, decision for decision, with the least-squares
    fit of the active columns kept as a thin QR on the device -- appended to by two passes of classical Gram-Schmidt, rebuilt
    from the first dropped position when columns leave -- where nnls_rows factors the whole active block anew at every step.
    ``G`` (rows, n): a host array (uploaded once) or a device tensor; ``d`` (rows,).  Per outer step the gradient pass reads G
    once and the append reads Q four times; one 64-byte status record comes back per least-squares solve and nothing else
    until the weights at the end.  A picked column whose remainder after the two passes is at most
    BG_NNLS_DEPENDENT_MULTIPLE machine epsilons of its norm is numerically dependent on the active ones: it is not appended
    and is tabu, which stands for the case in which nnls_rows' fit throws the new column out again.
    The same two ValueErrors as nnls_rows; ``max_cols`` or n beyond nnls_limits is a ValueError before anything is launched.
    WHERE IT PARTS FROM nnls_rows: the two pick the same columns as long as the data decide the picks (all test fixtures; N = 1024,
    r = 40 and the fit phase at N = 4096, r = 96: DESIGN K28).  Once the active columns fit d to rounding, the other columns of such
    a G are within the dependence cut of their span.  nnls_rows' lstsq (minimum norm) still adds them and shares the weight;
    this routine does not, so a ``min_cols`` beyond the numerical rank of G ends in "no column left to add" here, the message naming
    the dependent candidates, where nnls_rows returns (N = 4096, r = 96 at the default 3 r = 288 rows: refused at 202 / 198
    columns), and a fill that rounding orders (``min_cols`` near that rank) may return other columns than nnls_rows does.
    ``info``: a dict that receives adds, drops, dependent, solves and min_ratio (the smallest |v| / |G[:, j]| appended).
    Returns (x, relative residual), x a host float64 array of length n.  Two calls on the same input give the same bits."""
    from . import lib as _lib
    rows, n = int(G.shape[0]), int(G.shape[1])
    tau, min_cols, max_cols = float(tau), int(min_cols), int(max_cols)
    max_active, limit_cols = nnls_limits()
    if max_cols > max_active or n > limit_cols:
        raise ValueError(f"nnls_rows_device: beyond bg_nnls_limits: max_cols {max_cols} (<= {max_active}), {n} columns (<= {limit_cols})")
    ws = NnlsWorkspace(G, d, max(1, min(max_cols, n)), device)
    dn = float(np.linalg.norm(_host64(d)))
    counts = {} if info is None else info                     # kept up to date, so that a refusal leaves them too
    counts.update({"adds": 0, "drops": 0, "dependent": 0, "solves": 0, "min_ratio": float("inf")})
    count = 0

    def result(rel):
        x = np.zeros(n)
        x[ws.order[:count].cpu().numpy()] = ws.x[:count].cpu().numpy()
        return x, rel

    if n == 0:
        rel = 1.0 if dn > 0.0 else 0.0
        if rel <= tau and min_cols <= 0:
            return result(rel)
        raise _no_column_left(0, rel, tau, min_cols)
    for _ in range(3 * n + 10):
        ws.residual(count)
        ws.pick(dn, tau, min_cols, max_cols)                 # the loop head below, taken on the device as well: it gates
        if count < ws.kmax:                                  # the append and the solve queued behind it
            ws.append(count)
            ws.solve(count + 1)
        st = ws.read()
        rel = float(st["rel"])
        fit_done = rel <= tau
        if fit_done and count >= min_cols:
            return result(rel)
        j, wj = int(st["pick"]), float(st["w"])
        if j < 0 or not np.isfinite(wj) or (not fit_done and wj <= 0.0):
            raise _no_column_left(count, rel, tau, min_cols, counts["dependent"])
        if count + 1 > max_cols:
            raise _too_many_rows(rel, tau, min_cols, max_cols)
        if int(st["stop"]) != _lib.BG_NNLS_GO:
            raise RuntimeError(f"nnls_rows_device: the device stopped with {int(st['stop'])} where the host goes on")
        if st["dependent"]:
            counts["dependent"] += 1                         # tabu on the device already
            continue
        counts["adds"] += 1
        counts["solves"] += 1
        counts["min_ratio"] = min(counts["min_ratio"], float(st["ratio"]))
        held = count + 1
        while not st["accepted"] and int(st["count"]) > 0:
            counts["drops"] += held - int(st["count"])
            held = int(st["count"])
            for k in range(int(st["p0"]), int(st["count"])):
                ws.append(k, rebuild=True)
            ws.solve(int(st["count"]))
            st = ws.read()
            counts["solves"] += 1
            if int(st["stop"]) != _lib.BG_NNLS_GO:
                raise RuntimeError("nnls_rows_device: the repair of the QR after a drop met a dependent column")
        count = int(st["count"])
        if st["pick_active"] and not fit_done:
            ws.mark(-1, 0)
        elif not st["pick_active"]:
            ws.mark(j, 1)                                    # the fit threw the new column out again: not this one next time
    raise ValueError("row sampling: the active-set iteration did not end")


def _limits_accessor(symbol, count, doc):
    def limits():
        from . import lib as _lib
        return _lib.limits(symbol, count)
    limits.__doc__ = f"{doc}.  Needs no device."
    return limits


for _name, _symbol, _count, _doc in (
        ("hyper_rom_limits", "bg_hyper_rom_limits", 2, "(max_r, max_m) of bg_hyper_rom_run"),
        ("hyper_wide_rom_limits", "bg_hyper_rom_wide_limits", 2, "(max_r, max_m) of bg_hyper_rom_run_wide"),
        ("hyper_blocked_rom_limits", "bg_hyper_rom_blocked_limits", 2, "(max_r, max_m) of bg_hyper_rom_run_blocked"),
        ("hyper_ann_rom_limits", "bg_hyper_ann_rom_limits", 6, "(max_n, max_nbar, max_width, max_layers, max_m, max_nodes) of bg_hyper_ann_rom_run"),
        ("hyper_ann_wide_rom_limits", "bg_hyper_ann_rom_wide_limits", 6, "(max_n, max_nbar, max_width, max_layers, max_m, max_nodes) of bg_hyper_ann_rom_run_wide"),
        ("hyper_quad_rom_limits", "bg_hyper_quad_rom_limits", 3, "(max_n, max_m, max_nodes) of bg_hyper_quad_rom_run"),
        ("hyper_local_rom_limits", "bg_hyper_local_rom_limits", 4, "(max_r, max_m, max_mg, max_clusters) of bg_hyper_local_rom_run"),
        ("hyper_rbf_rom_limits", "bg_hyper_rbf_rom_limits", 5, "(max_n, max_nbar, max_ns, max_m, max_nodes) of bg_hyper_rbf_rom_run"),
        ("nnls_limits", "bg_nnls_limits", 2, "(max_active, max_cols) of the bg_nnls_* steps behind nnls_rows_device")):
    globals()[_name] = _limits_accessor(_symbol, _count, _doc)
    globals()[_name].__name__ = globals()[_name].__qualname__ = _name


def _sampling_prelude(who, X, projection, runs, tau, stride):
    """What the five build_*_row_sampling functions open with: the projection in lower case (ValueError unless Galerkin or
    LSPG), the mesh as a host array, and the refusal of no runs, stride < 1 or tau <= 0 in the name of ``who``."""
    projection = str(projection).lower()
    if projection not in ("galerkin", "lspg"):
        raise ValueError("projection must be 'Galerkin' or 'LSPG'")
    if int(stride) < 1 or not (tau > 0.0) or len(runs) < 1:
        raise ValueError(f"{who} takes at least one run, stride >= 1 and tau > 0")
    return projection, _host64(X)


def build_row_sampling(X, Phi, runs, dt, projection, E=0.0, supg=True, tau=1e-4, stride=10, min_rows=None, max_rows=None,
                       solver="host"):
    """The sampled mesh rows and weights of the hyper-reduced POD PROM (ECSW-style: energy-conserving sampling and
    weighting), fitted on the host by non-negative least squares.

    ``runs``: a list of (hist (N, nT+1), mu1, mu2), CPU or device tensors or arrays.  For every run and every ``stride``-th
    step n the pair Un = Phi Phi^T s_n, U0 = Phi Phi^T s_{n+1} gives the contributions c_i = w_i R_i (row_contributions) of
    all mesh rows to the reduced right-hand side; stacked they are G (pairs r, N), and d = G 1 is what the full sum gives.
    Row 0 (the Dirichlet row) is forced in with weight 1 and moved to the right-hand side; the other weights are
    nnls_rows(G[:, 1:], d - G[:, 0]): stopped at |G xi - d| <= tau |d|, then filled by the same greedy rule up to
    ``min_rows`` rows (default 3 r: fewer rows have diverged at r = 40 even where the training residual was met).
    ``max_rows`` defaults to the limit of the loop that takes r: hyper_rom_limits' (256) up to its r = 40, hyper_wide_rom_limits'
    (512) up to its r = 96, hyper_blocked_rom_limits' (1024) above; needing more is a ValueError.  ``solver="device"`` keeps its
    own limit: nnls_rows_device holds at most 512 active columns (nnls_limits) and refuses a ``max_rows`` beyond 513 before it
    launches anything, so with a basis of more than 96 modes it needs an explicit ``max_rows`` <= 513, and a 3 r fill beyond
    r = 171 is host work.  Returns a RowSampling.
    Two facts about wide bases, from a study at N = 600, r = 96 (3 r = 288 rows): the fill up to 3 r needs enough training
    pairs -- with three runs and stride 20 the greedy rule has no column left to add at 269, and ``min_rows`` must be given
    (200 rows stayed within 4e-11 of the full PROM there); and the NNLS is host work, about a minute at r = 96 with nine runs
    and stride 10 on eight threads (113 / 127 s per projection on 16 CPU
    threads, where ``solver="device"`` fits the first 176 / 172 rows, the host's, in 0.05 / 0.06 s against 3.0 / 2.9 s and refuses
    the fill to 288 as beyond the rank of G; at N = 1024, r = 40: the host's 123 / 120 rows in 0.06 / 0.04 s against 1.8 / 1.4 s).
    ``solver``: "host" (the default: nnls_rows, as ever) or "device" (nnls_rows_device, csrc/nnls.hip: the same iteration
    on a QR kept on the device, DESIGN K28; it refuses a ``min_rows`` beyond the numerical rank of G, see its docstring); anything
    else is a ValueError."""
    projection, X = _sampling_prelude("build_row_sampling", X, projection, runs, tau, stride)
    fit = _solver_argument(solver)
    Phi = _host_matrix(Phi)
    N = len(X)
    if Phi.ndim != 2 or Phi.shape[0] != N:
        raise ValueError("Phi must have one row per mesh node")
    r = Phi.shape[1]
    min_rows = min(3 * r, N) if min_rows is None else int(min_rows)
    if max_rows is None:
        (narrow_r, narrow_m), (wide_r, wide_m) = hyper_rom_limits(), hyper_wide_rom_limits()
        max_rows = narrow_m if r <= narrow_r else wide_m if r <= wide_r else hyper_blocked_rom_limits()[1]
    G, pairs = row_sampling_system(X, Phi, runs, dt, projection, E, supg, stride)
    return _fit_row_sampling(G, pairs, projection, tau, min_rows, int(max_rows), **fit)


def _solver_argument(solver):
    """What a build_*_row_sampling passes on to _fit_row_sampling for its ``solver``: nothing for "host", so that the default
    route calls it as it always has; ValueError for anything but "host" or "device"."""
    if solver not in ("host", "device"):
        raise ValueError("solver must be 'host' or 'device'")
    return {} if solver == "host" else {"solver": solver}


def _fit_row_sampling(G, pairs, projection, tau, min_rows, max_rows, solver="host"):
    """The RowSampling of a training matrix G (pairs r, N): row 0 forced in with weight 1, the rest by nnls_rows
    (``solver`` "host") or nnls_rows_device ("device")."""
    _solver_argument(solver)
    d = G.sum(axis=1)
    fit = nnls_rows if solver == "host" else nnls_rows_device
    x, _ = fit(G[:, 1:], d - G[:, 0], float(tau) * float(np.linalg.norm(d)) / max(float(np.linalg.norm(d - G[:, 0])), 1e-300),
                     max(min_rows - 1, 0), max_rows - 1)
    xi_full = np.concatenate([[1.0], x])
    rows = np.flatnonzero(xi_full > 0.0)
    residual = float(np.linalg.norm(G[:, rows] @ xi_full[rows] - d) / np.linalg.norm(d))
    return RowSampling(rows.astype(np.int32), xi_full[rows], projection, residual, pairs, tau)


def row_sampling_system(X, Phi, runs, dt, projection, E=0.0, supg=True, stride=10):
    """(G, pairs): the training matrix of build_row_sampling, (pairs r, N), column i the contributions of mesh row i; the
    full reduced right-hand sides are d = G 1.  ``X``, ``Phi``: host arrays; ``projection``: "galerkin" or "lspg"."""
    blocks = []
    for Sn, mu1, mu2 in _host_runs(runs, len(X)):
        P = Phi @ (Phi.T @ Sn)
        for n in range(0, Sn.shape[1] - 1, int(stride)):
            blocks.append(row_contributions(X, Phi, P[:, n + 1], P[:, n], mu1, mu2, float(dt), projection, float(E), supg))
    return _stack_contributions(blocks, "build_row_sampling")


def _host_runs(runs, N):
    """The runs (hist (N, nT+1), mu1, mu2) of a row-sampling builder as host float64 arrays and floats."""
    for hist, mu1, mu2 in runs:
        Sn = _host64(hist)
        if Sn.ndim != 2 or Sn.shape[0] != N or Sn.shape[1] < 2:
            raise ValueError("every run is (hist (N, nT+1), mu1, mu2)")
        yield Sn, float(mu1), float(mu2)


def _stack_contributions(blocks, who):
    G = np.concatenate(blocks, axis=0)
    if not np.isfinite(G).all():
        raise ValueError(f"{who}: the training data is not finite")
    return G, len(blocks)


def _manifold_row_sampling_system(who, X, P, S, lift, tangents, runs, dt, projection, E, supg, stride):
    """(G, pairs) for a PROM on the manifold u = P q + S lift(q): what ann_, rbf_ and quad_row_sampling_system share.  For
    every run and every ``stride``-th step n: Q = P^T hist, the pair Un, U0 lifted from q_n, q_{n+1}, and the contributions of
    all mesh rows with the tangent W = P + dW.  ``lift(q)``: (pairs, n) -> (pairs, k), the coordinates on S;
    ``tangents(q)``: (pairs, n) -> the (N, n) increments dW, one per pair.  Each model keeps its own arithmetic in the two."""
    blocks = []
    for Sn, mu1, mu2 in _host_runs(runs, len(X)):
        steps = np.arange(0, Sn.shape[1] - 1, int(stride))
        Q = P.T @ Sn                                                            # (n, nT+1)
        q_n, q_1 = Q[:, steps].T, Q[:, steps + 1].T
        Un = P @ q_n.T + S @ lift(q_n).T                                        # on the manifold
        U0 = P @ q_1.T + S @ lift(q_1).T
        for dW, u0, un in zip(tangents(q_1), U0.T, Un.T):
            blocks.append(row_contributions(X, P + dW, u0, un, mu1, mu2, float(dt), projection, float(E), supg))
    return _stack_contributions(blocks, who)


# ---- row sampling for the hyper-reduced POD-ANN PROM (rom.pod_ann_run_hyper, bg_hyper_ann_rom_run and _run_wide) ----
def ann_row_sampling_system(X, U_p, U_s, model, runs, dt, projection, E=0.0, supg=True, stride=10):
    """(G, pairs): the training matrix of build_ann_row_sampling, (pairs n, N).  ``X``, ``U_p``, ``U_s``: host arrays;
    ``model``: the closure, evaluated on the host in float32 (value and Jacobian, as the PROM evaluates them)."""
    import copy
    from . import rom as _rom
    ann = _rom.AnnEvaluator(copy.deepcopy(model).to(device="cpu", dtype=torch.float32).eval(), U_p.shape[1], torch.float32)
    return _manifold_row_sampling_system(
        "build_ann_row_sampling", X, U_p, U_s, lambda q: ann.forward(torch.as_tensor(q.copy())).numpy(),
        lambda q: (U_s @ J for J in ann.jacobian(torch.as_tensor(q.copy())).numpy()), runs, dt, projection, E, supg, stride)


def build_ann_row_sampling(X, U_p, U_s, model, runs, dt, projection, E=0.0, supg=True, tau=1e-4, stride=10, min_rows=None,
                           max_rows=None, solver="host"):
    """build_row_sampling for the POD-ANN PROM (rom.pod_ann_run_hyper: bg_hyper_ann_rom_run for n <= 8 primary modes, and
    rom.pod_ann_run_hyper_wide: bg_hyper_ann_rom_run_wide for n <= 20): the same host NNLS (nnls_rows, row 0 forced in with
    weight 1) on training pairs that lie on the closure manifold.  For every run (hist (N, nT+1), mu1, mu2) and every
    ``stride``-th step n: q_n = U_p^T s_n, Un = U_p q_n + U_s N(q_n), U0 likewise at n + 1, and the contributions
    c_i = w_i R_i of all mesh rows (picard_rows) with the tangent W = U_p + U_s dN(q_{n+1}): w_i = W[i] for "galerkin",
    (A W)[i] for "lspg".  ``model``: the closure (an nn.Module); value and Jacobian are taken in float32 on the host.

    ``min_rows`` defaults to 3 n as the POD builder's does.  With that default on the committed closure (n = 5, nbar = 91,
    N = 512, nine training runs, tau = 1e-4) the fit itself asks for far more rows -- 181 (Galerkin) and 136 (LSPG) -- and
    the sampled iteration stayed within 6.4e-4 / 2.6e-3 (rel-L2, 40 steps) of the full PROM at mu = (4.6, 0.021) and
    (5.3, 0.017), with no divergence, no capped step that the full PROM does not have (the first LSPG step caps in both)
    and iteration totals within 1 of the full PROM's; the default was therefore left at 3 n.  A closure whose fit is met by few rows may need more: at N = 2049 a random closure ran with
    ``min_rows`` = 120.  ``max_rows`` defaults to the limit of the loop that takes n (hyper_ann_rom_limits, or
    hyper_ann_wide_rom_limits beyond its n); needing more is a ValueError.
    Returns a RowSampling; save_row_sampling / load_row_sampling store it.
    ``solver``: "host" or "device", as in build_row_sampling."""
    projection, X = _sampling_prelude("build_ann_row_sampling", X, projection, runs, tau, stride)
    fit = _solver_argument(solver)
    U_p, U_s = _host_matrix(U_p), _host_matrix(U_s)
    N = len(X)
    if U_p.ndim != 2 or U_s.ndim != 2 or U_p.shape[0] != N or U_s.shape[0] != N:
        raise ValueError("U_p and U_s must have one row per mesh node")
    min_rows = min(3 * U_p.shape[1], N) if min_rows is None else int(min_rows)
    if max_rows is None:         # the limit of the loop that takes this n
        max_rows = (hyper_ann_rom_limits() if U_p.shape[1] <= hyper_ann_rom_limits()[0] else hyper_ann_wide_rom_limits())[4]
    max_rows = int(max_rows)
    G, pairs = ann_row_sampling_system(X, U_p, U_s, model, runs, dt, projection, E, supg, stride)
    return _fit_row_sampling(G, pairs, projection, tau, min_rows, max_rows, **fit)


# ---- row sampling for the hyper-reduced quadratic-manifold PROM (rom.quadratic_run_hyper, bg_hyper_quad_rom_run) ----
def quad_row_sampling_system(X, Phi, H, runs, dt, projection, E=0.0, stride=10):
    """(G, pairs): the training matrix of build_quad_row_sampling, (pairs n, N).  ``X``, ``Phi`` (N, n), ``H`` (N, n(n+1)/2):
    host arrays; ``projection``: "galerkin" or "lspg".  This stepper has no SUPG term (picard_rows with supg=False)."""
    n = Phi.shape[1]
    I, J = np.triu_indices(n)
    idx = np.zeros((n, n), dtype=np.int64)
    idx[I, J] = idx[J, I] = np.arange(len(I))
    H3 = H[:, idx] * (np.ones((n, n)) + np.eye(n))                              # (N, n, n): tangent = Phi + H3 . q
    return _manifold_row_sampling_system(
        "build_quad_row_sampling", X, Phi, H, lambda q: (q.T[I] * q.T[J]).T, lambda q: (H3 @ qk for qk in q), runs, dt, projection,
        E, False, stride)


def build_quad_row_sampling(X, Phi, H, runs, dt, projection, E=0.0, tau=1e-5, stride=10, min_rows=None, max_rows=None,
                            solver="host"):
    """build_row_sampling for the quadratic-manifold PROM (rom.quadratic_run_hyper): the same host NNLS (nnls_rows, row 0
    forced in with weight 1) on training pairs that lie on the manifold.  For every run (hist (N, nT+1), mu1, mu2) and every
    ``stride``-th step n: q_n = Phi^T s_n, Un = Phi q_n + H sym(q_n), U0 likewise at n + 1, and the contributions
    c_i = w_i R_i of all mesh rows (picard_rows without the SUPG term, which this stepper does not have) with the tangent
    W = Phi + H dQ/dq(q_{n+1}): w_i = W[i] for "galerkin", (A W)[i] for "lspg".

    ``tau`` defaults to 1e-5, not the 1e-4 of the other builders: at 1e-4 the LSPG iteration is unusable.  Measured with the
    numpy restatement of the sampled iteration against the full PROM (N = 2049, dt = 0.0125, n = 40, alpha = 1e-2, nine
    training runs, every 10th step, rel-L2 over 4 steps at mu = (4.6, 0.021) and (5.3, 0.017)): Galerkin tau = 1e-4: 172 rows,
    1.6e-3 .. 1.8e-3; LSPG 1e-4: 156 rows, 7.4e-2 .. 9.9e-2 with three iterations more than the full PROM; LSPG 1e-5: 171
    rows, 1.9e-3 .. 2.1e-3; LSPG 1e-6: 174 rows, 1.6e-3 .. 1.8e-3; at tau <= 1e-5 every iteration count equals the full PROM's.
    ``min_rows`` defaults to 3 n as the POD builder's does.  The training matrix has a small numerical rank (184 .. 190 of
    2049 columns there, 107 .. 110 of 1024 at N = 1024 with the same dt), and a sampling with more rows than that rank fits
    it exactly and then IS the full PROM to rounding: with ``min_rows`` = 250 the loop stayed within 2e-9 of the full PROM
    over 40 steps at N = 1024 (dt = 0.025) and N = 4096 (dt = 0.00625), every count equal, where the default's 161 .. 179
    rows drifted to 2e-3 .. 2e-2 and, LSPG at N = 4096, ended in steps that hit the cap.  For long runs ask for
    ``min_rows`` above the rank.  ``max_rows`` defaults to the kernel's limit (hyper_quad_rom_limits); needing more is a
    ValueError.  Returns a RowSampling; save_row_sampling / load_row_sampling store it.
    ``solver``: "host" or "device", as in build_row_sampling."""
    projection, X = _sampling_prelude("build_quad_row_sampling", X, projection, runs, tau, stride)
    fit = _solver_argument(solver)
    Phi, H = _host_matrix(Phi), _host_matrix(H)
    N = len(X)
    if Phi.ndim != 2 or H.ndim != 2 or Phi.shape[0] != N or H.shape != (N, Phi.shape[1] * (Phi.shape[1] + 1) // 2):
        raise ValueError("Phi must be (N, n) and H (N, n(n+1)/2), one row per mesh node")
    min_rows = min(3 * Phi.shape[1], N) if min_rows is None else int(min_rows)
    max_rows = hyper_quad_rom_limits()[1] if max_rows is None else int(max_rows)
    G, pairs = quad_row_sampling_system(X, Phi, H, runs, dt, projection, E, stride)
    return _fit_row_sampling(G, pairs, projection, tau, min_rows, max_rows, **fit)


# ---- row sampling for the hyper-reduced local POD PROM (rom.local_prom_run_hyper, bg_hyper_local_rom_run) ----
def _host_local_bases(centres, local_bases, U_global, num_global_modes, N, who):
    """(centres (C, mg), [Phi_0 .. Phi_{C-1}], U_g (N, mg)) as host float64 arrays; ValueError for shapes that cannot be right
    or a centre without a basis."""
    centres, mg = _host_matrix(centres), int(num_global_modes)
    Ug = _host_matrix(U_global)
    if centres.ndim != 2 or centres.shape[1] != mg or Ug.ndim != 2 or Ug.shape[0] != N or Ug.shape[1] < mg:
        raise ValueError(f"{who}: centres must be (C, m) and U_global (N, >= m) with m = num_global_modes")
    missing = [c for c in range(len(centres)) if c not in local_bases]
    if missing:
        raise ValueError(f"{who}: centre {missing[0]} has no local basis")
    bases = [_host_matrix(local_bases[c]) for c in range(len(centres))]
    if any(b.ndim != 2 or b.shape[0] != N or b.shape[1] < 1 for b in bases):
        raise ValueError(f"{who}: every local basis must be (N, >= 1), one row per mesh node")
    return centres, bases, np.ascontiguousarray(Ug[:, :mg])


def local_row_sampling_system(X, centres, local_bases, U_global, num_global_modes, runs, dt, projection, E=0.0, supg=True,
                              stride=10):
    """(G, pairs): the training matrix of build_local_row_sampling, column i the contributions of mesh row i.  For every run
    and every ``stride``-th step n the cluster c is the nearest centre to U_g^T s_n (the first index of the smallest squared
    distance, as local_prom_burgers picks it), the pair is Un = Phi_c Phi_c^T s_n, U0 = Phi_c Phi_c^T s_{n+1}, and the block
    row_contributions(X, Phi_c, U0, Un, ...) has r_c rows; the full reduced right-hand sides are d = G 1.  ``X``: a host
    array; ``projection``: "galerkin" or "lspg"."""
    centres, bases, Ug = _host_local_bases(centres, local_bases, U_global, num_global_modes, len(X), "local_row_sampling_system")
    blocks = []
    for Sn, mu1, mu2 in _host_runs(runs, len(X)):
        for n in range(0, Sn.shape[1] - 1, int(stride)):
            qg = Ug.T @ Sn[:, n]
            Phi = bases[int(np.argmin(((centres - qg[None, :]) ** 2).sum(1)))]
            P = Phi @ (Phi.T @ Sn[:, n:n + 2])
            blocks.append(row_contributions(X, Phi, P[:, 1], P[:, 0], mu1, mu2, float(dt), projection, float(E), supg))
    return _stack_contributions(blocks, "build_local_row_sampling")


def build_local_row_sampling(X, centres, local_bases, U_global, num_global_modes, runs, dt, projection, E=0.0, supg=True,
                             tau=1e-4, stride=10, min_rows=None, max_rows=None, solver="host"):
    """build_row_sampling for the local POD PROM (rom.local_prom_run_hyper): ONE sampling for all clusters, fitted by the same
    host NNLS (nnls_rows, row 0 forced in with weight 1) on training pairs that each lie in the span of the cluster the
    reference would hold there (local_row_sampling_system).  ``centres`` (C, m), ``local_bases`` {c: (N, r_c)}, ``U_global``
    and ``num_global_modes`` are local_prom_burgers's arguments; ``runs`` as in build_row_sampling.
    ``min_rows`` defaults to min(3 max_c r_c, N), ``max_rows`` to the kernel's limit (hyper_local_rom_limits); needing more
    is a ValueError.  Returns a RowSampling; save_row_sampling / load_row_sampling store it.
    ``solver``: "host" or "device", as in build_row_sampling."""
    projection, X = _sampling_prelude("build_local_row_sampling", X, projection, runs, tau, stride)
    fit = _solver_argument(solver)
    N = len(X)
    _, bases, _ = _host_local_bases(centres, local_bases, U_global, num_global_modes, N, "build_local_row_sampling")
    min_rows = min(3 * max(b.shape[1] for b in bases), N) if min_rows is None else int(min_rows)
    max_rows = hyper_local_rom_limits()[1] if max_rows is None else int(max_rows)
    G, pairs = local_row_sampling_system(X, centres, local_bases, U_global, num_global_modes, runs, dt, projection, E, supg, stride)
    return _fit_row_sampling(G, pairs, projection, tau, min_rows, max_rows, **fit)


# ---- row sampling for the hyper-reduced POD-RBF PROM (rom.pod_rbf_run_hyper, bg_hyper_rbf_rom_run) ----
def _rbf_host_closure(X_train, W, epsilon, x_min, x_max, y_min, y_max, kernel):
    """(value, jacobian) of the scaled RBF closure on the host in fp64 numpy, for a batch q (P, n): value (P, nbar) and
    jacobian (P, nbar, n).  The closure of rom.RbfClosure (scaling with the dx / dy floors of _rbf_range); training
    arithmetic for build_rbf_row_sampling, not a stepper."""
    kind = _rbf_kind(kernel)
    Xt, Wm = _host_matrix(X_train), _host_matrix(W)
    vec = lambda v: _host64(v).reshape(-1)
    x_min, y_min = vec(x_min), vec(y_min)
    dx, dy = _rbf_range(x_min, vec(x_max)), _rbf_range(y_min, vec(y_max))
    if Xt.ndim != 2 or Wm.ndim != 2 or Wm.shape != (Xt.shape[0], len(dy)) or Xt.shape[1] != len(dx):
        raise ValueError("X_train must be (Ns, n) and W (Ns, nbar)")
    eps2 = float(epsilon) ** 2

    def kernel_terms(q):
        diff = (2.0 * ((np.atleast_2d(q) - x_min) / dx) - 1.0)[:, None, :] - Xt[None]          # (P, Ns, n)
        r2 = (diff * diff).sum(axis=2)
        if kind == 0:
            p = np.exp(-eps2 * r2)
            return diff, p, -2.0 * eps2 * p
        p = 1.0 / np.sqrt(1.0 + eps2 * r2)
        return diff, p, -eps2 * p ** 3

    # The operation order of the reference (FEM/fem_burgers.py:225-260).  The weights reach 3.6e2 with results of O(1): a
    # float64 contraction over the centres carries 5e-14 of rounding (two differently ordered ones differ by 1e-13), so the
    # two contractions accumulate in long double (offline arithmetic: a few million products per run).
    Wl = Wm.astype(np.longdouble)

    def value(q):
        return 0.5 * ((kernel_terms(q)[1].astype(np.longdouble) @ Wl).astype(np.float64) + 1.0) * dy + y_min

    def jacobian(q):
        diff, _, coef = kernel_terms(q)
        G = (coef[:, :, None] * diff).astype(np.longdouble)                                    # (P, Ns, n)
        return (0.5 * dy)[None, :, None] * (np.einsum("ij,pik->pjk", Wl, G).astype(np.float64) * (2.0 / dx))

    return value, jacobian


def rbf_row_sampling_system(X, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max, kernel, runs, dt, projection,
                            E=0.0, supg=True, stride=10):
    """(G, pairs): the training matrix of build_rbf_row_sampling, (pairs n, N).  ``X``, ``U_p``, ``U_s``: host arrays; the
    closure is evaluated on the host in fp64 (value and Jacobian, _rbf_host_closure)."""
    value, jacobian = _rbf_host_closure(X_train, W, epsilon, x_min, x_max, y_min, y_max, kernel)
    if U_p.shape[1] != np.shape(X_train)[1] or U_s.shape[1] != np.shape(W)[1]:
        raise ValueError("X_train must be (Ns, n) and W (Ns, nbar) for the n, nbar of U_p, U_s")
    return _manifold_row_sampling_system(
        "build_rbf_row_sampling", X, U_p, U_s, value, lambda q: (U_s @ J for J in jacobian(q)), runs, dt, projection, E, supg,
        stride)


def build_rbf_row_sampling(X, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max, runs, dt, projection,
                           kernel="gaussian", E=0.0, supg=True, tau=1e-4, stride=10, min_rows=None, max_rows=None, solver="host"):
    """build_row_sampling for the POD-RBF PROM (rom.pod_rbf_run_hyper): the same host NNLS (nnls_rows, row 0 forced in with
    weight 1) on training pairs that lie on the closure manifold.  For every run (hist (N, nT+1), mu1, mu2) and every
    ``stride``-th step n: q_n = U_p^T s_n, Un = U_p q_n + U_s f(q_n), U0 likewise at n + 1, and the contributions
    c_i = w_i R_i of all mesh rows (picard_rows) with the tangent W = U_p + U_s J(q_{n+1}): w_i = W[i] for "galerkin",
    (A W)[i] for "lspg".  The closure (X_train, W, epsilon, the four scaling vectors, ``kernel``) is evaluated on the host
    in fp64 numpy.

    ``min_rows`` defaults to min(200, N, max_rows), not to 3 n as the POD and POD-ANN builders': in a numpy restatement of
    the weighted-row iteration (6 - 8 steps) the 3 n = 51 rows the fit is content with at tau = 1e-4 did not hold the
    iteration.  Committed closure (n = 17, nbar = 79, N = 512), rows / table nodes / training residual / rel-L2 against
    the full PROM with ``min_rows`` = 51 and with 200:  gaussian Galerkin 169 / 336 / 9e-5 / 1.3e-4 and 200 / 393 / 7e-6 /
    7e-6;  gaussian LSPG 141 / 295 / 9e-5 / 1.3e-3 and 200 / 366 / 5e-6 / 1e-4;  imq LSPG 142 / 277 / 1e-4 / 4.9e-2 and
    200 / 373 / 6e-6 / 5.5e-4.  A closure fitted to a 2049-node mesh (imq): LSPG with 51 took 73 ... 127 rows at a
    residual of 1e-4 and left the full PROM by O(1) with capped steps, Galerkin 163 rows and 1e-3 ... 1e-2; with 200 rows
    (241 nodes, residual 1e-13) LSPG stays within 2e-11.  ``max_rows`` defaults to the kernel's limit
    (hyper_rbf_rom_limits); needing more is a ValueError.
    Returns a RowSampling; save_row_sampling / load_row_sampling store it.
    ``solver``: "host" or "device", as in build_row_sampling."""
    projection, X = _sampling_prelude("build_rbf_row_sampling", X, projection, runs, tau, stride)
    fit = _solver_argument(solver)
    U_p, U_s = _host_matrix(U_p), _host_matrix(U_s)
    N = len(X)
    if U_p.ndim != 2 or U_s.ndim != 2 or U_p.shape[0] != N or U_s.shape[0] != N:
        raise ValueError("U_p and U_s must have one row per mesh node")
    max_rows = hyper_rbf_rom_limits()[3] if max_rows is None else int(max_rows)
    min_rows = min(200, N, max_rows) if min_rows is None else int(min_rows)
    G, pairs = rbf_row_sampling_system(X, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max, kernel, runs, dt,
                                       projection, E, supg, stride)
    return _fit_row_sampling(G, pairs, projection, tau, min_rows, max_rows, **fit)


def save_row_sampling(directory, sampling):
    """A RowSampling as rows.npy, xi.npy and row_sampling.npz (projection, residual, pairs, tau); no pickles.  Returns the directory."""
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "rows.npy"), _host(sampling.rows))
    np.save(os.path.join(directory, "xi.npy"), _host(sampling.xi))
    np.savez(os.path.join(directory, "row_sampling.npz"), projection=np.array(sampling.projection, dtype=np.str_),
             residual=np.float64(sampling.residual), pairs=np.int64(sampling.pairs), tau=np.float64(sampling.tau))
    return directory


def load_row_sampling(directory):
    """The RowSampling save_row_sampling wrote."""
    with _npy(directory, "row_sampling.npz") as z:
        meta = {k: z[k] for k in z.files}
    return RowSampling(_npy(directory, "rows.npy"), _npy(directory, "xi.npy"), str(meta["projection"]), float(meta["residual"]),
                       int(meta["pairs"]), float(meta["tau"]))


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
    for name in ("centres", "U_global", "labels", "member_bits"):
        np.save(os.path.join(directory, name + ".npy"), _host(getattr(result, name)))
    np.savez(os.path.join(directory, "local_bases.npz"), **{str(c): _host(b) for c, b in result.local_bases.items()})
    np.savez(os.path.join(directory, "singular_values.npz"), **{str(c): _host(v) for c, v in result.singular_values.items()})
    km = result.kmeans
    np.savez(os.path.join(directory, "clustering.npz"), num_global_modes=np.int64(result.num_global_modes),
             member_counts=np.asarray(result.member_counts, dtype=np.int64), overlap=np.float64(result.overlap),
             n_iter=np.int64(km.n_iter), converged=np.bool_(km.converged), inertia=np.float64(km.inertia),
             changed=np.asarray(km.changed, dtype=np.int64))
    return directory


_RBF_ARRAYS = ("U_p", "U_s", "X_train", "W", "x_min", "x_max", "y_min", "y_max", "centre_index")


def save_rbf_closure(directory, fit):
    """An RbfFit as .npy / .npz files (no pickles): one .npy per tensor (U_p, U_s, X_train, W, x_min, x_max, y_min, y_max,
    centre_index) and closure.npz with the scalars (epsilon, ridge, backward_error, kernel as a string array).  Returns the
    directory."""
    os.makedirs(directory, exist_ok=True)
    for name in _RBF_ARRAYS:
        np.save(os.path.join(directory, name + ".npy"), _host(getattr(fit, name)))
    np.savez(os.path.join(directory, "closure.npz"), epsilon=np.float64(fit.epsilon), ridge=np.float64(fit.ridge),
             backward_error=np.float64(fit.backward_error), kernel=np.array(fit.kernel, dtype=np.str_))
    return directory


def load_rbf_closure(directory, device="cpu"):
    """The RbfFit save_rbf_closure wrote, as tensors on ``device``."""
    t = {name: torch.as_tensor(_npy(directory, name + ".npy")).to(device).contiguous() for name in _RBF_ARRAYS}
    with _npy(directory, "closure.npz") as z:
        meta = {k: z[k] for k in z.files}
    return RbfFit(t["U_p"], t["U_s"], t["X_train"], t["W"], float(meta["epsilon"]), str(meta["kernel"]), t["x_min"], t["x_max"],
                  t["y_min"], t["y_max"], float(meta["ridge"]), t["centre_index"], float(meta["backward_error"]))


def load_local_bases(directory, device="cpu"):
    """The LocalBases save_local_bases wrote, as tensors on ``device``."""
    dev = lambda a: torch.as_tensor(a).to(device)
    with _npy(directory, "local_bases.npz") as z:
        bases = {int(k): dev(z[k]).contiguous() for k in z.files}
    with _npy(directory, "singular_values.npz") as z:
        svals = {int(k): dev(z[k]) for k in z.files}
    with _npy(directory, "clustering.npz") as z:
        meta = {k: z[k] for k in z.files}
    centres, labels = dev(_npy(directory, "centres.npy")), dev(_npy(directory, "labels.npy"))
    km = KMeansResult(centres, labels, int(meta["n_iter"]), bool(meta["converged"]), float(meta["inertia"]), meta["changed"].tolist())
    return LocalBases(centres, dict(sorted(bases.items())), dev(_npy(directory, "U_global.npy")), int(meta["num_global_modes"]), labels,
                      dev(_npy(directory, "member_bits.npy")), meta["member_counts"].tolist(), dict(sorted(svals.items())),
                      float(meta["overlap"]), km)
