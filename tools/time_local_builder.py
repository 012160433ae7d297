#!/usr/bin/env python3
"""Time of the local POD builder (pod.build_local_bases) on a FOM sweep built on the device, and of the two things it
replaces: a torch-only Lloyd iteration (cdist + argmin + index_add_) from the same start, and the per-cluster SVDs one
thin_svd at a time (batched=False).  Prints one JSON line: milliseconds of each (median of --reps), the Lloyd passes, the
Jacobi sweeps per cluster, the members and widths per cluster, and whether the two SVD routes gave the same bits.
usage: python tools/time_local_builder.py [--n 512] [--batch 64] [--steps 500] [--clusters 11] [--m 12] [--dt 0.05] [--reps 3]"""
import argparse, json
from _timing import draw, time_runs
import numpy as np, torch
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512); ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=500); ap.add_argument("--clusters", type=int, default=11)
ap.add_argument("--m", type=int, default=12); ap.add_argument("--dt", type=float, default=0.05)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--max-modes", type=int, default=40)
a = ap.parse_args()
from burgers_hip import fom, pod
N, C, m = a.n, a.clusters, a.m
X = np.linspace(0, 100, N)
mu1, mu2 = draw(a.batch)
S = pod.snapshot_matrix(fom.fom_run(X, np.ones(N), mu1, mu2, a.dt, a.steps).hist).contiguous()       # (N, B (nT + 1))
Ug = pod.thin_svd(S)[0]
Q = (Ug[:, :m].t() @ S).t().contiguous()
rows = torch.as_tensor(np.random.default_rng(0).choice(Q.shape[0], C, replace=False), device=Q.device)


def torch_lloyd(max_iter=100):
    """The Lloyd iteration in library calls only: the same start, stopping rule and keep-if-empty rule as pod.kmeans."""
    cen, lab = Q[rows].clone(), torch.full((Q.shape[0],), -1, device=Q.device)
    for it in range(1, max_iter + 1):
        new = torch.cdist(Q, cen, compute_mode="donot_use_mm_for_euclid_dist").argmin(1)
        changed = int((new != lab).sum())
        lab = new
        if changed == 0:
            break
        sums = torch.zeros_like(cen).index_add_(0, lab, Q)
        cnt = torch.bincount(lab, minlength=C)
        cen = torch.where(cnt[:, None] > 0, sums / cnt[:, None].clamp(min=1), cen)
    return lab, it


info = {True: {}, False: {}}
build = lambda batched: pod.build_local_bases(S, C, m, U_global=Ug, epsilon_squared=1e-6, max_modes=a.max_modes, init=Q[rows],
                                              batched=batched, info=info[batched])
ms_km, km = time_runs(lambda: pod.kmeans(Q, C, init=Q[rows]), a.reps)
ms_tl, (tl_lab, tl_it) = time_runs(torch_lloyd, a.reps)
ms_b, built = time_runs(lambda: build(True), a.reps)
ms_s, plain = time_runs(lambda: build(False), a.reps)
med = lambda v: float(f"{np.median(v):.4g}")
print(json.dumps({
    "N": N, "snapshots": int(S.shape[1]), "clusters": C, "m": m,
    "kmeans_ms": med(ms_km), "torch_lloyd_ms": med(ms_tl), "kmeans_passes": km.n_iter, "torch_lloyd_passes": tl_it,
    "converged": km.converged, "same_labels_as_torch_lloyd": bool(torch.equal(km.labels.long(), tl_lab)),
    "builder_batched_ms": med(ms_b), "builder_sequential_ms": med(ms_s),
    "svd_stage_batched_ms": med(np.asarray(ms_b) - np.median(ms_km)), "svd_stage_sequential_ms": med(np.asarray(ms_s) - np.median(ms_km)),
    "clusters_in_the_batch": info[True]["batched"], "sweeps_batched": info[True]["sweeps"], "sweeps_sequential": info[False]["sweeps"],
    "members": built.member_counts, "widths": [int(built.local_bases[c].shape[1]) for c in range(C)],
    "same_bits": all(torch.equal(built.local_bases[c], plain.local_bases[c]) for c in range(C)),
}), flush=True)
