"""The NumPy references of the local POD builder tests (test_local_builder_abi.py, test_local_builder_gpu.py): a plain Lloyd
iteration with the direct-sum distance, the overlap rule of tests/golden/make_golden.py fx_local_pod, the builder on
np.linalg.svd, and the margins that say whether a reference label or membership is decided beyond rounding.  Nothing here
imports the code under test."""
import numpy as np


def d2_matrix(Q, centres):
    return ((Q[:, None, :] - centres[None]) ** 2).sum(2)


def margins(Q, centres, overlap=None, ignore=()):
    """(label margin, overlap margin): the smallest relative gap between the two smallest squared distances of a point,
    and the smallest relative distance of any d2[i, c] from overlap * d2min[i] (the label's own column aside).  ``ignore``:
    centre indices left out of the label margin (deliberate duplicates)."""
    d2 = d2_matrix(Q, centres)
    keep = [c for c in range(len(centres)) if c not in ignore]
    lab_margin = np.inf
    if len(keep) > 1:
        two = np.sort(d2[:, keep], 1)[:, :2]
        lab_margin = float(((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)).min())
    ov_margin = np.inf
    if overlap is not None:
        thr = overlap * d2.min(1)[:, None]
        rel = np.abs(d2 - thr) / np.maximum(thr, 1e-300)
        rel[np.arange(len(Q)), d2.argmin(1)] = np.inf
        ov_margin = float(rel.min())
    return lab_margin, ov_margin


def members(Q, centres, overlap):
    """(labels, (Ns, C) boolean membership): c == label or d2[:, c] < overlap * d2min (fx_local_pod)."""
    d2 = d2_matrix(Q, centres)
    lab = d2.argmin(1)
    return lab, (lab[:, None] == np.arange(len(centres))[None]) | (d2 < overlap * d2.min(1)[:, None])


def member_words(mask):
    return (mask.astype(np.uint64) << np.arange(mask.shape[1], dtype=np.uint64)[None]).sum(1, dtype=np.uint64)


def means(Q, labels, centres):
    """Centres moved to the float64 means of their points; a cluster without points keeps its centre.  Also the counts."""
    C = len(centres)
    new = np.stack([Q[labels == c].mean(0) if np.any(labels == c) else centres[c] for c in range(C)])
    return new, np.bincount(labels, minlength=C)


def lloyd(Q, init, max_iter=100):
    """Plain Lloyd from ``init``: dict with the final centres and labels, the pass count, converged, the labels of every pass,
    the number of labels every pass changed, the inertia of the final labels, and the smallest label margin met on the way."""
    centres = np.array(init, dtype=np.float64)
    labels = np.full(len(Q), -1)
    seq, changed, worst, converged, n_iter = [], [], np.inf, False, 0
    for n_iter in range(1, max_iter + 1):
        new = d2_matrix(Q, centres).argmin(1)
        worst = min(worst, margins(Q, centres)[0])
        changed.append(int((new != labels).sum()))
        labels = new
        seq.append(labels.copy())
        if changed[-1] == 0:
            converged = True
            break
        centres = means(Q, labels, centres)[0]
    if not converged:
        labels = d2_matrix(Q, centres).argmin(1)
        worst = min(worst, margins(Q, centres)[0])
    inertia = float(d2_matrix(Q, centres)[np.arange(len(Q)), labels].sum())
    return dict(centres=centres, labels=labels, n_iter=n_iter, converged=converged, seq=seq, changed=changed, inertia=inertia,
                margin=worst)


def builder(S, n_clusters, m, init_rows, overlap, epsilon_squared, max_modes):
    """The fx_local_pod recipe on np.linalg.svd: global basis, coordinates, Lloyd from the rows ``init_rows`` of Q, overlap
    sets, one truncated basis per cluster (energy rule of POD/pod.py:8-14, capped).  Returns a dict."""
    Ug, sg, _ = np.linalg.svd(S, full_matrices=False)
    Q = np.ascontiguousarray((Ug[:, :m].T @ S).T)
    km = lloyd(Q, Q[init_rows])
    lab, mask = members(Q, km["centres"], overlap)
    bases, svals = {}, {}
    for c in range(n_clusters):
        Uc, sc, _ = np.linalg.svd(S[:, mask[:, c]], full_matrices=False)
        loss = 1.0 - np.cumsum(sc ** 2) / np.sum(sc ** 2)
        K = min(int(np.argmax(loss <= epsilon_squared)) + 1, max_modes)
        bases[c], svals[c] = np.ascontiguousarray(Uc[:, :K]), sc
    return dict(U_global=Ug, Q=Q, kmeans=km, centres=km["centres"], labels=lab, mask=mask, bases=bases, svals=svals,
                margins=(km["margin"],) + margins(Q, km["centres"], overlap))


def blobs(seed=0, Ns=600, m=12, C=4, spread=0.3):
    """Well-separated clusters: C centres drawn at scale 4, Ns points around them, shuffled."""
    rng = np.random.default_rng(seed)
    mid = rng.normal(0.0, 4.0, (C, m))
    Q = mid[np.arange(Ns) % C] + rng.normal(0.0, spread, (Ns, m))
    return np.ascontiguousarray(Q[rng.permutation(Ns)])


def smooth_trajectory(Ns=600, m=12):
    """Points along one smooth curve, the shape POD coordinates of a time history take: decaying harmonics of t."""
    t = np.linspace(0.0, 1.0, Ns)
    j = np.arange(m)
    return np.ascontiguousarray(np.cos(np.outer(t, 1.0 + 0.7 * j) * np.pi + 0.3 * j) / (1.0 + j))


def synthetic_snapshots(N=40, samples=3, steps=100):
    """(N, samples * steps) travelling, widening bumps: a snapshot matrix whose clusters follow time, without a solver."""
    x = np.linspace(0.0, 1.0, N)[:, None]
    cols = []
    for a in np.linspace(0.8, 1.2, samples):
        t = np.linspace(0.0, 1.0, steps)[None, :]
        cols.append(1.0 + a * np.exp(-((x - 0.15 - 0.6 * a * t) / (0.08 + 0.05 * t)) ** 2))
    return np.ascontiguousarray(np.hstack(cols))
