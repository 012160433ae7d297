"""What the tests (and the timer) of the device-side POD-ANN loop for up to 20 primary modes (bg_ann_rom_run_wide) share:
the random closures, the bases, the cases the loop is tested at, and one cached oracle run per case and sample.  numpy only
at import; torch and the oracle are imported where they are used.

Closures: ``mlp(widths, act, bias, seed, scale)`` (torch.manual_seed(seed), every Linear.weight x 0.5, then the last
layer's weight and bias multiplied by ``scale``) also serves tests/test_ann_fused_gpu.py.  At scale 0.02 a wrong tangent
row moves the history by less than the float32 gate (a swap of columns 0 and 16 of the Jacobian: 8.3e-7 LSPG, 3.1e-7
Galerkin), so those closures only exercise shapes; the tangent-sensitive cases use scale 3.0 (1.4e-4 / 5.2e-5)."""
import functools
import os

import numpy as np

import loop_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL32 = 5e-6          # the float32 gate of the POD-ANN tests, tests/test_ann_fused_gpu.py
WIDE = "bg_ann_rom_run_wide"

# name: N, n, nbar, hidden widths, activation, bias, seed, scale, E
CASE_A = ("A", 512, 17, 79, (32, 64, 128, 256, 256), "ELU", True, 529, 3.0, 0.0)      # the reference's second model size
# the shapes, activations and limits of the GPU test (B = 19, 5 steps, E = 0.001)
SHAPE_CASES = [
    ("B-tanh", 512, 20, 76, (256, 33), "Tanh", True, 532, 3.0, 0.001),
    ("8-layers", 512, 20, 128, (256,) * 7, "ELU", True, 540, 0.02, 0.001),
    ("C-relu", 512, 9, 87, (7,), "ReLU", False, 521, 0.02, 0.001),
    ("ragged-301", 301, 13, 40, (130, 50), "Tanh", False, 314, 0.02, 0.001),
    ("full-256", 256, 12, 60, (64,), "ELU", True, 268, 0.02, 0.001),
    ("odd-255", 255, 17, 30, (16,) * 7, "ELU", True, 272, 0.02, 0.001),
    ("small-100", 100, 12, 30, (64,), "ELU", True, 112, 0.02, 0.001),
]
# the issue's cases B and C (ELU, so the oracle runs them) and the n = 8 model both entry points take
CASE_B = ("B", 512, 20, 76, (256, 33), "ELU", True, 532, 0.02, 0.001)
CASE_C = ("C", 512, 9, 87, (7,), "ELU", True, 521, 0.02, 0.001)
CASE_N8 = ("n8", 512, 8, 88, (7,), "ELU", True, 520, 0.02, 0.001)
ALL_CASES = [CASE_A, CASE_B, CASE_C, CASE_N8] + SHAPE_CASES


def mlp(widths, act, bias, seed, scale=1.0):
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    layers = []
    for i in range(len(widths) - 1):
        lin = nn.Linear(widths[i], widths[i + 1], bias=bias)
        with torch.no_grad():
            lin.weight.mul_(0.5)
        layers.append(lin)
        if i < len(widths) - 2:
            layers.append(getattr(nn, act)())
    with torch.no_grad():
        layers[-1].weight.mul_(scale)
        if bias:
            layers[-1].bias.mul_(scale)
    return nn.Sequential(*layers).eval()


def case_model(case, scale=None):
    _, _, n, nbar, hidden, act, bias, seed, sc, _ = case
    return mlp([n, *hidden, nbar], act, bias, seed, sc if scale is None else scale)


def weights(model):
    """(Ws, bs) as the oracle's pod_ann_prom takes them (zero bias where the layer has none)."""
    import torch.nn as nn
    lins = [m for m in model if isinstance(m, nn.Linear)]
    return ([m.weight.detach().cpu().numpy() for m in lins],
            [np.zeros(m.out_features, np.float32) if m.bias is None else m.bias.detach().cpu().numpy() for m in lins])


@functools.lru_cache(maxsize=None)
def bases(N, n, nbar):
    """(X, U_p, U_s).  N = 512 with n + nbar <= 96: the 96 committed modes of rbf_n17.npz re-split at n; otherwise the
    leading singular vectors of loop_cases.training_snapshots(N, 0.05)."""
    if N == 512 and n + nbar <= 96:
        g = np.load(os.path.join(GOLDEN, "rbf_n17.npz"))
        U = np.concatenate([g["U_p"], g["U_s"]], 1)
        X = np.linspace(0.0, 100.0, 512)
    else:
        X, _, U = loop_cases.training_snapshots(N, 0.05)
    Up, Us = np.ascontiguousarray(U[:, :n]), np.ascontiguousarray(U[:, n:n + nbar])
    for a in (Up, Us):
        a.setflags(write=False)
    return X, Up, Us


def case_bases(case):
    return bases(case[1], case[2], case[3])


def nonuniform_mesh():
    """The perturbed mesh of test_ann_fused_nonuniform_mesh."""
    X = np.linspace(0.0, 100.0, 512)
    X[1:-1] += np.random.default_rng(5).uniform(-0.03, 0.03, 510)
    return X


_oracle_cache = {}


def oracle(case, mu1, mu2, nT, proj, scale=None, X=None, swap=None):
    """(U, iters) of one sample by oracle.burgers_ref.pod_ann_prom (ELU closures only), cached per process; leave it as it
    is.  ``swap``: a pair of columns of the closure Jacobian to exchange (what a wrong tangent row would do)."""
    from oracle import burgers_ref as br
    assert case[5] == "ELU", "the oracle restates the reference's ELU network only"
    key = (case, float(mu1), float(mu2), nT, proj, scale, None if X is None else X.tobytes(), swap)
    if key not in _oracle_cache:
        Xc, Up, Us = case_bases(case)
        Xc = Xc if X is None else X
        Ws, bs = weights(case_model(case, scale))
        real = br.mlp_jacobian

        def swapped(w, b, q):
            J = real(w, b, q).copy()
            J[:, list(swap)] = J[:, list(swap)[::-1]]
            return J
        if swap is not None:
            br.mlp_jacobian = swapped
        try:
            _oracle_cache[key] = br.pod_ann_prom(Xc, 0.05, nT, np.ones(len(Xc)), mu1, case[9], mu2, Up, Us, Ws, bs,
                                                 projection=proj, return_iters=True)
        finally:
            br.mlp_jacobian = real
    return _oracle_cache[key]
