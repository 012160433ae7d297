import os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "1d-burgers-equation-roms_amd"))
sys.path.insert(0, REPO)
import numpy as np, torch
from burgers_hip import rom, fom, pod
N = 512; X = np.linspace(0, 100, N)
m1, m2 = np.meshgrid(np.linspace(4.25, 5.5, 3), np.linspace(0.015, 0.03, 3), indexing="ij")
res = fom.fom_run(X, np.ones(N), m1.ravel(), m2.ravel(), 0.05, 500)
S = pod.snapshot_matrix(res.hist).contiguous()
rng = np.random.default_rng(0)
for r, B in ((96, 1024), (160, 512)):
    Phi, s, _ = pod.pod_basis(S, n_modes=r)
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    for proj in ("Galerkin", "LSPG"):
        rom.pod_prom_run(X, np.ones(N), mu1[:16], mu2[:16], 0.05, 2, Phi, projection=proj)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = rom.pod_prom_run(X, np.ones(N), mu1, mu2, 0.05, 20, Phi, projection=proj)
        torch.cuda.synchronize(); t = time.perf_counter() - t0
        steps = int(out.iters.sum())
        print(f"library path r={r} {proj:8s} B={B}: {steps/t:.3e} sample-Newton-steps/s, {t*1e3:.1f} ms, iters/step {steps/(B*20):.2f}")
