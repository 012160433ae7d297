"""What the tests of the hyper-reduced POD-ANN loop for up to 20 primary modes (bg_hyper_ann_rom_run_wide) share: the
entry's name and the cases, as tuples of the hyper_ann_ref.CASES form (hyper_ann_ref.case_data takes them as they are).
numpy only at import."""
import numpy as np

ENTRY = "bg_hyper_ann_rom_run_wide"
NARROW = "bg_hyper_ann_rom_run"
NT = 6
LIMITS = (20, 128, 256, 8, 256, 768)
# name: N, dt, n, nbar, hidden widths, seed of the closure, scale, E, seed of the mesh (None: uniform)
CASES = {
    "wide-full-256": (256, 0.05, 17, 79, (32, 64, 128, 256, 256), 529, 3.0, 0.0, None),     # the reference's second model size
    "wide-perturbed-96": (96, 0.05, 20, 40, (33,), 532, 3.0, 0.01, 7),                      # n at the limit, a ragged width
}
# the thesis shape on the POD basis of a mesh beyond every other POD-ANN loop
LONG17 = (2049, 0.0125, 17, 79, (32, 64, 128, 256, 256), 529, 3.0, 0.0, None)
LEFT_OUT = [10, 50, 51, 70]


def sampling(rows, xi, proj):
    from burgers_hip import pod
    return pod.RowSampling(np.asarray(rows, dtype=np.int32), np.asarray(xi, dtype=np.float64), proj.lower(), 0.0, 0, 0.0)
