"""What at least three of the tools/time_*.py scripts share: the import path, the 3 x 3 training grid and its snapshots
built on the device with the list of training runs split from them, the bench's parameter draw, the warm-up plus
event-timed repetitions of one route or of several alternately, the tail of the report line, and the decoder of the
phase-clock record.  What a script measures, its options and its FLOP count stay in the script."""
import collections
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path[:0] = [REPO, os.path.join(REPO, "1d-burgers-equation-roms_amd")]
import numpy as np, torch

PEAK = 78.6e12                                             # fp64 matrix peak of one MI355X, FLOP/s
TRAIN_MU1, TRAIN_MU2 = np.repeat(np.linspace(4.25, 5.5, 3), 3), np.tile(np.linspace(0.015, 0.03, 3), 3)      # the 3 x 3 training grid


def training_snapshots(N, dt, steps=200):
    """(X, S): the uniform mesh and the snapshot matrix of the FOM runs of the 3 x 3 training grid, on the device."""
    from burgers_hip import fom, pod
    X = np.linspace(0, 100, N)
    return X, pod.snapshot_matrix(fom.fom_run(X, np.ones(N), TRAIN_MU1, TRAIN_MU2, dt, steps).hist).contiguous()


def training_list(S, host=False):
    """The ``runs`` of the pod.build_*_row_sampling functions, (hist (N, nT+1), mu1, mu2) per training point, split from the
    snapshot matrix ``S`` of training_snapshots; ``host``: every hist as a host copy."""
    T1 = S.shape[1] // 9
    hists = [S[:, k * T1:(k + 1) * T1] for k in range(9)]
    return [(h.cpu() if host else h, TRAIN_MU1[k], TRAIN_MU2[k]) for k, h in enumerate(hists)]


def draw(B, seed=20251121):
    rng = np.random.default_rng(seed)
    return rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B)


def time_runs(run, reps=1):
    """One warm-up call of ``run``, then ``reps`` calls between HIP events: (ms, res), the milliseconds of each repetition
    and the last result."""
    run(); torch.cuda.synchronize()                                 # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); res = run(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms, res


def time_alternately(runs, reps):
    """The routes ``runs`` {name: callable} timed alternately in one process: one warm-up of each (code objects, library
    handles, allocator), then ``reps`` rounds with every call between HIP events.  Returns (rates, last): the
    sample-Newton-steps/s of every repetition and the last result, by name."""
    rates, last = {k: [] for k in runs}, {}
    for f in runs.values():
        f(); torch.cuda.synchronize()
    for _ in range(reps):
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); last[k] = f(); e1.record(); torch.cuda.synchronize()
            rates[k].append(int(last[k].iters.sum().item()) / e0.elapsed_time(e1) * 1e3)
    return rates, last


def rates_of(ms, res):
    """Sample-Newton-steps/s of each repetition (every repetition of a run does the iterations of the last)."""
    its = int(res.iters.sum().item())
    return [its / t * 1e3 for t in ms]


def rates_text(rates):
    return ", ".join(f"{v:.3g}" for v in rates) + f" -> median {float(np.median(rates)):.3g} sample-Newton-steps/s"


PhaseReport = collections.namedtuple("PhaseReport", "per_pass total passes mhz")


def phase_report(res, names, passes_per_step=None):
    """Decode the record PhaseClock<ON, SLOTS>::store (csrc/wave_ops.hpp) leaves at the head of every row of ``res.iters``
    in a clock build (-DBG_PHASE_CLOCK, or -DBG_FUSED_ABLATE=bits for the fused loops); SLOTS = len(names):
      [0, SLOTS) kilo-clocks (units of 1024) per phase | [SLOTS] passes | [SLOTS + 1] shader kilo-clocks and
      [SLOTS + 2] 100 MHz kilo-ticks of the whole sample.
    Returns the medians over the samples: per_pass, the thousands of shader clocks per pass of each phase; their total;
    the passes per sample; the in-kernel clock in MHz.  ``passes_per_step``: the ablation builds' fixed iterations per
    time step, which then replace the counted passes."""
    slots, steps = len(names), res.iters.shape[1]
    if steps < slots + 3:
        raise ValueError(f"the phase-clock record of {slots} phases needs {slots + 3} time steps; the run had {steps}")
    it = res.iters[:, :slots + 3].double().cpu().numpy()
    passes = float(np.median(it[:, slots])) if passes_per_step is None else float(passes_per_step * steps)
    per_pass = np.median(it[:, :slots], axis=0) * 1.024 / passes
    return PhaseReport(per_pass, float(per_pass.sum()), passes, float(np.median(it[:, slots + 1] / it[:, slots + 2])) * 100.0)


def peak_text(rates, flop):
    """``flop``: floating-point operations per sample-Newton-step."""
    return f"{float(np.median(rates)) * flop / PEAK:.3f} of the 78.6 TFLOP/s fp64 matrix peak"
