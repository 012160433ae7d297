"""tools/_timing.phase_report against a record written by hand in the layout of PhaseClock::store (csrc/wave_ops.hpp):
[0, SLOTS) kilo-clocks per phase, [SLOTS] passes, [SLOTS + 1] shader kilo-clocks, [SLOTS + 2] 100 MHz kilo-ticks.
Every expected figure below is exact in binary64 (k * 1.024 is a whole number for the multiples of 125 used)."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from _timing import phase_report  # noqa: E402

NAMES = ["a", "b", "c", "d"]
# shader clocks per phase, as the device accumulates them (the record keeps clocks >> 10: the remainders must not show)
CYCLES = [[1250 * 1024 + 1023, 5000 * 1024, 0, 625 * 1024 + 7],
          [2500 * 1024, 2500 * 1024 + 512, 1023, 625 * 1024],
          [3750 * 1024 + 1, 7500 * 1024, 0, 1250 * 1024]]
PASSES = [10, 20, 40]
TOTAL_CLOCKS = [8000 * 1024, 6000 * 1024 + 100, 13000 * 1024]
TICKS = [400 * 1024, 250 * 1024, 520 * 1024 + 3]          # 2000, 2400, 2500 MHz


def record(steps):
    it = torch.full((3, steps), 3, dtype=torch.int32)      # what is not overwritten stays an iteration count
    for s in range(3):
        row = [c >> 10 for c in CYCLES[s]] + [PASSES[s], TOTAL_CLOCKS[s] >> 10, TICKS[s] >> 10]
        it[s, :min(steps, 7)] = torch.tensor(row[:steps], dtype=torch.int32)
    return types.SimpleNamespace(iters=it)


def test_medians_per_counted_pass():
    rep = phase_report(record(8), NAMES)
    assert rep.per_pass.tolist() == [128.0, 256.0, 0.0, 32.0]       # medians 2500, 5000, 0, 625 k over the median 20 passes
    assert rep.total == 416.0
    assert rep.passes == 20.0
    assert rep.mhz == 2400.0


def test_fixed_passes_per_step():
    rep = phase_report(record(8), NAMES, passes_per_step=5)          # the ablation builds: 5 iterations x 8 steps
    assert rep.per_pass.tolist() == [64.0, 128.0, 0.0, 16.0]
    assert rep.total == 208.0
    assert rep.passes == 40.0
    assert rep.mhz == 2400.0


def test_short_run_is_refused():
    with pytest.raises(ValueError, match=r"\b7\b"):
        phase_report(record(6), NAMES)
