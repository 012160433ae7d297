"""The round-robin ordering bg_jacobi_sweep runs (pod._round_robin): a sweep must meet every row pair exactly once,
and the pairs of one step must be disjoint (one workgroup per pair rotates two rows in place).  A pair left out
would keep its rows unorthogonalised, and the sweeps would end at the limit without converging."""
import itertools

import numpy as np
import pytest


@pytest.mark.parametrize("m", [1, 2, 3, 7, 256, 257, 777])
def test_round_robin_meets_every_pair_once(m):
    from burgers_hip import pod
    steps = pod._round_robin(m).numpy()
    n = m + (m & 1)
    assert steps.dtype == np.int32 and steps.shape == (max(n - 1, 0), n // 2, 2)
    seen = np.zeros((m, m), dtype=np.int64)
    for st in steps:
        live = st[(st >= 0).all(1)]
        assert (st >= -1).all() and (st < m).all()
        # a bye (-1) only ever faces the dummy player of an odd m, at most once per step
        assert len(st) - len(live) == (m & 1)
        rows = live.ravel()
        assert len(np.unique(rows)) == len(rows), "a row appears twice in one step"
        assert (live[:, 0] != live[:, 1]).all()
        lo, hi = live.min(1), live.max(1)
        np.add.at(seen, (lo, hi), 1)
    want = np.triu(np.ones((m, m), dtype=np.int64), 1)
    assert np.array_equal(seen, want), "a sweep must pair every unordered row pair exactly once"


def test_round_robin_small_cases_by_hand():
    from burgers_hip import pod
    pairs = lambda m: [sorted(tuple(sorted(p)) for p in st.tolist() if min(p) >= 0) for st in pod._round_robin(m).numpy()]
    assert pairs(1) == [[]]                                    # one step, the single row against the bye
    assert pairs(2) == [[(0, 1)]]
    got = sorted(itertools.chain.from_iterable(pairs(3)))
    assert got == [(0, 1), (0, 2), (1, 2)]
