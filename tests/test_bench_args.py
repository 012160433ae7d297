"""bench.py's command line: a plain run does only the headline, --full adds the side runs (no GPU needed)."""
import pytest

import bench


def test_plain_run_has_no_side_runs():
    a = bench.parse_args(["--gpus", "1", "--steps", "10", "--warmup", "2"])
    assert a.full is False and a.other_configs == "none" and a.default_workload


def test_full_default_workload_carries_the_other_configs():
    assert bench.parse_args(["--full"]).other_configs == "full"
    assert bench.parse_args(["--full", "--batch", "64"]).other_configs == "none"
    assert bench.parse_args(["--full", "--config", "ann"]).other_configs == "none"
    assert bench.parse_args(["--full", "--other-configs", "small"]).other_configs == "small"


@pytest.mark.parametrize("which", ["full", "small"])
def test_other_configs_need_full(which):
    with pytest.raises(SystemExit):
        bench.parse_args(["--other-configs", which])
