"""bench.py's options without a GPU: what a plain run and --full are told, the timed step count, and which samples of a
batch --dump-outputs writes (a fixed choice, within 64 MB for every BASELINE configuration)."""
import os

import pytest


@pytest.fixture(scope="module")
def bench():
    before = os.environ.get("GPU_MAX_HW_QUEUES")
    import bench as b
    if before is None:  # (bench.py sets the product's launch default on import; the tests' own processes keep theirs)
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    return b


def test_a_plain_run_is_the_default_and_full_is_asked_for(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.steps == 20 and a.warmup == 5 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "some/dir"])
    assert a.full is True and a.dump_outputs == "some/dir"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]])
def test_step_counts_that_time_nothing_are_refused(bench, argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


@pytest.mark.parametrize("config", [1, 2, 3, 4, 5])
def test_dump_selection_is_fixed_and_fits(bench, config):
    cfg = bench.CONFIGS[config]
    B, H, W = cfg["batch"], cfg["H"], cfg["W"]
    which = bench.dump_selection(B, H, W)
    assert which == bench.dump_selection(B, H, W)
    assert which == sorted(set(which)) and len(which) >= 1 and all(0 <= i < B for i in which)
    assert len(which) * 8 * H * W * 4 <= 64 * 2 ** 20
    if B * 8 * H * W * 4 <= bench.DUMP_BYTES:
        assert which == list(range(B))
