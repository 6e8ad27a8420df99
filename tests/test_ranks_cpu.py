"""tests/ranks.py itself, under gloo on the CPU: the reports come back, and a rank that raises, a rank that dies without a word and
ranks that never answer each fail the test with the evidence in the message — the first two long before the limit — and leave
no process behind.  A planted Python exception and a planted exit code are all the failure there is here."""
import multiprocessing
import os
import time

import pytest

import ranks


def _sum_worker(rank, world, k):
    import torch
    import torch.distributed as dist
    assert os.environ["MKE_RANKS_TEST"] == "set"
    x = torch.tensor([float(rank + k)])
    dist.all_reduce(x)
    return float(x)


def _raise_worker(rank, world):
    import torch.distributed as dist
    if rank == 1:
        raise ValueError("planted")
    dist.barrier()


def _exit_worker(rank, world):
    import torch.distributed as dist
    if rank == 1:
        os._exit(3)
    dist.barrier()


def _sleep_worker(rank, world):
    time.sleep(600)


def _rdv_files():
    import glob
    import tempfile
    return set(glob.glob(os.path.join(tempfile.gettempdir(), "mke_rdv_*")))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_reports_and_nothing_is_left(world):
    before = _rdv_files()
    got = ranks.run_ranks(world, _sum_worker, (5,), limit=120, env={"MKE_RANKS_TEST": "set"})
    v = float(sum(r + 5 for r in range(world)))
    assert got == {r: v for r in range(world)}
    assert multiprocessing.active_children() == []
    assert _rdv_files() <= before


@pytest.mark.timeout(120)
def test_a_rank_that_raises_fails_the_test_at_once_with_its_traceback():
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        ranks.run_ranks(2, _raise_worker, limit=120)
    assert time.monotonic() - t0 < 60
    text = str(e.value)
    assert "planted" in text and "ValueError" in text and "rank 1" in text
    assert multiprocessing.active_children() == []


@pytest.mark.timeout(120)
def test_a_rank_that_dies_without_reporting_is_named_with_its_exit_code():
    """Rank 0's collective may fail first and report first: the message still shows who ended with what."""
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        ranks.run_ranks(2, _exit_worker, limit=120)
    assert time.monotonic() - t0 < 60
    assert "1: 3" in str(e.value).split("exit codes of the ranks that have ended: ")[1].splitlines()[0]
    assert multiprocessing.active_children() == []


@pytest.mark.timeout(120)
def test_ranks_that_never_report_end_at_the_limit():
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as e:
        ranks.run_ranks(2, _sleep_worker, limit=15)
    assert time.monotonic() - t0 < 15 + 2 * (10 + 10) + 5       # the limit, terminate + kill bounds per rank, slack
    assert "ranks [0, 1] did not report within 15 s" in str(e.value)
    assert multiprocessing.active_children() == []
