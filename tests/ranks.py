"""The one harness of the multi-process tests: `run_ranks` starts a world of rank processes on a worker function and returns what
each rank returned; `one_rank_group` opens the same process group inside the calling process.

What `run_ranks` guarantees: a test fails as soon as a rank has reported an exception or has died without reporting (within about
a second, not at the limit), the failure names every rank's traceback and every exit code known by then, and when it returns or
raises none of its processes is alive and its rendezvous file is gone.  Nothing here tries anything twice."""
import contextlib
import os
import queue
import tempfile
import time
import traceback

JOIN = 180      # s for all ranks to exit once every report is in: the longest bound the call sites used (the eight-rank tests')


@contextlib.contextmanager
def _group(backend, rank, world, rdv, timeout=None):
    """The default process group over the rendezvous FILE `rdv` (no TCP port to collide on), destroyed on the way out.  "nccl" is
    the one-rank RCCL group on cuda:0 — RCCL refuses a second rank on a device."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    kw = {}
    if backend == "nccl":
        import torch
        assert world == 1, world
        kw["device_id"] = torch.device("cuda", 0)
    if timeout is not None:
        from datetime import timedelta
        kw["timeout"] = timedelta(seconds=timeout)
    dist.init_process_group(backend, init_method=f"file://{rdv}", rank=rank, world_size=world, **kw)
    try:
        yield
    finally:
        dist.destroy_process_group()


@contextlib.contextmanager
def one_rank_group(backend="nccl"):
    """A one-rank process group in THIS process, for tests that need a real communicator and no second rank."""
    rdv = tempfile.mktemp(prefix="mke_rdv_")
    try:
        with _group(backend, 0, 1, rdv):
            yield
    finally:
        if os.path.exists(rdv):
            os.unlink(rdv)


def _entry(rank, world, rdv, ret, backend, group_timeout, env, target, args):
    """A rank process: the group, `target`, its value — or its traceback — to the parent."""
    try:
        os.environ.update(env or {})
        with _group(backend, rank, world, rdv, group_timeout):
            ret.put(("ok", rank, target(rank, world, *args)))
    except Exception:   # noqa: BLE001 — reported to the parent, which fails the test with the text
        ret.put(("error", rank, traceback.format_exc()))
        raise


def run_ranks(world, target, args=(), *, limit, backend="gloo", group_timeout=None, env=None):
    """`target(rank, world, *args)` in `world` spawned processes inside one process group -> {rank: what it returned}.

    `target` is a module-level function without process-group or queue code.  `limit`: seconds for every rank to report.
    `group_timeout`: the collectives' own limit in seconds (default: the backend's); `env`: set in every rank before the group opens.
    Raises AssertionError (see the module's docstring) when a rank fails, dies, is late or exits with a non-zero code."""
    import torch.multiprocessing as mp
    assert 1 <= world <= 15, world      # the parent may hold the GPU too, and a box allows 16 processes with the GPU open
    rdv = tempfile.mktemp(prefix="mke_rdv_")
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=_entry, args=(r, world, rdv, ret, backend, group_timeout, env, target, args)) for r in range(world)]
    reports, errors = {}, {}

    def seen(what):
        codes = {r: p.exitcode for r, p in enumerate(procs) if p.exitcode is not None}
        text = "".join(f"\n--- rank {r} raised:\n{errors[r]}" for r in sorted(errors))
        return f"{what}; exit codes of the ranks that have ended: {codes}{text}"

    try:
        for p in procs:
            p.start()
        t_end = time.monotonic() + limit
        while len(reports) + len(errors) < world:
            # exit codes are read BEFORE the queue: what a rank put before it ended is in the pipe by then
            ended = [r for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
            try:
                kind, rank, value = ret.get(timeout=1.0)
                (reports if kind == "ok" else errors)[rank] = value
                continue                # take what is there first: the rank at fault is often not the first to report
            except queue.Empty:
                pass
            assert not errors, seen(f"rank {sorted(errors)[0]} failed")
            silent = [r for r in ended if r not in reports and r not in errors]
            assert not silent, seen(f"ranks {silent} ended without reporting")
            late = [r for r in range(world) if r not in reports]
            assert time.monotonic() < t_end, seen(f"ranks {late} did not report within {limit} s")
        assert not errors, seen(f"rank {sorted(errors)[0]} failed")
        t_end = time.monotonic() + JOIN
        for p in procs:
            p.join(max(0.0, t_end - time.monotonic()))
        bad = [r for r, p in enumerate(procs) if p.exitcode != 0]
        assert not bad, seen(f"ranks {bad} reported but did not exit with 0 within {JOIN} s")
        return reports
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
            if p.is_alive():
                p.kill()
                p.join(10)
        if os.path.exists(rdv):
            os.unlink(rdv)
