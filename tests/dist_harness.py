"""Process groups for the distributed tests: ``spawn_gloo`` runs a function on every rank of a
gloo group of spawned CPU processes, ``rccl_loopback`` is a one-rank "nccl" (= RCCL) group in the
calling process."""
import contextlib
import os
import queue
import socket
import time
import traceback

import torch.distributed as dist
import torch.multiprocessing as mp


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _entry(rank, world, port, target, args, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        q.put((rank, True, target(rank, world, *args)))
    except BaseException as e:  # noqa: BLE001 - reported to the parent instead of a queue timeout
        q.put((rank, False, f"{e!r}\n{traceback.format_exc()}"))
        raise
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def spawn_gloo(target, world, *args, timeout=300):
    """``target(rank, world, *args)`` (a module-level function) on every rank of a gloo group;
    returns the ranks' results in rank order.  Fails at once, with the worker's message, when a
    rank raised, and when one died without a word."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_entry, args=(r, world, port, target, args, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results, deadline = {}, time.monotonic() + timeout
    try:
        while len(results) < world:
            # looked at before the queue: what a rank reported before it died is in the pipe by now
            dead = {r: p.exitcode for r, p in enumerate(procs)
                    if r not in results and p.exitcode is not None}
            try:
                rank, ok, res = q.get(timeout=1)
            except queue.Empty:
                assert not dead, f"ranks died without a result (rank: exit code): {dead}"
                assert time.monotonic() < deadline, f"no result within {timeout} s"
                continue
            assert ok, f"rank {rank} raised {res}"
            results[rank] = res
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():  # only after a failure: a rank waiting in a collective for a dead one
                p.kill()
    return [results[r] for r in range(world)]


@contextlib.contextmanager
def rccl_loopback(dev):
    """A one-rank "nccl" process group on device ``dev``; skips the test if the process already
    has a group."""
    import pytest
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{free_port()}", rank=0,
                            world_size=1, device_id=dev)
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()
