"""One way to start ranks: gloo ranks of a CPU test as spawned processes, and the ranks of a GPU test as fresh
interpreters under torch.distributed.run.  A support module; it holds no tests."""
from __future__ import annotations

import os
import queue
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 240       # seconds spawn() waits for the ranks' results at most


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn(target, world, *args, n_results=None):
    """Runs ``target(rank, world, port, *args, q)`` in ``world`` spawned processes and returns what they put into
    the queue ``q``: one result per rank, or ``n_results`` of them (a gather to rank 0 alone gives one).  A rank
    that died ends the wait at once with the exit codes; the whole wait is capped at CAP seconds."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    results, end = [], time.monotonic() + CAP
    while len(results) < (world if n_results is None else n_results):
        try:
            results.append(q.get(timeout=0.2))
        except queue.Empty:
            codes = [p.exitcode for p in procs]
            if any(c not in (None, 0) for c in codes) or time.monotonic() > end:
                for p in procs:
                    p.kill()
                    p.join()
                raise AssertionError(f"a rank died, or no result came within {CAP} s: exit codes {codes}") from None
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return results


def torchrun(script, nproc, *script_args, env=None, timeout=280):
    """Runs ``script`` (a path below the repository root) under torch.distributed.run with ``nproc`` ranks on this
    node, from the repository root, with ``env`` added to the environment; returns the completed process after
    asserting that it exited with 0."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, script), *map(str, script_args)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r
