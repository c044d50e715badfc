"""CPU checks of gym_puzzles_amd/_device.py's check_tensors: what it refuses without a device, in which order,
and how it treats an optional entry.  (What it accepts needs CUDA tensors: tests/test_envs.py, tests/test_norm.py.)
And of the tests' own rank launcher, tests/ranks.py spawn: a rank that dies is reported at once."""
from __future__ import annotations

import numpy as np
import pytest


def test_check_tensors_rejections_and_optional():
    import torch

    from gym_puzzles_amd._device import check_tensors
    dev, f32 = torch.device("cuda", 0), torch.float32
    check_tensors("who", dev, ())
    check_tensors("who", dev, (("a", None, f32, (2,), True), ("b", None, torch.uint8, (2, 3), True)))    # None passes when optional
    with pytest.raises(ValueError, match="^who: a is not a tensor$"):
        check_tensors("who", dev, (("a", None, f32, (2,), False),))
    for optional in (False, True):            # a given value is checked either way
        with pytest.raises(ValueError, match="^who: b is not a tensor$"):
            check_tensors("who", dev, (("a", None, f32, (2,), True), ("b", np.zeros(2, np.float32), f32, (2,), optional)))
        with pytest.raises(ValueError, match="^who: a is on cpu, expected cuda:0$"):
            check_tensors("who", dev, (("a", torch.zeros(2), f32, (2,), optional),))
    with pytest.raises(ValueError, match="^who: a is on cpu"):     # the first bad entry is the one reported
        check_tensors("who", dev, (("a", torch.zeros(2), f32, (2,), False), ("b", 3, f32, (2,), False)))


def _dies(rank, world, port, q):
    raise SystemExit(3)


def test_spawn_reports_a_dead_rank():
    """ranks.spawn ends its wait as soon as a rank has died and names the exit code: no process group is
    formed here, and nothing waits for the 240 s cap."""
    import time

    from ranks import spawn
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match=r"exit codes \[3\]"):
        spawn(_dies, 1)
    assert time.monotonic() - t0 < 10
