"""Pixel observations: the numpy restatement of what ``mrp_pixels`` computes on the device.

The reference declares an ``'image'`` observation type next to ``'low-dim'``
(``multi_robot_puzzle_00.py:148-162``): ``obs_depth`` frames stacked vertically into a uint8 box
``(VIEWPORT_H * obs_depth, VIEWPORT_W, 3)`` that starts from ``np.zeros`` (``:197-200``).  Its own
``step()`` never fills that state, so the stack rule below is this build's definition (parity
unpinned): the newest frame goes to the bottom, the others move up by one, and an episode's first
stack has zeros above its first frame.

``csrc/mrp_pixels.h`` (``k_pixels``) renders the frame and applies the rule for every lane in one
launch; the functions here say the same in numpy and are what the tests compare it with.
"""
from __future__ import annotations

import numpy as np

LUMA = (77, 150, 29)   # integer BT.601 weights, sum 256: white -> 255, grey 128, wall 51, goal blue 136


def to_gray(rgb) -> np.ndarray:
    """uint8 [..., 3] -> uint8 [..., 1]: (77 R + 150 G + 29 B + 128) >> 8 in integer arithmetic."""
    c = np.asarray(rgb).astype(np.uint32)
    y = (LUMA[0] * c[..., 0] + LUMA[1] * c[..., 1] + LUMA[2] * c[..., 2] + 128) >> 8
    return y.astype(np.uint8)[..., None]


def stack_shape(width: int, height: int, channels: int, depth: int) -> tuple:
    """Shape of one lane's observation: ``depth`` frames stacked vertically."""
    return (int(depth) * int(height), int(width), int(channels))


def advance(prev, frames, done=None, depth: int | None = None) -> np.ndarray:
    """The next stacks, uint8 [n, depth*H, W, C], from the previous stacks and the new frames
    uint8 [n, H, W, C].  Every lane's frames move up by one slot and the new frame takes the bottom
    slot; a lane whose ``done`` entry is nonzero starts afresh, with zeros above its new frame.
    ``prev=None`` means that every lane starts afresh; ``depth`` then gives the number of slots
    (otherwise it is read from ``prev``)."""
    frames = np.asarray(frames, np.uint8)
    n, h = frames.shape[0], frames.shape[1]
    if prev is None:
        if depth is None:
            raise ValueError("advance: give depth when there is no previous stack")
        prev = np.zeros((n, depth * h) + frames.shape[2:], np.uint8)
        done = np.ones(n, np.uint8)
    prev = np.asarray(prev, np.uint8)
    depth = prev.shape[1] // h
    if depth < 1 or prev.shape != (n, depth * h) + frames.shape[2:]:
        raise ValueError(f"advance: stacks {prev.shape} do not hold frames {frames.shape}")
    out = np.zeros_like(prev)
    out[:, :(depth - 1) * h] = prev[:, h:]
    if done is not None:
        out[np.asarray(done).reshape(n) != 0, :(depth - 1) * h] = 0
    out[:, (depth - 1) * h:] = frames
    return out
