"""Pixel observations, CPU side: the C ABI names, the device-free argument check, and the numpy
restatement (gym_puzzles_amd/pixels.py) of the luma formula and the frame-stack rule that
tests/test_pixels_gpu.py compares the kernel with.
"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mrp.h")
NAMES = ("mrp_pixels", "mrp_pixels_device")


@pytest.fixture(scope="module")
def lib():
    from gym_puzzles_amd import build as b
    b.build()                       # no-op when up to date
    from gym_puzzles_amd import _native
    return _native.load()


def test_header_library_and_binding_name_the_entry_points(lib):
    from gym_puzzles_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrp_[a-z_0-9]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED, name
        assert len(getattr(lib, name).argtypes) == 8, name


def test_null_context_is_refused_without_a_device(lib):
    assert lib.mrp_pixels_device(None, 84, 84, 1, 3, None, None, None) == -1   # MRP_E_ARG
    assert b"mrp_pixels" in lib.mrp_last_error(None)
    assert lib.mrp_pixels(None, 84, 84, 1, 3, None, None, None) == -1


def test_pixels_header_is_a_build_dependency():
    from gym_puzzles_amd import build as b
    assert "mrp_pixels.h" in b.HEADERS
    assert os.path.join(b.CSRC, "mrp_pixels.h") in b.deps()


def test_to_gray_keeps_the_scene_colours_apart():
    from gym_puzzles_amd.pixels import to_gray
    rgb = np.array([[255, 255, 255], [128, 128, 128], [51, 51, 51], [58, 153, 255], [0, 0, 0]], np.uint8)
    g = to_gray(rgb)
    assert g.dtype == np.uint8 and g.shape == (5, 1)
    assert g[:, 0].tolist() == [255, 128, 51, 136, 0]
    img = np.arange(2 * 3 * 4 * 3, dtype=np.uint8).reshape(2, 3, 4, 3)
    assert to_gray(img).shape == (2, 3, 4, 1)
    r, gr, b = (int(v) for v in img[1, 2, 3])
    assert int(to_gray(img)[1, 2, 3, 0]) == (77 * r + 150 * gr + 29 * b + 128) >> 8


def test_stack_shape():
    from gym_puzzles_amd.pixels import stack_shape
    assert stack_shape(21, 13, 3, 2) == (26, 21, 3)
    assert stack_shape(84, 84, 1, 4) == (336, 84, 1)


def test_advance_shifts_clears_and_starts():
    from gym_puzzles_amd.pixels import advance
    H, W, C, depth = 2, 3, 1, 3
    prev = np.zeros((2, depth * H, W, C), np.uint8)
    for lane in range(2):
        for k in range(depth):
            prev[lane, k * H:(k + 1) * H] = 10 * (lane + 1) + k     # lane 0: 10 11 12, lane 1: 20 21 22
    frames = np.stack([np.full((H, W, C), 13, np.uint8), np.full((H, W, C), 23, np.uint8)])
    before = prev.copy()

    out = advance(prev, frames, done=np.array([0, 1], np.uint8))
    assert out.shape == prev.shape and out.dtype == np.uint8
    assert [int(out[0, k * H, 0, 0]) for k in range(depth)] == [11, 12, 13]     # undone: shifted by one slot
    assert [int(out[1, k * H, 0, 0]) for k in range(depth)] == [0, 0, 23]       # done: only the newest slot
    for lane in range(2):
        for k in range(depth):
            slot = out[lane, k * H:(k + 1) * H]
            assert (slot == slot[0, 0, 0]).all()
    assert (prev == before).all(), "advance leaves its input alone"

    out = advance(prev, frames)                                                # done=None: nobody ended
    assert [int(out[1, k * H, 0, 0]) for k in range(depth)] == [21, 22, 23]

    fresh = advance(None, frames, depth=depth)                                 # no previous stack: all lanes start
    assert (fresh == advance(prev, frames, done=np.ones(2, np.uint8))).all()
    assert [int(fresh[0, k * H, 0, 0]) for k in range(depth)] == [0, 0, 13]
    assert (advance(None, frames, depth=1) == frames).all()
    with pytest.raises(ValueError):
        advance(None, frames)
