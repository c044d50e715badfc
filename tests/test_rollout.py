"""CPU checks of the rollout layer (gym_puzzles_amd/rollout.py, mrp_gae_device): the numpy rule
gae_ref on hand-computed cases, the dtype promotion the kernel is built from, and the argument
checks of the C entry point that run before any HIP call.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from gym_puzzles_amd.rollout import gae_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64

# T=3, N=2, gamma = gae_lambda = 0.5: every value below is a small dyadic rational, exact in float32.
# Lane 0 runs through; lane 1 starts a new episode at row 2 and is done after the last row.
R = np.array([[1, 2], [3, 4], [5, 6]], f32)
V = np.array([[0.5, 1], [1.5, 2], [2.5, 3]], f32)
ES = np.array([[1, 1], [0, 0], [0, 1]], f32)
LV = np.array([4, 8], f32)
DONES = np.array([False, True])


def test_gae_ref_hand_values():
    # lane 0: d2 = 5 + .5*4 - 2.5 = 4.5; d1 = 3 + .5*2.5 - 1.5 = 2.75; d0 = 1 + .5*1.5 - .5 = 1.25
    #         A2 = 4.5, A1 = 2.75 + .25*4.5 = 3.875, A0 = 1.25 + .25*3.875 = 2.21875
    # lane 1: d2 = 6 - 3 = 3 (done: last_values ignored); d1 = 4 - 2 = 2 (row 2 starts an episode: no
    #         bootstrap from values[2], no propagation of A2); d0 = 2 + .5*2 - 1 = 2, A0 = 2 + .25*2 = 2.5
    adv, ret = gae_ref(R, V, ES, LV, DONES, 0.5, 0.5)
    assert adv.dtype == np.float32 and ret.dtype == np.float32
    assert np.array_equal(adv, np.array([[2.21875, 2.5], [3.875, 2], [4.5, 3]], f32))
    assert np.array_equal(ret, np.array([[2.71875, 3.5], [5.375, 4], [7, 6]], f32))


def test_gae_ref_lambda_zero_gives_td_errors():
    adv, ret = gae_ref(R, V, ES, LV, DONES, 0.5, 0.0)
    assert np.array_equal(adv, np.array([[1.25, 2], [2.75, 2], [4.5, 3]], f32))
    assert np.array_equal(ret, adv + V)


def test_gae_ref_done_ignores_last_values():
    a, _ = gae_ref(R, V, ES, LV, DONES, 0.5, 0.5)
    b, _ = gae_ref(R, V, ES, np.array([4, -1000], f32), DONES, 0.5, 0.5)
    assert np.array_equal(a, b)
    c, _ = gae_ref(R, V, ES, LV, np.array([0, 1], np.uint8), 0.5, 0.5)   # dones are cast with astype(bool)
    assert np.array_equal(a, c)
    d, _ = gae_ref(R, V, ES, LV, np.array([False, False]), 0.5, 0.5)
    assert d[2, 1] == 3 + 0.5 * 8 and d[2, 0] == a[2, 0]


def test_gae_ref_episode_start_cuts_the_chain():
    """Lane 1's rows 0-1 see nothing of row 2 or of what follows it."""
    R2, V2 = R.copy(), V.copy()
    R2[2, 1], V2[2, 1] = 77, -5
    a, _ = gae_ref(R, V, ES, LV, DONES, 0.5, 0.5)
    b, _ = gae_ref(R2, V2, ES, LV, DONES, 0.5, 0.5)
    assert np.array_equal(a[:2], b[:2]) and a[2, 1] != b[2, 1]


def test_gae_ref_truncation_bootstrap():
    """truncated + terminal_values equals adding float32(gamma) * tv to the rewards beforehand; the
    inputs are left as they were."""
    trunc = np.array([[0, 0], [0, 1], [0, 0]], np.uint8)
    tv = np.array([[9, 9], [9, 8], [9, 9]], f32)      # only [1, 1] is marked
    r0 = R.copy()
    adv, ret = gae_ref(R, V, ES, LV, DONES, 0.5, 0.5, trunc, tv)
    assert np.array_equal(R, r0)
    pre = R.copy()
    pre[1, 1] = pre[1, 1] + f32(0.5) * tv[1, 1]
    adv2, ret2 = gae_ref(pre, V, ES, LV, DONES, 0.5, 0.5)
    assert np.array_equal(adv, adv2) and np.array_equal(ret, ret2)
    # lane 1: d1 = 4 + .5*8 - 2 = 6, A1 = 6; A0 = 2 + .25*6 = 3.5; lane 0 untouched
    assert np.array_equal(adv, np.array([[2.21875, 3.5], [3.875, 6], [4.5, 3]], f32))
    assert adv.dtype == np.float32 and ret.dtype == np.float32


def _explicit(r, v, es, lv, dones, gamma, lam):
    """The form k_gae computes (include/mrp.h): float32 constants, a float64 accumulator, every
    operation rounded on its own."""
    g32, c32 = f32(gamma), f32(gamma * lam)
    T = r.shape[0]
    adv = np.zeros_like(r)
    nnt64 = f64(1.0) - dones.astype(bool).astype(f64)
    L = ((r[T - 1].astype(f64) + (g32 * lv).astype(f64) * nnt64) - v[T - 1].astype(f64)) + f64(0.0)
    adv[T - 1] = L.astype(f32)
    for s in reversed(range(T - 1)):
        nnt = f32(1.0) - es[s + 1]
        delta = (r[s] + (g32 * v[s + 1]) * nnt) - v[s]
        step = c32 * nnt
        assert delta.dtype == np.float32 and step.dtype == np.float32
        L = delta.astype(f64) + step.astype(f64) * L
        adv[s] = L.astype(f32)
    return adv, adv + v


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)])
def test_explicit_form_equals_gae_ref_bitwise(seed, gamma, lam):
    rs = np.random.RandomState(seed)
    T, N = 9, 5
    r, v = rs.standard_normal((T, N)).astype(f32), rs.standard_normal((T, N)).astype(f32)
    es = (rs.uniform(size=(T, N)) < 0.3).astype(f32)
    lv, dones = rs.standard_normal(N).astype(f32), rs.uniform(size=N) < 0.5
    want = gae_ref(r, v, es, lv, dones, gamma, lam)
    got = _explicit(r, v, es, lv, dones, gamma, lam)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == np.float32
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


@pytest.fixture(scope="module")
def lib():
    from gym_puzzles_amd import build as b
    b.build()                       # no-op when up to date
    from gym_puzzles_amd import _native
    return _native.load()


def test_library_exports_mrp_gae_device(lib):
    from gym_puzzles_amd import _native
    assert "mrp_gae_device" in _native.EXPORTED and hasattr(lib, "mrp_gae_device")


# made-up, distinct, non-null "device pointers": the refused calls never reach a HIP call
_P = dict(r=0x10000, v=0x20000, es=0x30000, tr=0x40000, tv=0x50000, lv=0x60000, ld=0x70000, adv=0x80000, ret=0x90000)


def _call(lib, T=4, N=8, **over):
    p = dict(_P, **over)
    return lib.mrp_gae_device(0, None, T, N, p["r"], p["v"], p["es"], p["tr"], p["tv"], p["lv"], p["ld"], 0.99, 0.95,
                              p["adv"], p["ret"])


@pytest.mark.parametrize("kw", [dict(T=0), dict(N=0), dict(r=None), dict(tv=None), dict(ret=_P["v"]), dict(adv=_P["ret"])],
                         ids=["n_steps=0", "n_lanes=0", "null rewards", "lone truncated", "returns is values",
                              "advantages is returns"])
def test_mrp_gae_device_refuses_bad_arguments(lib, kw):
    assert _call(lib, **kw) == -1
    assert lib.mrp_norm_last_error(None)


def test_mrp_gae_device_no_cpu_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    assert _call(lib) == -2
    assert b"no HIP device" in lib.mrp_norm_last_error(None)
    assert _call(lib, tr=None, tv=None) == -2


def test_rollout_buffer_is_reachable_without_the_gpu():
    """`gym_puzzles_amd.DeviceRolloutBuffer` resolves lazily, and neither the package nor rollout.py
    imports torch to get there."""
    code = ("import sys, gym_puzzles_amd as g; c = g.DeviceRolloutBuffer; import gym_puzzles_amd.rollout as r; "
            "assert c is r.DeviceRolloutBuffer and callable(r.gae_device); assert 'torch' not in sys.modules; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
