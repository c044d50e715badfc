"""ctypes binding of ``libmrp.so`` (the HIP/gfx950 step library; C ABI in ``include/mrp.h``).

The library is built in-tree by ``python -m gym_puzzles_amd.build`` (or
``__graft_entry__.build()``).  There is no CPU fallback: if the shared object is missing
or no HIP device is visible, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._device import Handle
from .spawn import ENV_IDS, ENV_VERSION  # noqa: F401  (ENV_IDS: the package's public name table)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmrp.so")

MRP_OK = 0
STATUS_RUNNING, STATUS_PUZZLE_COMPLETE, STATUS_AGENT_OOB, STATUS_BLOCK_OOB = 0, 1, 2, 3
STATUS_KIND_MASK, STATUS_NONFINITE, STATUS_FAULT = 0x3F, 0x40, 0x80   # include/mrp.h flag bits
COUNTER_NAMES = ("steps", "resets", "toi_events", "position_iterations", "touching_contacts", "nonfinite_steps",
                 "faulted_lanes")

MAXF = 24   # csrc/mrp_config.h: fixtures per env (mrp_shapes fills MAXF rows)

_i, _d, _u64, _P, _f = ctypes.c_int, ctypes.c_double, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_float
_ip, _PP = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)
# The C ABI of include/mrp.h, stated once: name -> (restype, argtypes).  load() applies it, EXPORTED is
# its key list, and tests/test_abi.py compares that list with the header and with the library's exports.
# Every build exports the whole ABI (the diagnostics answer MRP_E_STATE outside their -D builds), so an
# A/B library must be built from this ABI too: a missing symbol raises in load().
ABI = {
    "mrp_env_dims": (_i, [_i, _ip, _ip, _ip, _ip, _ip, _ip]),
    "mrp_create": (_i, [_i, _i, _i, _u64, _u64, _PP]),
    "mrp_destroy": (None, [_P]),
    "mrp_last_error": (ctypes.c_char_p, [_P]),
    "mrp_n_lanes": (_i, [_P]),
    "mrp_env_id": (_i, [_P]),
    "mrp_set_stream": (_i, [_P, _P]),
    "mrp_synchronize": (_i, [_P]),
    "mrp_set_reward_params": (_i, [_P] + [_d] * 7),
    "mrp_update_params": (_i, [_P, _d, _d]),
    "mrp_update_goal": (_i, [_P, _d, _d]),
    "mrp_reset": (_i, [_P] * 5),
    "mrp_reset_device": (_i, [_P] * 5),
    "mrp_step": (_i, [_P] * 8),
    "mrp_step_device": (_i, [_P] * 8),
    "mrp_step_ex": (_i, [_P] * 9),
    "mrp_step_device_ex": (_i, [_P] * 9),
    "mrp_step_n_device": (_i, [_P, _i] + [_P] * 8),
    "mrp_set_auto_reset": (_i, [_P, _i]),
    "mrp_set_frameskip": (_i, [_P, _i]),
    "mrp_set_seed": (_i, [_P, _u64]),
    "mrp_set_schedule": (_i, [_P, _i]),
    "mrp_get_schedule": (_i, [_P]),
    "mrp_set_time_limit": (_i, [_P, _i]),
    "mrp_get_bodies": (_i, [_P, _P]),
    "mrp_get_flags": (_i, [_P, _P]),
    "mrp_get_faults": (_i, [_P, _P]),
    "mrp_counters": (_i, [_P, _P, _P]),
    "mrp_counters_ex": (_i, [_P, _P]),
    "mrp_state_words": (_i, [_i]),
    "mrp_get_state": (_i, [_P, _P]),
    "mrp_set_state": (_i, [_P, _P]),
    "mrp_get_goals": (_i, [_P, _P]),
    "mrp_shapes": (_i, [_i, _P, _P, _P, _P]),
    "mrp_render": (_i, [_P, _P, _i, _i, _i, _P]),
    "mrp_render_device": (_i, [_P, _P, _i, _i, _i, _P]),
    "mrp_pixels": (_i, [_P, _i, _i, _i, _i, _P, _P, _P]),
    "mrp_pixels_device": (_i, [_P, _i, _i, _i, _i, _P, _P, _P]),
    "mrp_selftest_sincos": (_i, [_i, _P, _P, _P, _i]),
    "mrp_debug_stamps": (_i, [_i, _P]),
    "mrp_debug_stamps_ext": (_i, [_i, _P, _P, _P]),
    "mrp_debug_trace": (_i, [_i, _P, _i]),
    "mrp_debug_trace_words": (_i, []),
    "mrp_debug_progress": (_i, [_i, _PP, _i]),
    "mrp_debug_velbench": (_i, [_i, _i, _i, _i, _i, _P]),
    "mrp_debug_posbench": (_i, [_i, _i, _i, _i, _i, _P]),
    "mrp_norm_create": (_i, [_i, _i, _i, _d, _d, _d, _d, _PP]),
    "mrp_norm_destroy": (None, [_P]),
    "mrp_norm_last_error": (ctypes.c_char_p, [_P]),
    "mrp_norm_set_stream": (_i, [_P, _P]),
    "mrp_norm_set_training": (_i, [_P, _i]),
    "mrp_norm_set_norm_obs": (_i, [_P, _i]),
    "mrp_norm_reset_device": (_i, [_P, _P, _P]),
    "mrp_norm_step_device": (_i, [_P] * 10),
    "mrp_norm_step_device_ex": (_i, [_P] * 11),
    "mrp_norm_part_len": (_i, [_i]),
    "mrp_norm_local_device": (_i, [_P, _P, _P, _i, _P]),
    "mrp_norm_apply_device": (_i, [_P, _i, _P, ctypes.c_longlong, _i] + [_P] * 10),
    "mrp_norm_get_stats": (_i, [_P, _P]),
    "mrp_norm_set_stats": (_i, [_P, _P]),
    "mrp_gae_device": (_i, [_i, _P, _i, _i] + [_P] * 7 + [_d, _d, _P, _P]),
    "mrp_policy_create": (_i, [_i] * 6 + [_ip, _i, _PP]),
    "mrp_policy_destroy": (None, [_P]),
    "mrp_policy_last_error": (ctypes.c_char_p, [_P]),
    "mrp_policy_n_params": (_i, [_P]),
    "mrp_policy_set_params": (_i, [_P, _P, _P]),
    "mrp_policy_act_device": (_i, [_P, _P, _i, _P, _P, _u64, _u64, _u64, _i] + [_P] * 5),
    "mrp_policy_values_device": (_i, [_P, _P, _i, _P, _P]),
    "mrp_selftest_tanh": (_i, [_i, _P, _P, _i]),
    "mrp_policy_get_params": (_i, [_P, _P, _P]),
    "mrp_ppo_create": (_i, [_P, _i, _PP]),
    "mrp_ppo_destroy": (None, [_P]),
    "mrp_ppo_last_error": (ctypes.c_char_p, [_P]),
    "mrp_ppo_n_params": (_i, [_P]),
    "mrp_ppo_grad_device": (_i, [_P, _P, _i] + [_P] * 5 + [_f, _f, _d, _P, _P]),
    "mrp_ppo_step_device": (_i, [_P, _P, _i] + [_P] * 5 + [_f, _f, _d, _d] + [_f] * 7 + [_P]),
    "mrp_ppo_get_state": (_i, [_P, _P, _P]),
    "mrp_ppo_begin_device": (_i, [_P, _P]),
    "mrp_ppo_minibatch_device": (_i, [_P, _P, _i, _P, ctypes.c_longlong] + [_P] * 6 + [_i, _f, _f, _d, _f, _d, _d] + [_f] * 7
                                 + [_P, _P]),
    "mrp_ppo_progress": (_i, [_P, _P, _ip, _ip]),
    "mrp_ppo_get_staged": (_i, [_P, _i] + [_P] * 6),
    "mrp_ppo_apply_device": (_i, [_P, _P, _i, _P, ctypes.c_longlong, _d, _d] + [_f] * 7 + [_P]),
    "mrp_ppo_set_state": (_i, [_P, _P, _P]),
    "mrp_selftest_exp": (_i, [_i, _P, _P, _i]),
}
EXPORTED = tuple(ABI)

_lib = None


class MrpError(RuntimeError):
    pass


def load(path: str | None = None) -> ctypes.CDLL:
    """Load libmrp.so (raises if it has not been built: there is no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    LIB_PATH_ = path or os.environ.get("MRP_LIB") or LIB_PATH
    if not os.path.exists(LIB_PATH_):
        raise MrpError(f"{LIB_PATH} not built; run `python -m gym_puzzles_amd.build` (hipcc, gfx950)")
    L = ctypes.CDLL(LIB_PATH_)
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def trace_words() -> int:
    """Words per lane of mrp_debug_trace's rows (include/mrp.h MRP_TRACE_WORDS): size trace buffers
    from this, never from a literal, so a tool cannot overrun its buffer when the row grows."""
    return int(load().mrp_debug_trace_words())


def env_dims(env_id: int) -> dict:
    L = load()
    vals = [ctypes.c_int() for _ in range(6)]
    rc = L.mrp_env_dims(env_id, *[ctypes.byref(v) for v in vals])
    if rc != MRP_OK:
        raise ValueError(f"unknown env_id {env_id}")
    keys = ("obs_dim", "act_dim", "n_draws", "n_agents", "n_blocks", "max_episode_steps")
    return dict(zip(keys, (v.value for v in vals)))


def shapes(env_id: int) -> dict:
    """Fixture geometry of an env (host-only; creation order, local vertices)."""
    L = load()
    n = ctypes.c_int32()
    fb, cnt = np.zeros(MAXF, np.int32), np.zeros(MAXF, np.int32)
    v = np.zeros((MAXF, 8, 2), np.float32)
    if L.mrp_shapes(env_id, ctypes.byref(n), _p(fb), _p(cnt), _p(v)) != MRP_OK:
        raise ValueError(f"unknown env_id {env_id}")
    return {"n_fix": n.value, "fix_body": fb[:n.value], "counts": cnt[:n.value], "verts": v[:n.value]}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Batch(Handle):
    """N independent MultiRobotPuzzle worlds on one GPU (one ``mrp_ctx``)."""

    _DESTROY, _LAST_ERROR = "mrp_destroy", "mrp_last_error"

    def __init__(self, env_id: int, n_lanes: int, device: int = 0, seed: int = 0, lane_offset: int = 0):
        self.env_id, self.n_lanes, self.device = env_id, n_lanes, device
        self.__dict__.update(env_dims(env_id))
        self._open("mrp_create", env_id, n_lanes, device, seed, lane_offset)
        self.obs = np.zeros((n_lanes, self.obs_dim), np.float32)
        self.reward = np.zeros(n_lanes, np.float32)
        self.reward64 = np.zeros(n_lanes, np.float64)   # the reference's Python-float rewards
        self.done = np.zeros(n_lanes, np.uint8)
        self.truncated = np.zeros(n_lanes, np.uint8)
        self.status = np.zeros(n_lanes, np.uint8)
        self.terminal_obs = np.zeros((n_lanes, self.obs_dim), np.float32)
        # the output arrays live as long as the batch: their addresses are taken once, so a host step
        # costs one ctypes call (the gym-style single env steps one lane per call)
        self._out = (self.obs.ctypes.data, self.reward.ctypes.data, self.reward64.ctypes.data, self.done.ctypes.data,
                     self.truncated.ctypes.data, self.status.ctypes.data)
        self._term = self.terminal_obs.ctypes.data

    @property
    def handle(self):
        return self._h

    def set_reward_params(self, agentDelta=None, agentDistance=None, blockDelta=None, blockDistance=None,
                          puzzleComp=None, outOfBounds=1000, blkOutOfBounds=100):
        v0 = ENV_VERSION[self.env_id] != 2   # v3 defaults equal v0's (core.py:149-155)
        if puzzleComp is None:
            puzzleComp = 100 if ENV_VERSION[self.env_id] == 3 else 10000
        agentDelta = 10 if agentDelta is None else agentDelta
        agentDistance = (0.1 if v0 else 0.25) if agentDistance is None else agentDistance
        blockDelta = (50 if v0 else 25) if blockDelta is None else blockDelta
        blockDistance = (0.025 if v0 else 0.1) if blockDistance is None else blockDistance
        self._check_rc(load().mrp_set_reward_params(self._h, agentDelta, agentDistance, blockDelta, blockDistance,
                                                 puzzleComp, outOfBounds, blkOutOfBounds))

    def update_params(self, timestep, decay):
        self._check_rc(load().mrp_update_params(self._h, float(timestep), float(decay)))

    def update_goal(self, epoch, nb_epochs):
        self._check_rc(load().mrp_update_goal(self._h, float(epoch), float(nb_epochs)))

    def set_frameskip(self, frameskip: int):
        """world.Step calls per env step (MultiRobotPuzzle2(frameskip=k), multi_robot_puzzle_02.py:476-478)."""
        self._check_rc(load().mrp_set_frameskip(self._h, int(frameskip)))

    def set_auto_reset(self, enabled: bool):
        self._check_rc(load().mrp_set_auto_reset(self._h, 1 if enabled else 0))

    def reset(self, draws=None, actions=None, mask=None) -> np.ndarray:
        d = None if draws is None else np.ascontiguousarray(draws, np.float64).reshape(self.n_lanes, self.n_draws)
        a = None if actions is None else np.ascontiguousarray(actions, np.float32).reshape(self.n_lanes, self.act_dim)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(self.n_lanes)
        self._check_rc(load().mrp_reset(self._h, _p(m), _p(d), _p(a), _p(self.obs)))
        return self.obs

    def step(self, actions=None, want_terminal_obs=False):
        if actions is None:
            ap = None
        else:
            a = np.ascontiguousarray(actions, np.float32)
            if a.size != self.n_lanes * self.act_dim:
                raise ValueError(f"actions: expected {self.n_lanes} x {self.act_dim} values, got shape {a.shape}")
            ap = a.ctypes.data
        self._check_rc(self._L.mrp_step_ex(self._h, ap, *self._out, self._term if want_terminal_obs else None))
        return self.obs, self.reward, self.done, self.truncated

    def step_device(self, d_actions, d_obs, d_reward=None, d_done=None, d_trunc=None, d_status=None, d_term=None,
                    d_reward64=None):
        """Asynchronous step on device pointers (ints, e.g. torch ``tensor.data_ptr()``);
        ``d_reward64`` optionally receives the float64 rewards."""
        self._check_rc(load().mrp_step_device_ex(self._h, d_actions, d_obs, d_reward, d_reward64, d_done, d_trunc, d_status,
                                              d_term))

    def step_n_device(self, n_steps, d_actions, d_obs, d_reward=None, d_done=None, d_trunc=None, d_status=None,
                      d_term=None, d_reward64=None):
        """``n_steps`` consecutive steps in one launch (mrp_step_n_device); every array holds
        ``n_steps`` rows of ``n_lanes`` (step-major), device pointers as in step_device."""
        self._check_rc(load().mrp_step_n_device(self._h, int(n_steps), d_actions, d_obs, d_reward, d_reward64, d_done,
                                             d_trunc, d_status, d_term))

    def set_schedule(self, mode):
        """Lane scheduling (mrp_set_schedule): 0 off, 1 costliest-first dispatch, 2 issue priority
        from the previous step's cost, 3 both (True = 1); results are identical in every mode."""
        self._check_rc(load().mrp_set_schedule(self._h, int(mode)))

    def get_schedule(self) -> int:
        """The lane scheduling mode in force (mrp_get_schedule): mrp_create's per-env default until
        set_schedule is called."""
        return int(load().mrp_get_schedule(self._h))

    def set_seed(self, seed: int):
        """Re-key the device RNG (later resets and synthetic actions); lanes, parameters, stream
        and time limit are kept."""
        self._check_rc(load().mrp_set_seed(self._h, int(seed)))

    def set_time_limit(self, max_episode_steps: int):
        self._check_rc(load().mrp_set_time_limit(self._h, int(max_episode_steps)))

    def set_stream(self, stream_ptr):
        self._check_rc(load().mrp_set_stream(self._h, stream_ptr))

    def synchronize(self):
        self._check_rc(load().mrp_synchronize(self._h))

    def bodies(self) -> np.ndarray:
        out = np.zeros((self.n_lanes, 6 * (self.n_agents + self.n_blocks)), np.float32)
        self._check_rc(load().mrp_get_bodies(self._h, _p(out)))
        return out

    def flags(self) -> np.ndarray:
        out = np.zeros((self.n_lanes, self.n_agents + 1), np.int32)
        self._check_rc(load().mrp_get_flags(self._h, _p(out)))
        return out

    def faults(self) -> np.ndarray:
        """Per-lane loop-guard fault codes (0 = none; include/mrp.h mrp_get_faults)."""
        out = np.zeros(self.n_lanes, np.int32)
        self._check_rc(load().mrp_get_faults(self._h, _p(out)))
        return out

    def counters(self):
        a = np.zeros(1, np.int64)
        b = np.zeros(1, np.int64)
        self._check_rc(load().mrp_counters(self._h, _p(a), _p(b)))
        return int(a[0]), int(b[0])

    def counters_ex(self) -> dict:
        """Per-batch counters since creation (mrp_counters_ex; SURVEY.md 5 metrics)."""
        out = np.zeros(8, np.int64)
        self._check_rc(load().mrp_counters_ex(self._h, _p(out)))
        return {k: int(v) for k, v in zip(COUNTER_NAMES, out)}

    def get_state(self) -> np.ndarray:
        w = load().mrp_state_words(self.env_id)
        out = np.zeros((self.n_lanes, w), np.uint32)
        self._check_rc(load().mrp_get_state(self._h, _p(out)))
        return out

    def get_goals(self) -> np.ndarray:
        """block_final_pos per lane: float64 [n_lanes, n_blocks, 3] (v0 px, v2 scaled units)."""
        out = np.zeros((self.n_lanes, self.n_blocks, 3), np.float64)
        self._check_rc(load().mrp_get_goals(self._h, _p(out)))
        return out

    def render(self, lanes=None, width: int | None = None, height: int | None = None) -> np.ndarray:
        """rgb_array frames of the selected lanes: uint8 [n, height, width, 3] (row 0 = top),
        the reference's render(mode='rgb_array') (multi_robot_puzzle_00.py:528-592)."""
        w0, h0 = (1440, 810) if ENV_VERSION[self.env_id] == 2 else (640, 480)   # v0 and v3: 640 x 480
        width, height = width or w0, height or h0
        sel = np.ascontiguousarray(np.arange(self.n_lanes) if lanes is None else np.atleast_1d(lanes), np.int32)
        out = np.zeros((len(sel), height, width, 3), np.uint8)
        self._check_rc(load().mrp_render(self._h, _p(sel), len(sel), width, height, _p(out)))
        return out

    def render_device(self, d_lanes_ptr: int, n: int, width: int, height: int, d_rgb_ptr: int):
        """Asynchronous render into a device buffer (e.g. a torch uint8 tensor's data_ptr())."""
        self._check_rc(load().mrp_render_device(self._h, ctypes.c_void_p(d_lanes_ptr), n, width, height, ctypes.c_void_p(d_rgb_ptr)))

    def pixels_device(self, width: int, height: int, channels: int, depth: int, d_done_ptr, d_prev_ptr, d_next_ptr: int):
        """Asynchronous frame-stack update of every lane on device pointers (mrp_pixels_device):
        uint8 [n_lanes, depth, height, width, channels] ``next`` from ``prev`` (0 / None: fresh stacks)
        and the lanes' current state; lanes whose ``done`` byte (0 / None: none) is set start afresh."""
        ptr = (lambda a: ctypes.c_void_p(a) if a else None)
        self._check_rc(load().mrp_pixels_device(self._h, int(width), int(height), int(channels), int(depth), ptr(d_done_ptr),
                                             ptr(d_prev_ptr), ptr(d_next_ptr)))

    def pixels(self, width: int, height: int, channels: int = 3, depth: int = 1, done=None, prev=None) -> np.ndarray:
        """Pixel observations of every lane (mrp_pixels): uint8 [n_lanes, depth*height, width, channels],
        ``depth`` frames stacked vertically, oldest first; the newest is the frame of the lane's current
        state (RGB, or the integer luma with channels=1).  ``prev``: the stack this call returned last
        (None: a fresh episode, older frames zero); ``done`` [n_lanes]: lanes that start afresh.
        The numpy restatement of the rule is gym_puzzles_amd.pixels.advance."""
        shape = (self.n_lanes, int(depth) * int(height), int(width), int(channels))
        d = None if done is None else np.ascontiguousarray(done, np.uint8).reshape(self.n_lanes)
        if prev is not None:
            if prev.shape != shape or prev.dtype != np.uint8:
                raise ValueError(f"prev: expected uint8 {shape}, got {prev.dtype} {prev.shape}")
            prev = np.ascontiguousarray(prev)
        # sizes the library refuses (MrpError below) never reach the kernel: any buffer will do for them
        out = np.zeros(shape if min(shape) > 0 and depth <= 16 else (1,), np.uint8)
        self._check_rc(load().mrp_pixels(self._h, int(width), int(height), int(channels), int(depth), _p(d), _p(prev), _p(out)))
        return out

    def set_state(self, state: np.ndarray):
        s = np.ascontiguousarray(state, np.uint32)
        self._check_rc(load().mrp_set_state(self._h, _p(s)))


def selftest_sincos(x: np.ndarray, device: int = 0):
    """Evaluate the device sinf/cosf (glibc-faithful restatement) on ``x``."""
    x = np.ascontiguousarray(x, np.float32)
    s = np.zeros_like(x)
    c = np.zeros_like(x)
    rc = load().mrp_selftest_sincos(device, _p(x), _p(s), _p(c), x.size)
    if rc != MRP_OK:
        raise MrpError(f"mrp_selftest_sincos failed ({rc})")
    return s, c
