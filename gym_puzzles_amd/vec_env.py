"""SB3-style vectorised env over one device batch (reference callers
``train/train.py:63-82`` build ``DummyVecEnv([make_env] * n_envs)`` + ``VecNormalize``).

``MultiRobotPuzzleVecEnv(env_id, num_envs)`` exposes the stable-baselines3 ``VecEnv``
interface (reset / step_async / step_wait / step / close / seed / get_attr / set_attr /
env_method / env_is_wrapped) with SB3's auto-reset semantics: a finished lane is reset inside
the same ``mrp_step`` call on the GPU, ``obs`` holds its new first observation and
``infos[i]["terminal_observation"]`` the last one; ``infos[i]["TimeLimit.truncated"]`` marks
TimeLimit ends.  Spawns and reset actions then come from the device counter RNG (keyed by
seed and global lane), not from ``np.random``.

``step_torch`` is the zero-copy variant for a policy that lives on the same GPU: actions and
outputs are torch CUDA tensors and nothing crosses PCIe.

``obs_type="image"`` selects the reference's pixel observations (multi_robot_puzzle_00.py:148-162):
``reset()`` / ``step_wait()`` return uint8 frame stacks ``[N, obs_depth*H, W, C]`` that one kernel
launch renders from the resident lane state (``mrp_pixels_device``; the rule is
``gym_puzzles_amd.pixels.advance``), and ``pixels_torch`` is their zero-copy form.  A finished lane's
stack starts afresh from its new episode's first frame.  **``terminal_observation`` is not provided
for image observations**: the lane is reset inside the step that ends its episode, so its terminal
state no longer exists when the frame is drawn; ``TimeLimit.truncated`` and the failure flags are
reported as for ``"low-dim"``.

When stable-baselines3 is importable the class derives from its ``VecEnv`` and the spaces are
``gym.spaces.Box`` (what SB3's wrappers check with ``isinstance``); neither package is in this
image, so that path is untested here (parity unpinned) and ``MultiRobotPuzzleVecNormalize`` is
the tested way to get VecNormalize + Monitor.
"""
from __future__ import annotations

import numpy as np

from ._device import Handle, check_tensor, check_tensors, ptr, stream_of
from .dist import agree, broadcast_array
from ._native import ENV_IDS, STATUS_FAULT, STATUS_NONFINITE, Batch, env_dims
from .spawn import ENV_CFG, V2_AGENT_IDS, V3_AGENT_IDS
from .pixels import stack_shape
from .seeding import make_box

try:   # SB3 1.x/2.x: VecEnv(num_envs, observation_space, action_space)
    from stable_baselines3.common.vec_env.base_vec_env import VecEnv as _VecEnvBase
except ImportError:
    _VecEnvBase = object

_ID = dict(ENV_IDS)


def _lane_flags(batch: Batch, status: np.ndarray, infos: list) -> None:
    """Per-lane failure report (SURVEY.md 8b Errors): ``info['nan']`` for a lane whose step
    produced a NaN / inf, ``info['mrp_fault']`` = the loop-guard code of a lane whose guard has
    tripped (include/mrp.h status flag bits).  Never raises; healthy lanes get no extra keys."""
    nan = np.nonzero(status & STATUS_NONFINITE)[0]
    for i in nan:
        infos[i]["nan"] = True
    bad = np.nonzero(status & STATUS_FAULT)[0]
    if bad.size:
        codes = batch.faults()
        for i in bad:
            infos[i]["mrp_fault"] = int(codes[i])


class MultiRobotPuzzleVecEnv(_VecEnvBase):
    def __init__(self, env_id, num_envs: int, device: int = 0, seed: int = 0, lane_offset: int = 0,
                 max_episode_steps: int | None = None, frameskip: int = 1, num_agents: int | None = None,
                 obs_type: str = "low-dim", image_size=(84, 84), obs_depth: int = 3, grayscale: bool = True):
        self.env_index = _ID[env_id] if isinstance(env_id, str) else int(env_id)
        if num_agents is not None and num_agents != env_dims(self.env_index)["n_agents"]:
            # MultiRobotPuzzle2 / Heavy2(num_agents=N) (multi_robot_puzzle_02.py:139): the env id of that count
            cfg = ENV_CFG[self.env_index]
            key = (cfg[3], int(num_agents))
            ids = V2_AGENT_IDS if cfg[0] == 2 and cfg[2] == 1 else (V3_AGENT_IDS if cfg[0] == 3 else {})
            if key not in ids:
                raise NotImplementedError(f"num_agents={num_agents} is not instantiated for env {env_id!r}")
            self.env_index = ids[key]
        d = env_dims(self.env_index)
        self.num_envs = num_envs
        self.device = device
        self._seed = seed
        self._lane_offset = lane_offset
        # MultiRobotPuzzle2(frameskip=k) (multi_robot_puzzle_02.py:139,476-478): world.Step calls per env
        # step.  Only the v2 classes take it: v0 fixes frameskip 1 for its low-dim observations
        # (multi_robot_puzzle_00.py:161-162) and RobotPuzzleBase has none (core.py:77-418)
        self.frameskip = int(frameskip)
        if self.frameskip < 1:
            raise ValueError("frameskip must be >= 1")
        if obs_type not in ("low-dim", "image"):
            raise ValueError(f"obs_type={obs_type!r}: 'low-dim' or 'image' (multi_robot_puzzle_00.py:148)")
        self.obs_type = obs_type
        # image observations repeat world.Step in every env version (multi_robot_puzzle_00.py:161)
        if self.frameskip != 1 and ENV_CFG[self.env_index][0] != 2 and obs_type != "image":
            raise ValueError(f"frameskip={frameskip}: only the MultiRobotPuzzle2 envs (v2) repeat world.Step per env step")
        if obs_type == "image":
            # (width, height) of a frame, frames per stack, luma (1 channel) or RGB (3)
            self.image_size = (int(image_size[0]), int(image_size[1]))
            self.obs_depth, self.channels = int(obs_depth), 1 if grayscale else 3
            if min(self.image_size) < 1 or not 1 <= self.obs_depth <= 16:
                raise ValueError(f"image_size={image_size}, obs_depth={obs_depth}: sizes >= 1, depth 1..16")
            self.observation_space = make_box(0, 255, shape=stack_shape(*self.image_size, self.channels, self.obs_depth),
                                              dtype=np.uint8)
        else:
            self.observation_space = make_box(-np.inf, np.inf, shape=(d["obs_dim"],), dtype=np.float32)
        self.action_space = make_box(-1.0, 1.0, shape=(d["act_dim"],), dtype=np.float32)
        self.max_episode_steps = d["max_episode_steps"] if max_episode_steps is None else max_episode_steps
        # everything get_attr / step need exists before SB3's base __init__ runs (SB3 2.x queries
        # get_attr("render_mode") from it)
        self._attrs = {"render_mode": None}
        self._actions = None
        self._b = None
        self._make_batch()
        if _VecEnvBase is not object:
            _VecEnvBase.__init__(self, num_envs, self.observation_space, self.action_space)

    def _make_batch(self):
        if self._b is not None:
            self._b.close()
        self._b = Batch(self.env_index, self.num_envs, device=self.device, seed=self._seed,
                        lane_offset=self._lane_offset)
        self._b.set_time_limit(self.max_episode_steps)
        self._b.set_auto_reset(True)
        if self.frameskip != 1:
            self._b.set_frameskip(self.frameskip)
        self._stack = None          # image observations: the device tensor that holds the current stacks
        self._pair = None           # ... and this env's own ping-pong pair of them

    # -- VecEnv API ------------------------------------------------------------------------
    def reset(self) -> np.ndarray:
        obs = self._b.reset()
        if self.obs_type == "image":
            self._stack = None      # every lane starts afresh
            return self.pixels_torch().cpu().numpy()
        return obs.copy()

    def step_async(self, actions) -> None:
        self._actions = np.ascontiguousarray(actions, dtype=np.float32).reshape(self.num_envs, -1)

    def step_wait(self):
        if self.obs_type == "image":
            import torch
            _, rew, done, trunc = self._b.step(self._actions)
            d_done = torch.from_numpy(done).to(torch.device("cuda", self.device))
            obs = self.pixels_torch(d_done).cpu().numpy()   # the one copy of the stacks to the host
            infos = [{} for _ in range(self.num_envs)]
            for i in np.nonzero(done)[0]:
                infos[i]["TimeLimit.truncated"] = bool(trunc[i])
            _lane_flags(self._b, self._b.status, infos)
            return obs, rew.copy(), done.astype(bool), infos
        obs, rew, done, trunc = self._b.step(self._actions, want_terminal_obs=True)
        infos = [{} for _ in range(self.num_envs)]
        for i in np.nonzero(done)[0]:
            infos[i]["terminal_observation"] = self._b.terminal_obs[i].copy()
            infos[i]["TimeLimit.truncated"] = bool(trunc[i])
        _lane_flags(self._b, self._b.status, infos)
        return obs.copy(), rew.copy(), done.astype(bool), infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self) -> None:
        if self._b is not None:
            self._b.close()
            self._b = None

    def seed(self, seed=None):
        """Re-key the device RNG (takes effect from the next reset, as SB3's VecEnv.seed does);
        lane state, tuning parameters, stream and time limit are kept.  Returns one seed per env."""
        self._seed = 0 if seed is None else int(seed)
        self._b.set_seed(self._seed)
        return [self._seed + i for i in range(self.num_envs)]

    def get_attr(self, attr_name, indices=None):
        idx = self._indices(indices)
        if attr_name in ("observation_space", "action_space", "max_episode_steps"):
            return [getattr(self, attr_name)] * len(idx)
        if attr_name not in self._attrs:
            raise AttributeError(attr_name)
        return [self._attrs[attr_name]] * len(idx)

    def set_attr(self, attr_name, value, indices=None):
        self._attrs[attr_name] = value

    def env_method(self, method_name, *args, indices=None, **kwargs):
        """Tuning hooks apply to every lane of the batch (one parameter block per ctx)."""
        if method_name not in ("set_reward_params", "update_params", "update_goal"):
            raise AttributeError(method_name)
        getattr(self._b, method_name)(*args, **kwargs)
        return [None] * len(self._indices(indices))

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * len(self._indices(indices))

    def get_images(self):
        """One rgb_array frame per env (SB3 VecEnv.get_images; frames from mrp_render)."""
        return list(self._b.render())

    def _indices(self, indices):
        if indices is None:
            return list(range(self.num_envs))
        if isinstance(indices, int):
            return [indices]
        return list(indices)

    # -- zero-copy device path -----------------------------------------------------------------
    def step_torch(self, actions, obs, reward, done, truncated=None, terminal_obs=None, reward64=None, status=None):
        """One step on torch CUDA tensors on this env's device (float32 [N, A] actions, [N, O] obs,
        [N] reward, uint8 [N] done/truncated/status, optional [N, O] terminal_obs and float64 [N]
        reward64), asynchronous on that device's current torch stream.  ``actions`` may be None (the
        device RNG's synthetic actions); a tensor of another dtype, shape or device, or one that is not
        contiguous, raises ``ValueError`` before anything is launched."""
        import torch
        dev = torch.device("cuda", self.device)
        N, O, A = self.num_envs, self._b.obs_dim, self._b.act_dim
        f32, u8 = torch.float32, torch.uint8
        check_tensors("step_torch", dev, (
            ("actions", actions, f32, (N, A), True), ("obs", obs, f32, (N, O), False), ("reward", reward, f32, (N,), False),
            ("done", done, u8, (N,), False), ("truncated", truncated, u8, (N,), True), ("status", status, u8, (N,), True),
            ("terminal_obs", terminal_obs, f32, (N, O), True), ("reward64", reward64, torch.float64, (N,), True)))
        self._b.set_stream(stream_of(dev))
        self._b.step_device(ptr(actions), ptr(obs), ptr(reward), ptr(done), ptr(truncated), ptr(status), ptr(terminal_obs),
                            ptr(reward64))

    def pixels_torch(self, done=None, out=None):
        """The zero-copy companion of ``step_torch`` for ``obs_type="image"``: renders every lane's
        current state and advances the frame stacks in one launch on this device's current torch
        stream.  ``done``: the uint8 [N] CUDA tensor ``step_torch`` filled (None: no lane ended);
        lanes it marks start afresh, and so does every lane in the first call after ``reset()``.
        Returns the new stacks, a uint8 CUDA tensor [N, obs_depth*H, W, C]: ``out`` when given
        (it must not be the tensor that holds the previous stacks when obs_depth > 1), else one of
        the env's own two buffers, which the call after next overwrites."""
        if self.obs_type != "image":
            raise ValueError('pixels_torch: this VecEnv was built with obs_type="low-dim"')
        import torch
        dev = torch.device("cuda", self.device)
        shape = (self.num_envs,) + tuple(self.observation_space.shape)
        u8 = torch.uint8
        check_tensors("pixels_torch", dev, (("done", done, u8, (self.num_envs,), True), ("out", out, u8, shape, True)))
        if out is None:
            if self._pair is None:
                self._pair = [torch.zeros(shape, dtype=torch.uint8, device=dev) for _ in range(2)]
            out = self._pair[1] if self._stack is self._pair[0] else self._pair[0]
        self._b.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        (w, h), prev = self.image_size, self._stack
        self._b.pixels_device(w, h, self.channels, self.obs_depth, 0 if done is None else done.data_ptr(),
                              0 if prev is None else prev.data_ptr(), out.data_ptr())
        self._stack = out
        return out

    @property
    def batch(self) -> Batch:
        return self._b


# ---- data-parallel VecNormalize: the rule (numpy float64, every operation rounded on its own, no FMA) ------
# One set of obs / return statistics over the R * L lanes of R ranks, each with L lanes.  A rank takes the
# moments of its own lanes (moments_local_ref), the ranks' parts are gathered in rank order, and every rank folds
# them in that order (moments_combine_ref) and merges the result (rms_merge_ref), so the statistics are the same
# bits on every rank.  csrc/mrp_norm.hip (k_moments<true>, k_norm_merge) computes the fold and the merge with
# these operations in this order; its column sums are a 256-thread tree where numpy adds row after row, so the
# statistics are held to the bound of tests/vecnorm_exact.py, as the unsharded ones are.

def moments_local_ref(x) -> np.ndarray:
    """One rank's part of the statistic columns ``x`` ``[L]`` or ``[L, C]``: float64 ``[2 C]`` with
    ``part[2c]`` the column's mean over the L lanes and ``part[2c + 1]`` its ``M2 = sum((x - mean)^2)`` (two
    float64 passes, M2 not divided by L)."""
    x = np.asarray(x, np.float64)
    x = x.reshape(x.shape[0], -1)
    bm = x.sum(axis=0) / x.shape[0]
    part = np.empty(2 * x.shape[1], np.float64)
    part[0::2], part[1::2] = bm, ((x - bm) ** 2).sum(axis=0)
    return part


def moments_combine_ref(parts, L: int):
    """Fold the ranks' parts ``[R, >= 2 C]`` (row r from rank r, every rank with ``L`` lanes) in ascending rank
    order: returns ``(bm [C], bv [C], n)``, the batch moments over all ``n = R * L`` lanes.  Chan et al.'s
    pairwise update, left-associated as written; with one row ``bv`` is ``M2 / L``."""
    parts = np.asarray(parts, np.float64)
    ma, Ma, na = parts[0, 0::2].copy(), parts[0, 1::2].copy(), float(L)
    for r in range(1, parts.shape[0]):
        mb, Mb, nb = parts[r, 0::2], parts[r, 1::2], float(L)
        nt = na + nb
        d = mb - ma
        Ma = Ma + Mb + d * d * na * nb / nt
        ma = ma + d * nb / nt
        na = nt
    return ma, Ma / na, na


def rms_merge_ref(mean, var, count, bm, bv, n):
    """SB3 ``RunningMeanStd.update_from_moments`` (``rms_merge`` in csrc/mrp_norm.hip): ``(mean, var, count)``
    after the batch moments ``(bm, bv)`` over ``n`` values."""
    delta = bm - mean
    tot = count + n
    new_mean = mean + delta * n / tot
    m2 = var * count + bv * n + delta * delta * count * n / tot
    return new_mean, m2 / tot, tot


class DeviceVecNormalize(Handle):
    """stable-baselines3 ``VecNormalize`` + ``Monitor`` statistics kept on the GPU (libmrp's
    ``mrp_norm_*``).  The reference wraps every env in ``Monitor`` and the vector
    env in ``VecNormalize`` with default arguments (``train/train.py:68,80-82``).  All arrays are
    contiguous torch CUDA tensors on ``device``, float32 unless stated; ``reset`` and ``step`` raise
    ``ValueError`` for any other tensor before anything is launched.  The kernels are element-wise, so
    an output may be its input (``obs_out is obs``, ``reward_out is reward``, ``term_out is term_obs``).  Calls
    are asynchronous on the current torch stream.

    Contract (tests/vecnorm_exact.py, tests/test_norm_gpu.py): the statistics are within a bound derived
    from the inputs of the exact batch moments and merge; a float32 output is within half a float32 ulp of
    the exact value plus what that bound propagates, and exactly ``float32(+-clip)`` where saturated; counts
    and Monitor's returns and lengths are bit-exact; ``term_out``, ``ep_return`` and ``ep_len`` are written
    for done lanes only; NaN propagates as in numpy (a NaN observation makes its column's statistics and
    outputs NaN from then on, ``+-inf`` saturates).

    Data-parallel (``moments_local_ref`` / ``moments_combine_ref`` / ``rms_merge_ref`` above): with ``shard`` (a
    ``dist.Shard`` whose ``lanes_per_rank`` is ``n_lanes``) or an explicit ``exchange`` (a float64
    ``dist.GradExchange`` of at least ``part_len`` values) the statistics are one set over the
    ``shard.world * n_lanes`` lanes of all ranks, updated as SB3 updates one ``VecNormalize`` over that many envs
    and bit-identical on every rank; a NaN on any rank poisons its column on every rank.  A ``reset`` / ``step``
    that moves statistics is then the local phase (``mrp_norm_local_device`` into ``exchange.mine``), the
    exchange, and the apply phase (``mrp_norm_apply_device``), all on the current torch stream; with
    ``training`` off nothing is exchanged.  The discounted returns and Monitor stay per lane.  ``group``,
    ``host_stage`` and ``force_collective`` are ``GradExchange``'s, for the exchange built from ``shard``.  Every
    rank must hold the same ``(n_lanes, obs_dim, training, norm_obs)``: the first call after construction or after
    a change of the two flags compares them across ranks (one ``dist.agree``) and raises ``ValueError`` on
    every rank on a mismatch, before anything is enqueued.  Use ``sync_from`` after ``set_stats`` on one rank."""

    _DESTROY, _LAST_ERROR = "mrp_norm_destroy", "mrp_norm_last_error"

    def __init__(self, n_lanes: int, obs_dim: int, device: int = 0, clip_obs: float = 10.0, clip_reward: float = 10.0,
                 gamma: float = 0.99, epsilon: float = 1e-8, shard=None, exchange=None, group=None, host_stage: bool = False,
                 force_collective: bool = False):
        import torch
        self.n_lanes, self.obs_dim, self.device = n_lanes, obs_dim, device
        self._dev = torch.device("cuda", device)
        if shard is None and exchange is not None:
            shard = exchange.shard
        if shard is not None and shard.lanes_per_rank != n_lanes:
            raise ValueError(f"DeviceVecNormalize: shard.lanes_per_rank is {shard.lanes_per_rank}, n_lanes is {n_lanes}")
        self._open("mrp_norm_create", n_lanes, obs_dim, device, clip_obs, clip_reward, gamma, epsilon)
        self._training = True
        self._norm_obs = True
        self.shard, self.part_len, self._checked = shard, int(self._L.mrp_norm_part_len(obs_dim)), None
        if shard is not None and exchange is None:
            from .dist import GradExchange
            exchange = GradExchange(shard, self.part_len, self._dev, group=group, host_stage=host_stage,
                                    force_collective=force_collective, dtype=torch.float64)
        if exchange is not None:
            if exchange.dtype != torch.float64 or exchange.n_floats < self.part_len or exchange.world != shard.world:
                raise ValueError(f"DeviceVecNormalize: the exchange holds {exchange.n_floats} {exchange.dtype} values for "
                                 f"{exchange.world} ranks, expected at least {self.part_len} torch.float64 for {shard.world}")
            check_tensor("DeviceVecNormalize", "exchange.mine", exchange.mine, self._dev, torch.float64, (exchange.part_stride,))
        self.exchange = exchange

    def _launch(self, who, tensors, step, obs, reward, *rest):
        """Check every tensor of ``tensors`` (``check_tensors``' specs), then launch on the current torch stream:
        with an exchange and statistics to move the local phase, the exchange and the apply phase, else the
        plain entry (no collective).  ``rest`` are ``mrp_norm_apply_device``'s arguments after ``d_reward``."""
        check_tensors(who, self._dev, tensors)
        L, ex = self._L, self.exchange
        if ex is not None:
            self._check_ranks(who)
        self._check_rc(L.mrp_norm_set_stream(self._h, stream_of(self._dev)))
        if ex is not None and self._training and (self._norm_obs or step):
            self._check_rc(L.mrp_norm_local_device(self._h, obs, reward, step, ex.mine.data_ptr()))
            parts = ex()
            self._check_rc(L.mrp_norm_apply_device(self._h, int(parts.shape[0]), parts.data_ptr(), int(parts.shape[1]), step, obs,
                                                   reward, *rest))
        elif step:
            self._check_rc(L.mrp_norm_step_device_ex(self._h, obs, reward, *rest))
        else:
            self._check_rc(L.mrp_norm_reset_device(self._h, obs, rest[3]))

    def _check_ranks(self, who):
        """The ranks must take the same branch, or the collective hangs: ``dist.agree`` on ``(n_lanes, obs_dim,
        training, norm_obs)``, repeated only when the tuple changes."""
        mine = (int(self.n_lanes), int(self.obs_dim), self._training, self._norm_obs)
        if mine != self._checked:
            agree(who, "(n_lanes, obs_dim, training, norm_obs)", mine, self.exchange.world, self.exchange.group)
            self._checked = mine

    def sync_from(self, src=0, group=None):
        """Broadcast rank ``src``'s statistics and load them on every rank (after ``set_stats`` / a load on
        one rank, or on resume; synchronises).  The vector travels on the device under an nccl group and on
        the host otherwise; ``group`` defaults to the exchange's."""
        if group is None and self.exchange is not None:
            group = self.exchange.group
        st = np.zeros(2 * self.obs_dim + 4, np.float64)
        self._check_rc(self._L.mrp_norm_get_stats(self._h, st.ctypes.data))
        st = broadcast_array(st, src, group, self._dev)
        self._check_rc(self._L.mrp_norm_set_stats(self._h, st.ctypes.data))

    @property
    def training(self) -> bool:
        return self._training

    @training.setter
    def training(self, value: bool):
        self._training = bool(value)
        self._check_rc(self._L.mrp_norm_set_training(self._h, int(self._training)))

    @property
    def norm_obs(self) -> bool:
        return self._norm_obs

    @norm_obs.setter
    def norm_obs(self, value: bool):
        """SB3 VecNormalize.norm_obs: the observation statistics only move while it is set."""
        self._norm_obs = bool(value)
        self._check_rc(self._L.mrp_norm_set_norm_obs(self._h, int(self._norm_obs)))

    def reset(self, obs, obs_out):
        """``obs`` and ``obs_out``: float32 [N, O]."""
        import torch
        shape = (self.n_lanes, self.obs_dim)
        tensors = (("obs", obs, torch.float32, shape, False), ("obs_out", obs_out, torch.float32, shape, False))
        self._launch("DeviceVecNormalize.reset", tensors, 0, ptr(obs), None, None, None, None, ptr(obs_out), None, None, None, None)

    def step(self, obs, reward, done, obs_out, reward_out, term_obs=None, term_out=None, ep_return=None, ep_len=None,
             reward64=None):
        """float32 [N, O] ``obs`` / ``obs_out`` / ``term_obs`` / ``term_out``, float32 [N] ``reward`` /
        ``reward_out``, uint8 [N] ``done``, float64 [N] ``ep_return`` and int32 [N] ``ep_len``.
        ``reward64`` (float64 [N], optional): the env's float64 rewards, which Monitor's
        episode return then sums (SB3's Monitor sums the env's Python-float rewards)."""
        import torch
        N, NO, f32, f64 = (self.n_lanes,), (self.n_lanes, self.obs_dim), torch.float32, torch.float64
        tensors = (("obs", obs, f32, NO, False), ("reward", reward, f32, N, False), ("done", done, torch.uint8, N, False),
                   ("obs_out", obs_out, f32, NO, False), ("reward_out", reward_out, f32, N, False),
                   ("term_obs", term_obs, f32, NO, True), ("term_out", term_out, f32, NO, True),
                   ("ep_return", ep_return, f64, N, True), ("ep_len", ep_len, torch.int32, N, True),
                   ("reward64", reward64, f64, N, True))
        self._launch("DeviceVecNormalize.step", tensors, 1, ptr(obs), ptr(reward), ptr(reward64), ptr(done), ptr(term_obs),
                     ptr(obs_out), ptr(reward_out), ptr(term_out), ptr(ep_return), ptr(ep_len))

    def get_stats(self) -> dict:
        st = np.zeros(2 * self.obs_dim + 4, np.float64)
        self._check_rc(self._L.mrp_norm_get_stats(self._h, st.ctypes.data))
        D = self.obs_dim
        return {"obs_mean": st[:D], "obs_var": st[D:2 * D], "obs_count": st[2 * D], "ret_mean": st[2 * D + 1],
                "ret_var": st[2 * D + 2], "ret_count": st[2 * D + 3]}

    def set_stats(self, stats: dict) -> None:
        st = np.concatenate([np.asarray(stats["obs_mean"], np.float64), np.asarray(stats["obs_var"], np.float64),
                             [stats["obs_count"], stats["ret_mean"], stats["ret_var"], stats["ret_count"]]])
        self._check_rc(self._L.mrp_norm_set_stats(self._h, np.ascontiguousarray(st).ctypes.data))


class MultiRobotPuzzleVecNormalize:
    """``VecNormalize(MultiRobotPuzzleVecEnv)`` with ``Monitor`` episode records, computed on the
    device.  Same VecEnv surface as SB3's wrapper: ``reset()`` / ``step(actions)`` return host
    numpy arrays (normalised obs and reward), ``infos[i]`` carry ``terminal_observation``
    (normalised), ``TimeLimit.truncated`` and Monitor's ``episode`` = {"r", "l"} for finished
    lanes; ``get_original_obs()`` / ``get_original_reward()`` give the raw values."""

    def __init__(self, venv: MultiRobotPuzzleVecEnv, training: bool = True, norm_obs: bool = True, norm_reward: bool = True,
                 clip_obs: float = 10.0, clip_reward: float = 10.0, gamma: float = 0.99, epsilon: float = 1e-8, shard=None,
                 exchange=None):
        """``shard`` / ``exchange``: ``DeviceVecNormalize``'s (data-parallel: one set of statistics over the lanes
        of all ranks, so any rank's ``save()`` writes the one global file)."""
        import torch
        if getattr(venv, "obs_type", "low-dim") != "low-dim":
            raise ValueError("VecNormalize keeps running statistics of low-dim observations; image stacks are used as they are")
        self.venv = venv
        # SB3 semantics: the flags choose what step()/reset() return; while `training` is set the
        # returns' statistics are updated, and the observation statistics only when norm_obs is set
        self.norm_reward = bool(norm_reward)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.num_envs, self.observation_space, self.action_space = venv.num_envs, venv.observation_space, venv.action_space
        N, O = venv.num_envs, venv.observation_space.shape[0]
        dev = torch.device("cuda", venv.device)
        self.norm = DeviceVecNormalize(N, O, venv.device, clip_obs, clip_reward, gamma, epsilon, shard=shard, exchange=exchange)
        self.norm.training = training
        self.norm.norm_obs = norm_obs
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
        self._act, self._obs, self._rew = z(N, venv.action_space.shape[0]), z(N, O), z(N)
        self._done, self._trunc, self._term = z(N, dt=torch.uint8), z(N, dt=torch.uint8), z(N, O)
        self._nobs, self._nrew, self._nterm = z(N, O), z(N), z(N, O)
        self._epr, self._epl = z(N, dt=torch.float64), z(N, dt=torch.int32)
        self._rew64 = z(N, dt=torch.float64)
        self._status = z(N, dt=torch.uint8)

    @property
    def training(self):
        return self.norm.training

    @training.setter
    def training(self, v):
        self.norm.training = v

    @property
    def norm_obs(self):
        return self.norm.norm_obs

    @norm_obs.setter
    def norm_obs(self, v):
        self.norm.norm_obs = v

    def reset(self):
        import torch
        self._obs.copy_(torch.from_numpy(self.venv.reset()))
        self.norm.reset(self._obs, self._nobs)
        return (self._nobs if self.norm_obs else self._obs).cpu().numpy()

    def step(self, actions):
        import torch
        self._act.copy_(torch.as_tensor(np.asarray(actions, np.float32).reshape(self.num_envs, -1)))
        self.venv.step_torch(self._act, self._obs, self._rew, self._done, self._trunc, self._term, self._rew64, self._status)
        self.norm.step(self._obs, self._rew, self._done, self._nobs, self._nrew, self._term, self._nterm, self._epr, self._epl,
                       self._rew64)
        obs = (self._nobs if self.norm_obs else self._obs).cpu().numpy()
        rew = (self._nrew if self.norm_reward else self._rew).cpu().numpy()
        done, trunc = self._done.cpu().numpy().astype(bool), self._trunc.cpu().numpy().astype(bool)
        infos = [{} for _ in range(self.num_envs)]
        idx = np.nonzero(done)[0]
        if idx.size:
            term = (self._nterm if self.norm_obs else self._term).cpu().numpy()
            epr, epl = self._epr.cpu().numpy(), self._epl.cpu().numpy()
            for i in idx:
                infos[i]["terminal_observation"] = term[i].copy()
                infos[i]["TimeLimit.truncated"] = bool(trunc[i])
                infos[i]["episode"] = {"r": round(float(epr[i]), 6), "l": int(epl[i])}
        _lane_flags(self.venv.batch, self._status.cpu().numpy(), infos)
        return obs, rew, done, infos

    def get_original_obs(self):
        return self._obs.cpu().numpy()

    # ---- persistence (SB3's VecNormalize.save / VecNormalize.load, train/test.py:66) --------
    # SB3 pickles the wrapper; this build stores the same statistics and settings in an .npz
    # (nothing in the file is executed on load).
    def save(self, save_path: str) -> None:
        """Writes exactly `save_path` (train.py:149 saves to 'models/<run>/saved_env.pkl' and
        test.py:66 loads that same path back; np.savez on a bare path would append '.npz')."""
        st = self.norm.get_stats()
        with open(save_path, "wb") as f:
            np.savez(f, **st, clip_obs=self.clip_obs, clip_reward=self.clip_reward, gamma=self.gamma,
                     epsilon=self.epsilon, training=self.training, norm_obs=self.norm_obs, norm_reward=self.norm_reward)

    @classmethod
    def load(cls, load_path: str, venv: MultiRobotPuzzleVecEnv, shard=None, exchange=None) -> "MultiRobotPuzzleVecNormalize":
        with np.load(load_path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
        self = cls(venv, training=bool(d["training"]), norm_obs=bool(d["norm_obs"]), norm_reward=bool(d["norm_reward"]),
                   clip_obs=float(d["clip_obs"]), clip_reward=float(d["clip_reward"]), gamma=float(d["gamma"]),
                   epsilon=float(d["epsilon"]), shard=shard, exchange=exchange)
        self.norm.set_stats({k: d[k] for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")})
        return self

    def get_stats(self) -> dict:
        return self.norm.get_stats()

    def get_original_reward(self):
        return self._rew.cpu().numpy()

    def get_images(self):   # VecEnvWrapper passes rendering through (VecVideoRecorder, test.py:61-63)
        return self.venv.get_images()

    def env_method(self, method_name, *args, indices=None, **kwargs):
        return self.venv.env_method(method_name, *args, indices=indices, **kwargs)

    def get_attr(self, attr_name, indices=None):
        return self.venv.get_attr(attr_name, indices)

    def close(self):
        self.norm.close()
        self.venv.close()
