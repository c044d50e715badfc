"""Device rollout buffer: SB3's ``RolloutBuffer`` kept in HBM, with the TimeLimit bootstrap and GAE
in one kernel launch (``mrp_gae_device``, ``k_gae`` in ``csrc/mrp_norm.hip``).

stable-baselines3's ``OnPolicyAlgorithm.collect_rollouts`` stores each transition, adds
``gamma * V(terminal_observation)`` to the reward of every lane whose episode ended by
``TimeLimit.truncated``, and after ``n_steps`` ``RolloutBuffer.compute_returns_and_advantage`` runs
the GAE recurrence backwards.  The lanes of this project run in lockstep, so whole batches truncate
on the same step: the bootstrap is the usual way an episode ends here.

``gae_ref`` is the numpy restatement of that rule and the definition ``k_gae`` matches bit for bit,
numpy's dtype promotion (NEP 50, Python scalars weak) included.  stable-baselines3 is not installed
where this was written, so parity with SB3 itself is unpinned: the rule is this restatement.

This module is pure numpy at import; ``gae_device`` and ``DeviceRolloutBuffer`` import torch when used.
"""
from __future__ import annotations

import numpy as np

from ._device import check_tensor, check_tensors, index_of, ptr, stream_of


def gae_ref(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda, truncated=None, terminal_values=None):
    """SB3 RolloutBuffer.compute_returns_and_advantage, line by line, preceded by
    collect_rollouts' `rewards[idx] += gamma * terminal_value` for truncated lanes.
    rewards/values/terminal_values float32 [T, N]; episode_starts float32 [T, N] (0/1);
    truncated uint8/bool [T, N]; last_values float32 [N]; dones bool [N] (cast with astype(bool));
    gamma, gae_lambda Python floats.  Returns (advantages, returns), float32 [T, N].

    ``episode_starts[s]`` is the ``done`` of the step before row ``s`` (1 in the first row after
    ``reset()``, SB3's ``_last_episode_starts``).  Parity with SB3 itself is unpinned (see the module
    docstring).  The promotion that the kernel reproduces: ``delta`` and ``gamma * gae_lambda * nnt`` are
    float32 below the last row; on the last row ``nnt`` is float64 (``1.0 - bool_array``), so
    ``gamma * nv`` rounds to float32 and the rest of that ``delta`` is float64; ``last`` is float64
    from the first iteration on and ``adv[s]`` rounds it to float32 once."""
    rewards = rewards.copy()
    values, episode_starts = np.asarray(values), np.asarray(episode_starts)
    dones = np.asarray(dones).astype(bool)
    T = rewards.shape[0]
    if truncated is not None:
        m = np.asarray(truncated).astype(bool)
        rewards[m] = rewards[m] + (np.float32(gamma) * terminal_values[m])      # float32 throughout
    adv = np.zeros_like(rewards)
    last = 0
    for s in reversed(range(T)):
        if s == T - 1:
            nnt = 1.0 - dones                    # bool -> float64 here, as in SB3
            nv = last_values
        else:
            nnt = 1.0 - episode_starts[s + 1]    # float32
            nv = values[s + 1]
        delta = rewards[s] + gamma * nv * nnt - values[s]
        last = delta + gamma * gae_lambda * nnt * last
        adv[s] = last
    return adv, adv + values


def gae_device(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda, truncated=None, terminal_values=None,
               advantages=None, returns=None):
    """``gae_ref`` on the device in one launch (``mrp_gae_device``), bit for bit.  Contiguous CUDA
    tensors on one device: float32 [T, N] rewards / values / terminal_values, uint8 [T, N]
    episode_starts / truncated, float32 [N] last_values, uint8 [N] dones; ``truncated`` and
    ``terminal_values`` come together or not at all.  ``advantages`` / ``returns`` (float32 [T, N],
    allocated when omitted) may overlap no input and not each other.  Asynchronous on the current torch
    stream of the tensors' device.  Returns ``(advantages, returns)``."""
    import torch

    from ._native import MrpError, load
    if not isinstance(rewards, torch.Tensor) or not rewards.is_cuda:
        raise ValueError("gae_device: rewards must be a CUDA tensor")
    if rewards.dim() != 2:
        raise ValueError(f"gae_device: rewards is {tuple(rewards.shape)}, expected [T, N]")
    dev, (T, N) = rewards.device, rewards.shape
    if (truncated is None) != (terminal_values is None):
        raise ValueError("gae_device: truncated and terminal_values are given together or not at all")
    if advantages is None:
        advantages = torch.empty((T, N), dtype=torch.float32, device=dev)
    if returns is None:
        returns = torch.empty((T, N), dtype=torch.float32, device=dev)
    f32, u8 = torch.float32, torch.uint8
    for name, t, dt, shape in (("rewards", rewards, f32, (T, N)), ("values", values, f32, (T, N)),
                               ("episode_starts", episode_starts, u8, (T, N)), ("last_values", last_values, f32, (N,)),
                               ("dones", dones, u8, (N,)), ("truncated", truncated, u8, (T, N)),
                               ("terminal_values", terminal_values, f32, (T, N)), ("advantages", advantages, f32, (T, N)),
                               ("returns", returns, f32, (T, N))):
        if t is not None:
            check_tensor("gae_device", name, t, dev, dt, shape)
    L = load()
    rc = L.mrp_gae_device(index_of(dev), stream_of(dev), T, N, ptr(rewards), ptr(values), ptr(episode_starts),
                          ptr(truncated), ptr(terminal_values), ptr(last_values), ptr(dones), float(gamma), float(gae_lambda),
                          ptr(advantages), ptr(returns))
    if rc == -1:
        raise ValueError(L.mrp_norm_last_error(None).decode())
    if rc != 0:
        raise MrpError(f"mrp_gae_device failed ({rc}): {L.mrp_norm_last_error(None).decode()}")
    return advantages, returns


def collect_rollouts(env, policy, buffer, obs, episode_start, norm=None, eps_out=None):
    """SB3's ``OnPolicyAlgorithm.collect_rollouts`` on the device, ``buffer.n_steps`` iterations with no
    host synchronisation: ``policy.act`` (a ``policy.DevicePolicy``), ``env.step_torch`` with the clipped
    actions, the optional ``DeviceVecNormalize.step`` (``norm``), ``policy.values`` at the terminal
    observations, ``buffer.add``; then ``last_values`` and ``compute_returns_and_advantage``.

    ``obs`` float32 [N, obs_dim] and ``episode_start`` uint8 [N] are the observations the policy sees
    first (after ``reset()``, normalised when ``norm`` is given) and ones after a reset, or what the
    previous call returned; neither is written.  ``eps_out`` (float32 [n_steps, N, act_dim], optional)
    receives the noise of every step.  The buffer is reset first.  Returns the next ``(obs,
    episode_start)``."""
    import torch
    N, T, dev = buffer.n_lanes, buffer.n_steps, buffer.device
    O, A = policy.obs_dim, policy.act_dim
    f32, u8 = torch.float32, torch.uint8
    check_tensors("collect_rollouts", dev, (("obs", obs, f32, (N, O), False), ("episode_start", episode_start, u8, (N,), False),
                                            ("eps_out", eps_out, f32, (T, N, A), True)))
    if tuple(buffer.obs_shape) != (O,) or buffer.act_dim != A:
        raise ValueError(f"collect_rollouts: the buffer holds obs {buffer.obs_shape} / {buffer.act_dim} actions, "
                         f"the policy takes ({O},) / {A}")
    z = lambda *s, dt=f32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    raw, rew, done, trunc, term = z(N, O), z(N), z(N, dt=u8), z(N, dt=u8), z(N, O)
    nobs, nrew, nterm = (z(N, O), z(N), z(N, O)) if norm is not None else (raw, rew, term)
    clipped, tvals = z(N, A), z(N)
    obs, episode_start = obs.clone(), episode_start.clone()
    buffer.reset()
    for t in range(T):
        # the row's actions, values and log-probs are written in place
        out = (buffer.actions[t], clipped, buffer.values[t], buffer.log_probs[t])
        policy.act(obs, out=out, eps_out=None if eps_out is None else eps_out[t])
        env.step_torch(clipped, raw, rew, done, truncated=trunc, terminal_obs=term)
        if norm is not None:
            norm.step(raw, rew, done, nobs, nrew, term_obs=term, term_out=nterm)
        policy.values(nterm, out=tvals)          # entries of lanes that did not truncate are ignored
        buffer.add(obs, buffer.actions[t], nrew, episode_start, buffer.values[t], buffer.log_probs[t], truncated=trunc,
                   terminal_value=tvals)
        obs.copy_(nobs)
        episode_start.copy_(done)
    buffer.compute_returns_and_advantage(policy.values(obs), episode_start)
    return obs, episode_start


class DeviceRolloutBuffer:
    """SB3's ``RolloutBuffer`` as preallocated torch tensors on ``device``: ``observations``
    [T, N, *obs_shape] (``obs_dtype``, None = torch.float32; uint8 frame stacks are allowed), ``actions`` [T, N, A],
    float32 [T, N] ``rewards`` / ``values`` / ``log_probs`` / ``terminal_values`` / ``advantages`` /
    ``returns`` and uint8 [T, N] ``episode_starts`` / ``truncated``.

    ``add`` copies one row on the device without a host sync; ``truncated`` and ``terminal_value``
    are ``step_torch``'s TimeLimit flags and the value function at its ``terminal_obs`` (entries of
    lanes that did not truncate are ignored).  ``compute_returns_and_advantage`` applies the bootstrap
    and GAE in one ``mrp_gae_device`` launch; ``get`` yields shuffled minibatches gathered on the device."""

    def __init__(self, n_steps, n_lanes, obs_shape, act_dim, device=0, gamma=0.99, gae_lambda=0.95, obs_dtype=None):
        import torch
        self.n_steps, self.n_lanes, self.obs_shape, self.act_dim = int(n_steps), int(n_lanes), tuple(obs_shape), int(act_dim)
        if self.n_steps < 1 or self.n_lanes < 1:
            raise ValueError("DeviceRolloutBuffer: n_steps and n_lanes must be >= 1")
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        T, N = self.n_steps, self.n_lanes
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=self.device)  # noqa: E731
        self.observations = z(T, N, *self.obs_shape, dt=torch.float32 if obs_dtype is None else obs_dtype)
        self.actions = z(T, N, self.act_dim)
        self.rewards, self.values, self.log_probs, self.terminal_values = z(T, N), z(T, N), z(T, N), z(T, N)
        self.advantages, self.returns = z(T, N), z(T, N)
        self.episode_starts, self.truncated = z(T, N, dt=torch.uint8), z(T, N, dt=torch.uint8)
        self.pos, self.full = 0, False

    def reset(self) -> None:
        self.pos, self.full = 0, False

    def add(self, obs, action, reward, episode_start, value, log_prob, truncated=None, terminal_value=None) -> None:
        """Store one transition of every lane in row ``pos``.  ``episode_start`` is the ``done`` of the
        step before (ones after ``reset()``); ``value`` / ``log_prob`` / ``terminal_value`` hold one
        entry per lane (a trailing axis of 1 is accepted)."""
        if self.full:
            raise RuntimeError("DeviceRolloutBuffer.add: the buffer is full")
        if (truncated is None) != (terminal_value is None):
            raise ValueError("DeviceRolloutBuffer.add: truncated and terminal_value are given together or not at all")
        p, N = self.pos, self.n_lanes
        self.observations[p].copy_(obs.reshape(self.observations[p].shape))
        self.actions[p].copy_(action.reshape(N, self.act_dim))
        self.rewards[p].copy_(reward.reshape(N))
        self.episode_starts[p].copy_(episode_start.reshape(N))
        self.values[p].copy_(value.reshape(N))
        self.log_probs[p].copy_(log_prob.reshape(N))
        if truncated is None:
            self.truncated[p].zero_()
            self.terminal_values[p].zero_()
        else:
            self.truncated[p].copy_(truncated.reshape(N))
            self.terminal_values[p].copy_(terminal_value.reshape(N))
        self.pos += 1
        self.full = self.pos == self.n_steps

    def compute_returns_and_advantage(self, last_values, dones):
        """GAE over the full buffer: ``last_values`` float32 [N] is the value function at the
        observations after the last row, ``dones`` uint8 (or bool) [N] that step's ``done``."""
        import torch
        if not self.full:
            raise RuntimeError("DeviceRolloutBuffer.compute_returns_and_advantage: the buffer is not full")
        last_values = last_values.reshape(self.n_lanes).contiguous()
        dones = dones.reshape(self.n_lanes).to(torch.uint8).contiguous()
        return gae_device(self.rewards, self.values, self.episode_starts, last_values, dones, self.gamma, self.gae_lambda,
                          self.truncated, self.terminal_values, self.advantages, self.returns)

    def flat_index(self, generator=None):
        """One epoch's sample order: a ``torch.randperm`` of the T*N samples in SB3's ``swap_and_flatten``
        order (sample ``i`` is lane ``i // T``, row ``i % T``) as int64 row numbers into ``flat_fields``."""
        import torch
        if not self.full:
            raise RuntimeError("DeviceRolloutBuffer: the buffer is not full")
        T, N = self.n_steps, self.n_lanes
        gdev = self.device if generator is None else generator.device
        perm = torch.randperm(T * N, generator=generator, device=gdev).to(self.device)
        return (perm % T) * N + perm // T     # row-major [T, N] position of sample i

    def flat_fields(self):
        """``[observations, actions, values, log_probs, advantages, returns]`` as row-major ``[T*N, ...]``
        views of the buffer's tensors."""
        total = self.n_steps * self.n_lanes
        fields = (self.observations, self.actions, self.values, self.log_probs, self.advantages, self.returns)
        return [f.reshape(total, *f.shape[2:]) for f in fields]

    def get(self, batch_size=None, generator=None):
        """Yield ``(observations, actions, old_values, old_log_prob, advantages, returns)`` minibatches
        that follow a ``torch.randperm`` of the T*N samples in SB3's ``swap_and_flatten`` order: flat
        index ``i`` is lane ``i // T``, row ``i % T``.  ``batch_size=None``: one batch of everything;
        the last batch holds the remainder."""
        flat, fields = self.flat_index(generator), self.flat_fields()
        total = self.n_steps * self.n_lanes
        batch_size = total if batch_size is None else int(batch_size)
        for start in range(0, total, batch_size):
            idx = flat[start:start + batch_size]
            yield tuple(f.index_select(0, idx) for f in fields)
