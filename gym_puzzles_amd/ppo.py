"""Device PPO update: one optimiser step of stable-baselines3's ``PPO.train()`` on a minibatch --
``evaluate_actions``, the clipped surrogate, value and entropy losses, the backward pass through
``ActorCriticPolicy`` / ``MlpExtractor``, global grad-norm clipping and Adam -- as HIP kernels that
write the device policy's parameters in place (``csrc/mrp_ppo.hip``, ``mrp_ppo_*`` in
``include/mrp.h``), with no host synchronisation and no atomics.

``ppo_grad_ref``, ``adam_ref`` and ``ppo_train_ref`` are the numpy statement of the rule and the
definition the kernels match bit for bit.  Everything is float32 with every operation rounded on its
own unless stated otherwise; ``B`` is the minibatch size, ``invB = float32(1.0 / B)``.

* ``exp_ref``: this build's float32 exp (``csrc/mrp_math.h`` ``exp_f32``), operation for operation;
* evaluate: ``mean`` and ``value`` are the forward rule's (``policy.linear_ref`` chains, ``tanh_ref`` /
  relu), ``d = action - mean`` and ``log_prob`` is ``policy_ref``'s formula on the stored, unclipped
  action; the entropy is ``sum_i((0.5 + LOG_SQRT_2PI) + log_std_i)`` ascending from +0;
* loss terms: ``ratio = exp(log_prob - old_log_prob)``, ``pl1 = adv * ratio``, ``pl2 = adv *
  fmin_(fmax_(ratio, 1 - c), 1 + c)``, the policy term ``-(pl1 <= pl2 ? pl1 : pl2)``, the value term
  ``(ret - v) * (ret - v)``; ``clip_range_vf`` and ``target_kl`` are not built;
* upstream gradients: ``g = (pl1 <= pl2) ? (-(adv * ratio)) * invB : +0``, ``dmean_i = g * (d_i /
  (std_i * std_i))``, the ``log_std`` term ``g * ((d_i * d_i) / (std_i * std_i) - 1)``, ``dvalue =
  ((v - ret) * float32(2 * vf_coef)) * invB``;
* backprop: into a head's input ``s[k] = fma chain over the head's outputs i ascending from +0 of
  fma(dmean_i, Wa[i][k], acc)`` (the value head is one product); through a hidden layer ``s[n][k] =
  fma chain over j ascending from +0 of fma(delta_out[n][j], W[j][k], acc)``, then ``delta_in = s *
  act'`` with ``tanh' = fma(-t, t, 1)`` and ``relu' = t > 0 ? 1 : 0`` on the stored activation ``t``;
  at the trunk's output the towers' ``s`` add as ``s_pi + s_vf``; no observation gradient, no pad terms;
* parameter gradients in chunks of ``CHUNK`` samples in minibatch order: within a chunk ``dW[j][k] =
  fma chain over n ascending from +0 of fma(delta[n][j], x[n][k], acc)``, ``db[j]`` and the
  ``log_std`` terms plain adds from +0; the chunks' partials are added in ascending order starting
  from chunk 0's; ``log_std``'s gradient gets ``- float32(ent_coef)`` added last;
* statistics (policy loss, value loss, entropy loss, approx_kl, clip fraction): float64 sums from 0.0
  of the float32 per-sample terms, each chunk sequential, then the chunks sequential, times ``1.0 /
  B`` in float64, rounded to float32 once;
* clip: flat order ``log_std``, trunk, policy tower, value tower, action head, value head (each
  ``weight`` row-major, then ``bias``: SB3's ``parameters()``); float64 sum of squares, partial ``t``
  (0..255) over elements ``t, t + 256, ...``, then the partials ascending; ``coef = float32(min(1,
  max_grad_norm / (sqrt(sum) + 1e-6)))``; every gradient is multiplied by ``coef``;
* Adam (``adam_ref`` holds the operation order), then ``std = exp_ref(log_std)``.

``normalize_advantage`` in ``DevicePPO`` is torch arithmetic on the gathered minibatch and lies
outside the bitwise rule: the rule takes the advantages it is given.  The module is pure numpy at
import; ``DevicePPO`` imports torch when used.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from ._device import Handle, check_tensor, ptr, stream_of
from .policy import (_INV_LN2, _LN2_HI, _LN2_LO, _TANH_C, LOG_SQRT_2PI, PolicyParams, _activate, _layers,  # noqa: F401
                     flatten_params, fma32, linear_ref, state_dict_from_params, unflatten_params)

_f32, _f64 = np.float32, np.float64
CHUNK = 256            # samples per partial sum of a parameter gradient (and of a statistic)
NORM_LANES = 256       # interleaved partials of the grad-norm's sum of squares
STAT_NAMES = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")
EXP_LO, EXP_HI = -104.0, 89.0     # exp_f32 clamps its argument here: exp(-104) rounds to +0, exp(89) to +inf


# ---- exp ---------------------------------------------------------------------------------------------
def exp_ref(x):
    """``exp_f32`` of ``csrc/mrp_math.h`` on a float32 array, operation for operation: float64
    arithmetic rounded per operation, ``n = nearest(y / ln 2)`` (ties away), the two-part ``ln 2``
    reduction, the degree-11 Taylor ``expm1``, ``2^n (1 + p)`` and one rounding to float32 (which
    takes overflow to +inf and underflow through the subnormals to +0).  NaN comes back unchanged."""
    x = np.ascontiguousarray(x, _f32)
    ux = x.view(np.uint32)
    nan = (ux & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    with np.errstate(all="ignore"):
        y = np.where(nan, _f32(0.0), x).astype(_f64)
        y = np.where(y < EXP_LO, EXP_LO, y)
        y = np.where(y > EXP_HI, EXP_HI, y)
        t = y * _INV_LN2
        n = np.trunc(t + np.where(t < 0.0, -0.5, 0.5)).astype(np.int64)
        dn = n.astype(_f64)
        r = (y - dn * _LN2_HI) - dn * _LN2_LO
        q = np.full_like(r, _TANH_C[11])
        for k in range(10, 1, -1):
            q = q * r + _TANH_C[k]
        p = r + (r * r) * q
        e = (((1023 + n) << 52).view(_f64) * (1.0 + p)).astype(_f32)
    return np.where(nan, ux, e.view(np.uint32)).astype(np.uint32).view(_f32)


# ---- the gradient rule -------------------------------------------------------------------------------
def _seq_sum64(x):
    """Sequential float64 sum from 0.0 (``np.sum`` adds pairwise)."""
    return np.cumsum(np.concatenate([[0.0], np.asarray(x, _f64)]))[-1]


def _chunk_sum64(x):
    return _seq_sum64([_seq_sum64(x[s:s + CHUNK]) for s in range(0, len(x), CHUNK)])


def _act_prime(t, activation):
    if activation == "tanh":
        return fma32(-t, t, _f32(1.0))
    return np.where(t > 0, _f32(1.0), _f32(0.0)).astype(_f32)


def _weight_grad(delta, x):
    """Chunked ``dW[j][k]`` and ``db[j]`` of one layer: float32 [out, in], [out]."""
    B = delta.shape[0]
    dw = db = None
    for s in range(0, B, CHUNK):
        dc, xc = delta[s:s + CHUNK], x[s:s + CHUNK]
        pw = linear_ref(dc.T, xc.T, np.zeros(x.shape[1], _f32))     # chain over n of fma(delta[n][j], x[n][k], acc)
        pb = _col_sum(dc)
        dw, db = (pw, pb) if dw is None else (dw + pw, db + pb)
    return dw.astype(_f32), db.astype(_f32)


def _col_sum(a):
    acc = np.zeros(a.shape[1], _f32)
    for n in range(a.shape[0]):
        acc = acc + a[n]
    return acc


def _chunked_col_sum(a):
    out = None
    for s in range(0, a.shape[0], CHUNK):
        p = _col_sum(a[s:s + CHUNK])
        out = p if out is None else out + p
    return out.astype(_f32)


def _evaluate(params, obs, actions):
    """SB3's ``evaluate_actions`` by the forward rule, with what the backward pass needs: the layers'
    activations ``(trunk layers, trunk output, policy-tower layers, value-tower layers, the heads'
    inputs)``, ``values``, ``log_prob`` (``policy_ref``'s formula on ``actions``), the entropy, ``d =
    actions - mean`` and ``std * std``.  ``tests/test_ppo.py`` pins ``values`` and ``log_prob`` to
    ``policy_ref``'s bit for bit: a ratio of exactly 1 on unchanged parameters rests on that."""
    def forward(layers, x):
        ts = []
        for w, b in layers:
            x = _activate(linear_ref(x, w, b), params.activation)
            ts.append(x)
        return ts
    t_sh = forward(params.shared, obs)
    trunk = t_sh[-1] if t_sh else obs
    t_pi, t_vf = forward(params.pi, trunk), forward(params.vf, trunk)
    f_pi, f_vf = (t_pi[-1] if t_pi else trunk), (t_vf[-1] if t_vf else trunk)
    mean = linear_ref(f_pi, *params.action)
    v = linear_ref(f_vf, *params.value)[:, 0]
    std, log_std = params.std[None, :], params.log_std[None, :]
    d = actions - mean
    var = std * std
    terms = ((-(d * d)) / (_f32(2.0) * var) - log_std) - LOG_SQRT_2PI
    lp = np.zeros(obs.shape[0], _f32)
    for i in range(params.act_dim):
        lp = lp + terms[:, i]
    ent = _f32(0.0)
    for i in range(params.act_dim):
        ent = _f32(ent + ((_f32(0.5) + LOG_SQRT_2PI) + params.log_std[i]))
    return (t_sh, trunk, t_pi, t_vf, f_pi, f_vf), v, lp, ent, d, var


def evaluate_actions_ref(params, obs, actions):
    """``(values [N], log_prob [N], entropy)`` of SB3's ``evaluate_actions`` by the rule: float32, the
    entropy one number (it does not depend on the sample)."""
    obs = np.ascontiguousarray(obs, _f32)
    actions = np.ascontiguousarray(actions, _f32).reshape(obs.shape[0], params.act_dim)
    with np.errstate(over="ignore", invalid="ignore"):
        _, v, lp, ent, _, _ = _evaluate(params, obs, actions)
    return v, lp, ent


def ppo_grad_ref(params, obs, actions, old_log_probs, advantages, returns, clip_range=0.2, ent_coef=0.0, vf_coef=0.5):
    """The flat gradient (float32, ``flatten_params`` order) of SB3's PPO loss on one minibatch and the
    five statistics (float32 [5], ``STAT_NAMES``), by the rule of the module docstring."""
    obs = np.ascontiguousarray(obs, _f32)
    B, A = obs.shape[0], params.act_dim
    actions = np.ascontiguousarray(actions, _f32).reshape(B, A)
    old, adv, ret = (np.ascontiguousarray(v, _f32).reshape(B) for v in (old_log_probs, advantages, returns))
    act = params.activation
    invB, c = _f32(1.0 / B), _f32(clip_range)
    vf2, ent_c = _f32(2.0 * float(vf_coef)), _f32(ent_coef)

    with np.errstate(over="ignore", invalid="ignore"):
        (t_sh, trunk, t_pi, t_vf, f_pi, f_vf), v, lp, ent, d, var = _evaluate(params, obs, actions)
        diff = lp - old
        ratio = exp_ref(diff)
        lo, hi = _f32(1.0) - c, _f32(1.0) + c
        clamped = np.where(ratio > lo, ratio, lo)                 # fmax_(ratio, lo), then fmin_(., hi)
        clamped = np.where(clamped < hi, clamped, hi).astype(_f32)
        pl1, pl2 = adv * ratio, adv * clamped
        first = pl1 <= pl2
        p_term = -np.where(first, pl1, pl2)
        v_term = (ret - v) * (ret - v)
        kl_term = (ratio - _f32(1.0)) - diff
        clip_term = (np.abs(ratio - _f32(1.0)) > c).astype(_f32)
        e_term = np.full(B, -ent, _f32)
        stats = np.array([_chunk_sum64(t) * (1.0 / B) for t in (p_term, v_term, e_term, kl_term, clip_term)]).astype(_f32)

        g = np.where(first, (-(adv * ratio)) * invB, _f32(0.0)).astype(_f32)
        dmean = g[:, None] * (d / var)
        ls_term = g[:, None] * ((d * d) / var - _f32(1.0))
        dvalue = (((v - ret) * vf2) * invB)[:, None]

        grads = {}

        def backward(layers, ts, s, inputs, key):
            """``s``: the gradient at the tower's output; returns it at the tower's input."""
            for i in range(len(layers) - 1, -1, -1):
                w = layers[i][0]
                delta = (s * _act_prime(ts[i], act)).astype(_f32)
                grads[key, i] = _weight_grad(delta, inputs[i])
                s = linear_ref(delta, w.T, np.zeros(w.shape[1], _f32)) if inputs[i] is not obs else None
            return s
        wa, wv = params.action[0], params.value[0]
        grads["action", 0] = _weight_grad(dmean.astype(_f32), f_pi)
        grads["value", 0] = _weight_grad(dvalue.astype(_f32), f_vf)
        s_pi = linear_ref(dmean, wa.T, np.zeros(wa.shape[1], _f32))
        s_vf = (dvalue * wv[0][None, :]).astype(_f32)
        s_pi = backward(params.pi, t_pi, s_pi, [trunk] + t_pi[:-1], "pi")
        s_vf = backward(params.vf, t_vf, s_vf, [trunk] + t_vf[:-1], "vf")
        if params.shared:
            backward(params.shared, t_sh, s_pi + s_vf, [obs] + t_sh[:-1], "shared")
        g_ls = _chunked_col_sum(ls_term.astype(_f32)) + (-ent_c)
    parts = [g_ls]
    for key, n in (("shared", len(params.shared)), ("pi", len(params.pi)), ("vf", len(params.vf)), ("action", 1), ("value", 1)):
        for i in range(n):
            parts += [grads[key, i][0].ravel(), grads[key, i][1]]
    return np.concatenate(parts).astype(_f32), stats


# ---- clip and Adam -----------------------------------------------------------------------------------
def clip_coef_ref(grad, max_grad_norm):
    """``clip_grad_norm_``'s factor as float32: the float64 sum of squares in ``NORM_LANES`` interleaved
    partials (each sequential, then the partials ascending), ``min(1, max / (sqrt(sum) + 1e-6))``."""
    g = np.ascontiguousarray(grad, _f32).astype(_f64)
    sq = np.concatenate([g * g, np.zeros(-g.size % NORM_LANES)]).reshape(-1, NORM_LANES)
    partial = np.cumsum(np.concatenate([np.zeros((1, NORM_LANES)), sq]), axis=0)[-1]
    total = _seq_sum64(partial)
    return _f32(min(1.0, float(max_grad_norm) / (math.sqrt(total) + 1e-6)))


class AdamState:
    """Adam's first and second moments (flat float32, ``flatten_params`` order) and the step count."""

    def __init__(self, n):
        self.m, self.v, self.t = np.zeros(n, _f32), np.zeros(n, _f32), 0


def adam_scalars(t, lr, betas=(0.9, 0.999), eps=1e-5):
    """The float32 scalars of step ``t`` (1-based), computed in float64: ``(b1, 1 - b1, b2, 1 - b2,
    sqrt(1 - b2^t), lr / (1 - b1^t), eps)``."""
    b1, b2 = float(betas[0]), float(betas[1])
    return tuple(_f32(x) for x in (b1, 1.0 - b1, b2, 1.0 - b2, math.sqrt(1.0 - b2 ** t), float(lr) / (1.0 - b1 ** t), eps))


def adam_ref(p, grad, state, lr, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-5):
    """One clipped Adam step on flat float32 vectors (torch's formula, SB3's ``eps``); advances
    ``state`` in place and returns ``(new p, coef)``.  Every operation is float32 and rounded alone:

        g = grad * coef;  m = (b1 * m) + (omb1 * g);  v = (b2 * v) + ((omb2 * g) * g)
        p = p - step * (m / ((sqrt(v) / sqrt_bc2) + eps))
    """
    coef = clip_coef_ref(grad, max_grad_norm)
    state.t += 1
    b1, omb1, b2, omb2, sbc2, step, e = adam_scalars(state.t, lr, betas, eps)
    g = np.ascontiguousarray(grad, _f32) * coef
    state.m = ((b1 * state.m) + (omb1 * g)).astype(_f32)
    state.v = ((b2 * state.v) + ((omb2 * g) * g)).astype(_f32)
    denom = (np.sqrt(state.v) / sbc2) + e
    return (np.ascontiguousarray(p, _f32) - step * (state.m / denom)).astype(_f32), coef


def ppo_step_ref(params, state, batch, lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 betas=(0.9, 0.999), eps=1e-5):
    """``ppo_grad_ref`` then ``adam_ref`` on one minibatch ``(obs, actions, old_log_probs, advantages,
    returns)``; returns ``(new params with std = exp_ref(log_std), stats)``."""
    grad, stats = ppo_grad_ref(params, *batch, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef)
    flat, _ = adam_ref(flatten_params(params), grad, state, lr, max_grad_norm, betas, eps)
    return unflatten_params(params, flat, std=exp_ref(flat[:params.act_dim])), stats


def ppo_train_ref(params, state, data, epochs, batch_size, **hp):
    """SB3's ``PPO.train()`` loop on host arrays: ``data = (obs, actions, old_log_probs, advantages,
    returns)`` with the samples along axis 0, ``epochs`` one index array per epoch (the shuffled sample
    order); every epoch is cut into consecutive minibatches of ``batch_size`` (the last may be short),
    one ``ppo_step_ref`` each.  Returns ``(params, stats [n_updates, 5])``; ``state.t`` counts the steps."""
    stats = []
    for order in epochs:
        order = np.asarray(order)
        for s in range(0, order.size, int(batch_size)):
            idx = order[s:s + int(batch_size)]
            params, st = ppo_step_ref(params, state, tuple(np.asarray(a)[idx] for a in data), **hp)
            stats.append(st)
    return params, np.array(stats, _f32).reshape(-1, 5)


# ---- the device class --------------------------------------------------------------------------------
class DevicePPO(Handle):
    """The rule on the device: ``grad`` is ``ppo_grad_ref``, ``step`` is ``ppo_step_ref`` written into
    ``policy``'s device parameters in place (the next ``policy.act`` uses them), ``train`` is SB3's
    epoch / minibatch loop over a ``DeviceRolloutBuffer``.  Nothing here synchronises the device; the
    statistics stay in device tensors.  The optimiser state (master parameters, gradient, Adam moments)
    belongs to this object; ``policy.set_params`` afterwards is picked up by the next call and leaves
    the moments as they are.  ``learning_rate`` is read at every step.  The library reads ``policy``'s
    handle in every call, so a call after ``policy.close()`` raises ``ValueError``."""

    _DESTROY, _LAST_ERROR, _VALUE_ERRORS = "mrp_ppo_destroy", "mrp_ppo_last_error", (-1, -3)

    def __init__(self, policy, learning_rate=3e-4, n_epochs=10, batch_size=64, clip_range=0.2, ent_coef=0.0, vf_coef=0.5,
                 max_grad_norm=0.5, normalize_advantage=True, betas=(0.9, 0.999), eps=1e-5, max_batch=None):
        self.policy, self.learning_rate, self.n_epochs, self.batch_size = policy, learning_rate, int(n_epochs), int(batch_size)
        self.clip_range, self.ent_coef, self.vf_coef, self.max_grad_norm = clip_range, ent_coef, vf_coef, max_grad_norm
        self.normalize_advantage, self.betas, self.eps = bool(normalize_advantage), tuple(betas), eps
        self.max_batch = int(self.batch_size if max_batch is None else max_batch)
        self.t = 0
        self.device = policy.device
        self._open("mrp_ppo_create", policy._h, self.max_batch)
        self.n_params = int(self._L.mrp_ppo_n_params(self._h))

    @property
    def _h(self):
        self.policy._h     # mrp_ppo reads the policy's handle in every call: ValueError once that is closed
        return super()._h

    def _batch(self, obs, actions, old_log_probs, advantages, returns):
        import torch
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError("DevicePPO: obs must be a [B, obs_dim] CUDA tensor")
        B, f32 = int(obs.shape[0]), torch.float32
        if B < 1:
            raise ValueError("DevicePPO: the minibatch holds no sample")
        named = (("obs", obs, (B, self.policy.obs_dim)), ("actions", actions, (B, self.policy.act_dim)),
                 ("old_log_probs", old_log_probs, (B,)), ("advantages", advantages, (B,)), ("returns", returns, (B,)))
        for name, t, shape in named:
            check_tensor("DevicePPO", name, t, self.device, f32, shape)
        if B > self.max_batch:
            raise ValueError(f"DevicePPO: a minibatch of {B} samples, max_batch is {self.max_batch}")
        return B, [ptr(t) for _, t, _ in named]

    def _out(self, name, t, n):
        import torch
        if t is None:
            return torch.empty(n, dtype=torch.float32, device=self.device)
        check_tensor("DevicePPO", name, t, self.device, torch.float32, (n,))
        return t

    def grad(self, obs, actions, old_log_probs, advantages, returns, out=None, stats_out=None):
        """``ppo_grad_ref`` on the device: returns ``(flat_grad [n_params], stats [5])`` device
        tensors (``out`` / ``stats_out`` when given).  Parameters and optimiser state are not changed.
        An output whose memory overlaps an input's or the other output's anywhere raises ``ValueError``."""
        B, ptrs = self._batch(obs, actions, old_log_probs, advantages, returns)
        g, st = self._out("out", out, self.n_params), self._out("stats_out", stats_out, 5)
        f = ctypes.c_float
        self._check_rc(self._L.mrp_ppo_grad_device(self._h, stream_of(self.device), B, *ptrs, f(self.clip_range), f(self.ent_coef),
                                                   ctypes.c_double(self.vf_coef), ptr(g), ptr(st)))
        return g, st

    def step(self, obs, actions, old_log_probs, advantages, returns, stats_out=None):
        """One optimiser step (``ppo_step_ref``) in place; returns the ``stats [5]`` device tensor."""
        B, ptrs = self._batch(obs, actions, old_log_probs, advantages, returns)
        st = self._out("stats_out", stats_out, 5)
        sc = adam_scalars(self.t + 1, self.learning_rate, self.betas, self.eps)
        f = ctypes.c_float
        self._check_rc(self._L.mrp_ppo_step_device(self._h, stream_of(self.device), B, *ptrs, f(self.clip_range), f(self.ent_coef),
                                                   ctypes.c_double(self.vf_coef), ctypes.c_double(self.max_grad_norm),
                                                   *[f(float(x)) for x in sc], ptr(st)))
        self.t += 1
        return st

    def train(self, buffer, generator=None):
        """``n_epochs`` passes over ``buffer.get(batch_size, generator)``, one ``step`` per minibatch;
        returns the ``[n_updates, 5]`` device tensor of statistics.  ``normalize_advantage`` is SB3's
        ``(adv - adv.mean()) / (adv.std() + 1e-8)`` as torch operations on the gathered minibatch
        (unbiased std, skipped for one sample): outside the bitwise rule."""
        import torch
        total = buffer.n_steps * buffer.n_lanes
        per_epoch = -(-total // self.batch_size)
        stats = torch.zeros(self.n_epochs * per_epoch, 5, dtype=torch.float32, device=self.device)
        u = 0
        for _ in range(self.n_epochs):
            for obs, actions, _, old_lp, adv, ret in buffer.get(self.batch_size, generator):
                if self.normalize_advantage and adv.numel() > 1:
                    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
                self.step(obs.reshape(obs.shape[0], -1), actions, old_lp, adv, ret, stats_out=stats[u])
                u += 1
        return stats

    def state(self):
        """``(m, v)``: host copies of Adam's moments, flat float32 (synchronises the device)."""
        m, v = np.zeros(self.n_params, _f32), np.zeros(self.n_params, _f32)
        self._check_rc(self._L.mrp_ppo_get_state(self._h, m.ctypes.data, v.ctypes.data))
        return m, v
