"""Device PPO update: one optimiser step of stable-baselines3's ``PPO.train()`` on a minibatch --
``evaluate_actions``, the clipped surrogate, value and entropy losses, the backward pass through
``ActorCriticPolicy`` / ``MlpExtractor``, global grad-norm clipping and Adam -- as HIP kernels that
write the device policy's parameters in place (``csrc/mrp_ppo.hip``, ``mrp_ppo_*`` in
``include/mrp.h``), with no host synchronisation and no atomics.

``ppo_grad_ref``, ``adam_ref``, ``normalize_adv_ref``, ``kl_stop_ref``, ``ppo_train_ref``, ``combine_ref`` and
``ppo_train_dist_ref`` are the numpy statement of the rule and the definition the kernels match bit for bit.  Everything is float32 with every operation rounded on its
own unless stated otherwise; ``B`` is the minibatch size, ``invB = float32(1.0 / B)``.

* ``exp_ref``: this build's float32 exp (``csrc/mrp_math.h`` ``exp_f32``), operation for operation;
* evaluate: ``mean`` and ``value`` are the forward rule's (``policy.linear_ref`` chains, ``tanh_ref`` /
  relu), ``d = action - mean`` and ``log_prob`` is ``policy_ref``'s formula on the stored, unclipped
  action; the entropy is ``sum_i((0.5 + LOG_SQRT_2PI) + log_std_i)`` ascending from +0;
* loss terms: ``ratio = exp(log_prob - old_log_prob)``, ``pl1 = adv * ratio``, ``pl2 = adv *
  fmin_(fmax_(ratio, 1 - c), 1 + c)``, the policy term ``-(pl1 <= pl2 ? pl1 : pl2)``, the value term
  ``(ret - v) * (ret - v)``;
* ``clip_range_vf`` (``cv``, with the rollout's ``old_values``): ``dv = v - old_v``, ``vp = old_v +
  fmin_(fmax_(dv, -cv), cv)``, the value term ``(ret - vp) * (ret - vp)``, and ``dvalue = ((vp - ret) *
  float32(2 * vf_coef)) * invB`` where ``dv >= -cv and dv <= cv`` (torch's clamp backward is inclusive at
  both ends), ``+0`` elsewhere; without it ``vp`` is ``v`` and every sample passes;
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
* Adam (``adam_ref`` holds the operation order), then ``std = exp_ref(log_std)``;
* ``normalize_adv_ref``: SB3's ``(adv - adv.mean()) / (adv.std() + 1e-8)`` on a minibatch in float64, each
  operation rounded alone: ``mean = chunk sum of adv * (1.0 / B)``, ``dev_i = float64(adv_i) - mean``, ``var
  = chunk sum of dev * dev / (B - 1)``, ``out_i = float32(dev_i / (sqrt(var) + 1e-8))``; the chunk sums are
  the statistics' (``CHUNK`` samples sequential from 0.0, then the chunks sequential); one sample is
  returned as it is;
* ``target_kl`` (``kl_stop_ref``): after a minibatch's statistics, ``float64(approx_kl) > 1.5 *
  float64(target_kl)`` (strict) means that this minibatch is not applied and the whole ``train`` call
  ends; ``ppo_train_ref`` holds the order;
* data-parallel training (``combine_ref``, ``ppo_train_dist_ref``): ``R`` ranks hold one copy of the
  parameters and of Adam's state each and a rollout buffer of their own.  For a minibatch every rank ``r``
  computes ``g_r, s_r = ppo_grad_ref`` on its local minibatch with ``invB = float32(1.0 / B_local)`` (its
  advantages through ``normalize_adv_ref`` on the local minibatch first, ``clip_range_vf`` as above): the
  gradient before clipping.  Then ``g = g_0; g = g + g_1; ...; g = g + g_{R-1}`` in ascending rank order,
  every add a float32 add rounded alone, and ``g = g * float32(1.0 / R)``; the five statistics are combined
  by the same adds and the same multiply in float32 (all five are means).  At ``R = 1`` this is the
  identity, signed zeros included.  ``kl_stop_ref`` then decides on the combined ``approx_kl``, and if it
  does not stop ``clip_coef_ref`` and ``adam_ref`` run on the combined gradient, with the combined row as
  the statistics row recorded.  The order is fixed and nothing is atomic, so every rank computes the same
  bits: after any number of minibatches the ranks' parameters, ``std``, moments, ``t`` and ``stopped`` are
  identical.  The combined gradient is the gradient of the mean of the ranks' losses; it is not, bit for
  bit, what one rank holding the union minibatch computes (that is another chunk order).

``DevicePPO(minibatch="device")`` gathers the minibatch and normalises its advantages by this rule in HIP;
with ``minibatch="torch"`` (the default) the gather is ``index_select`` and ``normalize_advantage`` is
torch arithmetic on the gathered minibatch, outside the bitwise rule: the rule takes the advantages it
is given.  The module is pure numpy at import; ``DevicePPO`` imports torch when used.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from ._device import Handle, check_tensor, check_tensors, ptr, stream_of
from .dist import agree, broadcast_array
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


def ppo_grad_ref(params, obs, actions, old_log_probs, advantages, returns, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, *,
                 old_values=None, clip_range_vf=None):
    """The flat gradient (float32, ``flatten_params`` order) of SB3's PPO loss on one minibatch and the
    five statistics (float32 [5], ``STAT_NAMES``), by the rule of the module docstring.  ``clip_range_vf``
    (with ``old_values`` [B], the rollout's value predictions) is SB3's value clipping."""
    if clip_range_vf is not None and old_values is None:
        raise ValueError("ppo_grad_ref: clip_range_vf needs old_values")
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
        if clip_range_vf is None:
            vp, passed = v, np.ones(B, bool)
        else:
            old_v, cv = np.ascontiguousarray(old_values, _f32).reshape(B), _f32(clip_range_vf)
            dv = v - old_v
            cl = np.where(dv > -cv, dv, -cv)                         # fmax_(dv, -cv), then fmin_(., cv)
            cl = np.where(cl < cv, cl, cv).astype(_f32)
            vp, passed = old_v + cl, (dv >= -cv) & (dv <= cv)
        v_term = (ret - vp) * (ret - vp)
        kl_term = (ratio - _f32(1.0)) - diff
        clip_term = (np.abs(ratio - _f32(1.0)) > c).astype(_f32)
        e_term = np.full(B, -ent, _f32)
        stats = np.array([_chunk_sum64(t) * (1.0 / B) for t in (p_term, v_term, e_term, kl_term, clip_term)]).astype(_f32)

        g = np.where(first, (-(adv * ratio)) * invB, _f32(0.0)).astype(_f32)
        dmean = g[:, None] * (d / var)
        ls_term = g[:, None] * ((d * d) / var - _f32(1.0))
        dvalue = np.where(passed, ((vp - ret) * vf2) * invB, _f32(0.0)).astype(_f32)[:, None]

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


def normalize_adv_ref(adv):
    """SB3's ``(adv - adv.mean()) / (adv.std() + 1e-8)`` (unbiased std) on one minibatch by the rule of
    the module docstring: float64, every operation rounded alone, the sums in the statistics' chunk order,
    one rounding to float32.  A single sample comes back unchanged, as SB3 skips it."""
    adv = np.ascontiguousarray(adv, _f32).reshape(-1)
    B = adv.size
    if B == 1:
        return adv.copy()
    mean = _chunk_sum64(adv) * (1.0 / B)
    dev = adv.astype(_f64) - mean
    var = _chunk_sum64(dev * dev) / (B - 1)
    return (dev / (math.sqrt(var) + 1e-8)).astype(_f32)


def kl_stop_ref(approx_kl_stat, target_kl):
    """SB3's early stop on the rule's float32 ``approx_kl`` statistic: strictly above ``1.5 * target_kl``."""
    return bool(_f64(approx_kl_stat) > 1.5 * _f64(target_kl))


def ppo_step_ref(params, state, batch, lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 betas=(0.9, 0.999), eps=1e-5, *, old_values=None, clip_range_vf=None):
    """``ppo_grad_ref`` then ``adam_ref`` on one minibatch ``(obs, actions, old_log_probs, advantages,
    returns)``; returns ``(new params with std = exp_ref(log_std), stats)``."""
    grad, stats = ppo_grad_ref(params, *batch, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef, old_values=old_values,
                               clip_range_vf=clip_range_vf)
    return _apply_ref(params, state, grad, lr, max_grad_norm, betas, eps), stats


def _apply_ref(params, state, grad, lr, max_grad_norm, betas, eps):
    flat, _ = adam_ref(flatten_params(params), grad, state, lr, max_grad_norm, betas, eps)
    return unflatten_params(params, flat, std=exp_ref(flat[:params.act_dim]))


def ppo_train_ref(params, state, data, epochs, batch_size, *, old_values=None, normalize_advantage=False, clip_range_vf=None,
                  target_kl=None, lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, betas=(0.9, 0.999),
                  eps=1e-5):
    """SB3's ``PPO.train()`` loop on host arrays: ``data = (obs, actions, old_log_probs, advantages,
    returns)`` (and ``old_values`` for ``clip_range_vf``) with the samples along axis 0, ``epochs`` one index
    array per epoch (the shuffled sample order); every epoch is cut into consecutive minibatches of
    ``batch_size`` (the last may be short).  A minibatch is evaluated (its advantages through
    ``normalize_adv_ref`` first with ``normalize_advantage``) and its statistics row appended; with
    ``target_kl``, if ``kl_stop_ref`` holds it is not applied and the whole call ends; otherwise the clip
    and Adam are applied.  Returns ``(params, stats [n_evaluated, 5])``, the stopping minibatch's row
    included; ``state.t`` counts the applied steps only."""
    stats = []
    stop = False
    for order in epochs:
        order = np.asarray(order)
        for s in range(0, order.size, int(batch_size)):
            idx = order[s:s + int(batch_size)]
            obs, actions, old_lp, adv, ret = (np.asarray(a)[idx] for a in data)
            if normalize_advantage:
                adv = normalize_adv_ref(adv)
            grad, st = ppo_grad_ref(params, obs, actions, old_lp, adv, ret, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef,
                                    old_values=None if old_values is None else np.asarray(old_values)[idx], clip_range_vf=clip_range_vf)
            stats.append(st)
            stop = target_kl is not None and kl_stop_ref(st[3], target_kl)
            if stop:
                break
            params = _apply_ref(params, state, grad, lr, max_grad_norm, betas, eps)
        if stop:
            break
    return params, np.array(stats, _f32).reshape(-1, 5)


# ---- data-parallel training --------------------------------------------------------------------------
def combine_ref(grads, stats):
    """The ranks' gradients (float32 ``[R, n_params]``) and statistics (float32 ``[R, 5]``), one row per
    rank in ascending rank order, combined by the rule of the module docstring: ``g = rows[0]``, then ``g = g
    + rows[r]`` for ``r = 1 .. R - 1`` (float32 adds, each rounded alone), then ``g * float32(1.0 / R)``.
    Returns ``(grad [n_params], stats [5])``; the identity at ``R = 1``."""
    grads, stats = np.ascontiguousarray(grads, _f32), np.ascontiguousarray(stats, _f32)
    if grads.ndim != 2 or grads.shape[0] < 1 or stats.shape != (grads.shape[0], 5):
        raise ValueError("combine_ref: grads is [R, n_params] and stats [R, 5] with R >= 1")
    R = grads.shape[0]
    inv = _f32(1.0 / R)

    def combine(rows):
        g = rows[0].copy()
        for r in range(1, R):
            g = (g + rows[r]).astype(_f32)
        return (g * inv).astype(_f32)
    with np.errstate(over="ignore", invalid="ignore"):
        return combine(grads), combine(stats)


def ppo_train_dist_ref(params, state, datas, epochs, batch_size, perms, *, old_values=None, normalize_advantage=False,
                       clip_range_vf=None, target_kl=None, lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                       betas=(0.9, 0.999), eps=1e-5):
    """``ppo_train_ref`` for ``R = len(datas)`` ranks in lockstep.  ``datas[r]`` is rank ``r``'s ``(obs,
    actions, old_log_probs, advantages, returns)`` (``old_values[r]`` its value predictions for
    ``clip_range_vf``), ``perms[r]`` its ``epochs`` index arrays (one sample order per epoch).  For every
    minibatch each rank takes its own rows by its own order, normalises its local advantages with
    ``normalize_advantage`` and runs ``ppo_grad_ref``; ``combine_ref``'s row is the statistics row recorded;
    ``kl_stop_ref`` on the combined ``approx_kl`` ends the call for every rank; otherwise the clip and Adam
    run on the combined gradient.  One ``params`` and one ``state`` serve all ranks.  ``ValueError`` unless
    every rank has ``epochs`` orders of one common length.  Returns ``(params, stats [n_evaluated, 5])``."""
    R, epochs, bs = len(datas), int(epochs), int(batch_size)
    if R < 1 or len(perms) != R or (old_values is not None and len(old_values) != R):
        raise ValueError("ppo_train_dist_ref: one data tuple, one list of orders (and one old_values) per rank")
    orders = [[np.asarray(o) for o in p] for p in perms]
    if any(len(p) != epochs for p in orders) or len({o.size for p in orders for o in p}) > 1:
        raise ValueError("ppo_train_dist_ref: the ranks' minibatch counts differ (T * N, batch_size and n_epochs must agree)")
    stats = []
    stop = False
    for e in range(epochs):
        for s in range(0, orders[0][e].size, bs):
            grads, rows = [], []
            for r in range(R):
                idx = orders[r][e][s:s + bs]
                obs, actions, old_lp, adv, ret = (np.asarray(a)[idx] for a in datas[r])
                if normalize_advantage:
                    adv = normalize_adv_ref(adv)
                g, st = ppo_grad_ref(params, obs, actions, old_lp, adv, ret, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef,
                                     old_values=None if old_values is None else np.asarray(old_values[r])[idx],
                                     clip_range_vf=clip_range_vf)
                grads.append(g)
                rows.append(st)
            grad, st = combine_ref(np.stack(grads), np.stack(rows))
            stats.append(st)
            stop = target_kl is not None and kl_stop_ref(st[3], target_kl)
            if stop:
                break
            params = _apply_ref(params, state, grad, lr, max_grad_norm, betas, eps)
        if stop:
            break
    return params, np.array(stats, _f32).reshape(-1, 5)


# ---- the device class --------------------------------------------------------------------------------
def _or_off(x):        # an optional option as the ABI takes it: negative is off
    return -1.0 if x is None else x


class DevicePPO(Handle):
    """The rule on the device: ``grad`` is ``ppo_grad_ref``, ``step`` is ``ppo_step_ref`` written into
    ``policy``'s device parameters in place (the next ``policy.act`` uses them), ``train`` is SB3's
    epoch / minibatch loop over a ``DeviceRolloutBuffer`` (``ppo_train_ref``).  ``train``, ``step`` and
    ``grad`` never synchronise the device; the statistics stay in device tensors.  The optimiser state
    (master parameters, gradient, Adam moments) belongs to this object; ``policy.set_params`` afterwards is
    picked up by the next call and leaves the moments as they are.  ``learning_rate`` is read at every
    step.  The library reads ``policy``'s handle in every call, so a call after ``policy.close()`` raises
    ``ValueError``.

    ``clip_range_vf`` and ``target_kl`` are SB3's options (None: off).  ``target_kl`` acts in ``train``
    and is decided on the device: after such a ``train`` the step count ``t``, ``n_applied`` and ``stopped``
    are read back (one ``mrp_ppo_progress``, which synchronises) when first asked for, and the next ``step``
    / ``train`` asks, because Adam's bias correction needs ``t``.  ``minibatch="device"`` gathers each
    minibatch and normalises its advantages (``normalize_adv_ref``) in HIP; ``"torch"`` (the default) is
    ``index_select`` and torch arithmetic.

    Data-parallel training (``combine_ref`` / ``ppo_train_dist_ref``): with ``shard`` (a ``dist.Shard`` of
    ``world > 1``) or an explicit ``exchange`` (a ``dist.GradExchange`` of ``n_params + 5`` floats) ``train``
    splits every minibatch in two: the local gradient before clipping and the local statistics go into
    ``exchange.mine``, the exchange gathers every rank's, and ``mrp_ppo_apply_device`` combines them in rank
    order and applies the clip, the ``target_kl`` decision and Adam, the same bits on every rank.  Call
    ``sync_from`` once before training so that the replicas start equal.  ``step`` and ``grad`` stay local."""

    _DESTROY, _LAST_ERROR, _VALUE_ERRORS = "mrp_ppo_destroy", "mrp_ppo_last_error", (-1, -3)

    def __init__(self, policy, learning_rate=3e-4, n_epochs=10, batch_size=64, clip_range=0.2, ent_coef=0.0, vf_coef=0.5,
                 max_grad_norm=0.5, normalize_advantage=True, betas=(0.9, 0.999), eps=1e-5, max_batch=None, clip_range_vf=None,
                 target_kl=None, minibatch="torch", shard=None, exchange=None):
        if minibatch not in ("torch", "device"):
            raise ValueError(f"DevicePPO: minibatch is {minibatch!r}, expected 'torch' or 'device'")
        if clip_range_vf is not None and not clip_range_vf >= 0:
            raise ValueError("DevicePPO: clip_range_vf must be None or >= 0")
        if target_kl is not None and not target_kl >= 0:
            raise ValueError("DevicePPO: target_kl must be None or >= 0")
        self.policy, self.learning_rate, self.n_epochs, self.batch_size = policy, learning_rate, int(n_epochs), int(batch_size)
        self.clip_range, self.ent_coef, self.vf_coef, self.max_grad_norm = clip_range, ent_coef, vf_coef, max_grad_norm
        self.normalize_advantage, self.betas, self.eps = bool(normalize_advantage), tuple(betas), eps
        self.clip_range_vf, self.target_kl, self.minibatch = clip_range_vf, target_kl, minibatch
        self.max_batch = int(self.batch_size if max_batch is None else max_batch)
        self._t, self._n_applied, self._stopped, self._pending, self._staged = 0, 0, False, False, None
        self._base, self._checked = 0, None      # t before a pending train; the (T * N, batch, epochs) the ranks last agreed on
        self.device = policy.device
        self._open("mrp_ppo_create", policy._h, self.max_batch)
        self.n_params = int(self._L.mrp_ppo_n_params(self._h))
        if exchange is None and shard is not None and shard.world > 1:
            from .dist import GradExchange
            exchange = GradExchange(shard, self.n_params + 5, self.device)
        if exchange is not None and exchange.n_floats < self.n_params + 5:
            raise ValueError(f"DevicePPO: the exchange holds {exchange.n_floats} floats, n_params + 5 is {self.n_params + 5}")
        self.exchange = exchange

    @property
    def _h(self):
        self.policy._h     # mrp_ppo reads the policy's handle in every call: ValueError once that is closed
        return super()._h

    # ---- the step count and the device's progress words
    def progress(self):
        """``(stopped, applied)`` of the device's progress words since the last ``train`` / ``step`` /
        ``grad`` began (``mrp_ppo_progress``: synchronises the stream).  ``ValueError`` if a gathered
        index lay outside the fields' rows."""
        stopped, applied = ctypes.c_int(), ctypes.c_int()
        self._check_rc(self._L.mrp_ppo_progress(self._h, stream_of(self.device), ctypes.byref(stopped), ctypes.byref(applied)))
        return bool(stopped.value), int(applied.value)

    def _resolve(self):
        if self._pending:
            self._pending = False         # cleared first: a bad index raises once and leaves t at its base
            self._stopped, self._n_applied = self.progress()
            self._t = self._base + self._n_applied

    @property
    def t(self):
        """Optimiser steps applied so far (Adam's step count)."""
        self._resolve()
        return self._t

    @t.setter
    def t(self, value):
        self._resolve()
        self._t = int(value)

    @property
    def n_applied(self):
        """Steps the last ``train`` applied."""
        self._resolve()
        return self._n_applied

    @property
    def stopped(self):
        """Whether the last ``train`` ended at ``target_kl``."""
        self._resolve()
        return self._stopped

    # ---- one minibatch
    def _batch(self, obs, actions, old_log_probs, advantages, returns, old_values=None, index=None):
        import torch
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError("DevicePPO: obs must be a [B, obs_dim] CUDA tensor")
        rows, f32 = int(obs.shape[0]), torch.float32
        if index is None:
            B = rows
        else:
            if not isinstance(index, torch.Tensor) or index.dim() != 1:
                raise ValueError("DevicePPO: index must be a 1-d int64 CUDA tensor")
            B = int(index.shape[0])
            check_tensor("DevicePPO", "index", index, self.device, torch.int64, (B,))
        if B < 1 or rows < 1:
            raise ValueError("DevicePPO: the minibatch holds no sample")
        if self.clip_range_vf is not None and old_values is None:
            raise ValueError("DevicePPO: clip_range_vf is set and old_values is missing")
        # a missing field passes here and is the library's "null pointer"
        named = (("obs", obs, f32, (rows, self.policy.obs_dim), True), ("actions", actions, f32, (rows, self.policy.act_dim), True),
                 ("old_values", old_values, f32, (rows,), True), ("old_log_probs", old_log_probs, f32, (rows,), True),
                 ("advantages", advantages, f32, (rows,), True), ("returns", returns, f32, (rows,), True))
        check_tensors("DevicePPO", self.device, named)
        if B > self.max_batch:
            raise ValueError(f"DevicePPO: a minibatch of {B} samples, max_batch is {self.max_batch}")
        return B, rows, [ptr(spec[1]) for spec in named]

    def _out(self, name, t, n):
        import torch
        if t is None:
            return torch.empty(n, dtype=torch.float32, device=self.device)
        check_tensor("DevicePPO", name, t, self.device, torch.float32, (n,))
        return t

    def _begin(self):
        self._resolve()
        self._check_rc(self._L.mrp_ppo_begin_device(self._h, stream_of(self.device)))

    def _adam(self, t):
        return [ctypes.c_float(float(x)) for x in adam_scalars(t, self.learning_rate, self.betas, self.eps)]

    def _call(self, predicated, stream, B, index, rows, ptrs, normalize, target_kl, t, grad, stats):
        """One minibatch on checked pointers: the gradient alone into ``grad``, or with ``grad`` None the
        optimiser step that Adam counts as ``t``.  ``predicated``: ``mrp_ppo_minibatch_device`` under the progress
        words (after ``_begin``); else ``mrp_ppo_step_device`` / ``mrp_ppo_grad_device``, which have no index, no
        normalisation, no ``old_values`` and no ``target_kl``."""
        f, d, L = ctypes.c_float, ctypes.c_double, self._L
        if predicated:
            self._check_rc(L.mrp_ppo_minibatch_device(
                self._h, stream, B, index, rows, *ptrs, 1 if normalize else 0, f(self.clip_range), f(_or_off(self.clip_range_vf)),
                d(_or_off(target_kl)), f(self.ent_coef), d(self.vf_coef), d(self.max_grad_norm), *self._adam(t), grad, stats))
            if index is not None or (normalize and B > 1):
                self._staged = B
            return
        head = (self._h, stream, B, *ptrs[:2], *ptrs[3:], f(self.clip_range), f(self.ent_coef), d(self.vf_coef))
        if grad is not None:
            self._check_rc(L.mrp_ppo_grad_device(*head, grad, stats))
        else:
            self._check_rc(L.mrp_ppo_step_device(*head, d(self.max_grad_norm), *self._adam(t), stats))

    def _single(self, fields, old_values, index, normalize, out, stats_out, want_grad):
        """``grad`` and ``step``: one checked minibatch through the unpredicated entry, or with any of
        ``old_values``, ``index``, ``normalize`` and ``clip_range_vf`` through the predicated one."""
        B, rows, ptrs = self._batch(*fields, old_values, index)
        g = self._out("out", out, self.n_params) if want_grad else None
        st = self._out("stats_out", stats_out, 5)
        predicated = old_values is not None or index is not None or normalize or self.clip_range_vf is not None
        if predicated:
            self._begin()
        self._call(predicated, stream_of(self.device), B, ptr(index), rows, ptrs, normalize, None, 1 if want_grad else self.t + 1,
                   ptr(g), ptr(st))
        if not want_grad:
            self._t += 1
        return g, st

    def _finish(self, t0, n, target_kl):
        """The bookkeeping after ``n`` enqueued minibatches from step count ``t0``: all applied without
        ``target_kl``, else the device's progress words decide (``_resolve``)."""
        if target_kl is None:
            self._t, self._n_applied, self._stopped = t0 + n, n, False
        else:
            self._base, self._pending = t0, True

    def grad(self, obs, actions, old_log_probs, advantages, returns, out=None, stats_out=None, *, old_values=None, index=None,
             normalize=False):
        """``ppo_grad_ref`` on the device: returns ``(flat_grad [n_params], stats [5])`` device
        tensors (``out`` / ``stats_out`` when given).  Parameters and optimiser state are not changed.
        An output whose memory overlaps an input's or the other output's anywhere raises ``ValueError``.

        ``old_values`` [B] is read under ``clip_range_vf``.  With ``index`` (int64 [B]) the fields hold any
        number of rows and the minibatch is rows ``index`` of them, gathered on the device; ``normalize``
        passes the advantages through ``normalize_adv_ref`` on the device first."""
        return self._single((obs, actions, old_log_probs, advantages, returns), old_values, index, normalize, out, stats_out, True)

    def step(self, obs, actions, old_log_probs, advantages, returns, stats_out=None, *, old_values=None, index=None,
             normalize=False):
        """One optimiser step (``ppo_step_ref``) in place; returns the ``stats [5]`` device tensor.
        ``old_values``, ``index`` and ``normalize`` as in ``grad``.  ``target_kl`` belongs to ``train``:
        a ``step`` is always applied."""
        return self._single((obs, actions, old_log_probs, advantages, returns), old_values, index, normalize, None, stats_out, False)[1]

    def train(self, buffer, generator=None, poll=False):
        """``n_epochs`` passes over the buffer's shuffled minibatches (``buffer.get``'s ``randperm`` and
        flat order), one optimiser step each (``ppo_train_ref``); returns the ``[n_updates, 5]`` device
        tensor of statistics and never synchronises.

        With ``minibatch="torch"`` the minibatches are ``buffer.get``'s and ``normalize_advantage`` is
        SB3's ``(adv - adv.mean()) / (adv.std() + 1e-8)`` as torch operations (unbiased std, skipped for
        one sample): outside the bitwise rule.  With ``"device"`` gather and ``normalize_adv_ref`` run in
        HIP, one library call per minibatch.  With ``target_kl`` every minibatch is still enqueued; those
        from the stopping one on do nothing on the device and their statistics rows stay zero.
        ``poll=True`` reads ``stopped`` after each epoch (a synchronisation) and stops enqueueing: the
        results are the same.

        With an exchange (data-parallel training) every minibatch is the local phase into
        ``exchange.mine``, the exchange, and ``mrp_ppo_apply_device`` (``ppo_train_dist_ref``), in either
        gather mode.  Every rank must pass the same ``T * N``, ``batch_size`` and ``n_epochs``: they are
        compared across ranks (one ``dist.agree``, only when they differ from the last ones
        compared) and a mismatch raises ``ValueError`` on every rank before anything is enqueued."""
        import torch
        total, bs = buffer.n_steps * buffer.n_lanes, self.batch_size
        stats = torch.zeros(self.n_epochs * -(-total // bs), 5, dtype=torch.float32, device=self.device)
        ex, kl, use_v, gather = self.exchange, self.target_kl, self.clip_range_vf is not None, self.minibatch == "device"
        if ex is not None:
            self._check_ranks(total)
        # without an option, an exchange or the device gather a minibatch is one unpredicated mrp_ppo_step_device
        predicated = ex is not None or gather or use_v or kl is not None
        if predicated:
            self._begin()
        t0, stream, u = self.t, stream_of(self.device), 0
        if ex is None:
            def run(B, index, rows, ptrs, normalize):
                self._call(predicated, stream, B, index, rows, ptrs, normalize, kl, t0 + u + 1, None, stats[u].data_ptr())
        else:
            # the local phase writes the gradient before clipping and the statistics side by side into exchange.mine
            P = self.n_params
            local_g, local_s = ex.mine[:P].data_ptr(), ex.mine[P:P + 5].data_ptr()

            def run(B, index, rows, ptrs, normalize):
                self._call(True, stream, B, index, rows, ptrs, normalize, None, 1, local_g, local_s)
                self._apply(stream, ex(), kl, t0 + u + 1, stats[u].data_ptr())
        if gather:
            obs, actions, values, old_lp, adv, ret = buffer.flat_fields()
            _, rows, ptrs = self._batch(obs.reshape(total, -1), actions, old_lp, adv, ret, values if use_v else None,
                                        index=torch.zeros(1, dtype=torch.int64, device=self.device))

        def minibatches():
            """One epoch's ``(B, index, rows, ptrs, normalize)``: slices of ``flat_index`` over the flat fields, or
            ``buffer.get``'s gathered minibatches with torch's normalisation."""
            if gather:
                flat = buffer.flat_index(generator)
                for start in range(0, total, bs):
                    idx = flat[start:start + bs]
                    if idx.shape[0] > self.max_batch:
                        raise ValueError(f"DevicePPO: a minibatch of {idx.shape[0]} samples, max_batch is {self.max_batch}")
                    yield int(idx.shape[0]), idx.data_ptr(), rows, ptrs, self.normalize_advantage
            else:
                for obs, actions, values, old_lp, adv, ret in buffer.get(bs, generator):
                    if self.normalize_advantage and adv.numel() > 1:
                        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
                    B, n, p = self._batch(obs.reshape(obs.shape[0], -1), actions, old_lp, adv, ret, values if use_v else None)
                    yield B, None, n, p, False
        for _ in range(self.n_epochs):
            for mb in minibatches():
                run(*mb)
                u += 1
            if poll and kl is not None and self.progress()[0]:
                break
        self._finish(t0, u, kl)
        return stats

    # ---- data-parallel training
    def _check_ranks(self, total):
        """Every rank must enqueue the same number of minibatches: ``dist.agree`` on ``(T * N, batch_size,
        n_epochs)``, repeated only when the triple changes."""
        triple = (int(total), self.batch_size, self.n_epochs)
        if triple != self._checked:
            agree("DevicePPO.train", "(T * N, batch_size, n_epochs)", triple, self.exchange.world, self.exchange.group)
            self._checked = triple

    def _apply(self, stream, parts, target_kl, t, stats):
        """One ``mrp_ppo_apply_device`` on a checked ``[R, stride]`` tensor; ``t`` is the step this would be."""
        d = ctypes.c_double
        self._check_rc(self._L.mrp_ppo_apply_device(self._h, stream, int(parts.shape[0]), parts.data_ptr(), int(parts.shape[1]),
                                                    d(_or_off(target_kl)), d(self.max_grad_norm), *self._adam(t), stats))

    def apply(self, parts, stats_out=None):
        """The apply phase alone (``combine_ref``, then ``kl_stop_ref`` and ``adam_ref`` on the combined
        values) on ``parts``, a float32 ``[R, stride]`` device tensor whose row ``r`` holds rank ``r``'s flat
        gradient before clipping in its first ``n_params`` floats and its five statistics behind them
        (``stride >= n_params + 5``, ``R`` in 1..64).  Returns the combined ``stats [5]`` device tensor
        (``stats_out`` when given, which may not overlap ``parts``).  Never synchronises.  With
        ``target_kl`` the decision is the device's: ``t``, ``n_applied`` and ``stopped`` resolve as after
        ``train``, and a stopped call leaves ``stats_out`` as it was."""
        import torch
        if not isinstance(parts, torch.Tensor) or parts.dim() != 2:
            raise ValueError("DevicePPO.apply: parts must be a [R, stride] CUDA tensor")
        check_tensor("DevicePPO", "parts", parts, self.device, torch.float32, tuple(parts.shape))
        st = self._out("stats_out", stats_out, 5)
        self._begin()
        t0 = self._t
        self._apply(stream_of(self.device), parts, self.target_kl, t0 + 1, ptr(st))
        self._finish(t0, 1, self.target_kl)
        return st

    def set_state(self, m, v, t):
        """Load Adam's moments (flat float32 ``[n_params]`` host arrays) and the step count: the inverse
        of ``state()`` and ``t`` (synchronises the device)."""
        m, v = (np.ascontiguousarray(a, _f32).reshape(-1) for a in (m, v))
        if m.size != self.n_params or v.size != self.n_params:
            raise ValueError(f"DevicePPO.set_state: m and v hold {self.n_params} floats each")
        self._resolve()
        self._check_rc(self._L.mrp_ppo_set_state(self._h, m.ctypes.data, v.ctypes.data))
        self._t = int(t)

    def sync_from(self, src=0, group=None):
        """Broadcast rank ``src``'s flat parameters, ``std``, ``m``, ``v`` and ``t`` and load them on every
        rank, so that the replicas start equal (synchronises; every rank's policy must hold parameters of
        the one architecture already).  The tensors travel on the device under an nccl group and on the
        host otherwise."""
        like = self.policy.get_params()
        m, v = self.state()
        P, A = self.n_params, self.policy.act_dim
        mine, step = np.concatenate([flatten_params(like), like.std, m, v]).astype(_f32), np.array([self.t], np.int64)
        a = broadcast_array(mine, src, group, self.device)
        step = broadcast_array(step, src, group, self.device)       # an int64 of its own: float32 holds 24 bits
        self.policy.set_params(unflatten_params(like, a[:P], std=a[P:P + A].copy()))
        self.set_state(a[P + A:2 * P + A], a[2 * P + A:], int(step[0]))

    def staged(self):
        """Host copies of the staging buffers as the last gathered or device-normalised minibatch left
        them: a dict of ``obs``, ``actions``, ``old_values`` (under ``clip_range_vf``), ``old_log_probs``,
        ``advantages``, ``returns`` (synchronises the device).  For tests."""
        if self._staged is None:
            raise ValueError("DevicePPO.staged: no minibatch has been staged")
        B = self._staged
        out = {"obs": np.zeros((B, self.policy.obs_dim), _f32), "actions": np.zeros((B, self.policy.act_dim), _f32),
               "old_values": np.zeros(B, _f32) if self.clip_range_vf is not None else None, "old_log_probs": np.zeros(B, _f32),
               "advantages": np.zeros(B, _f32), "returns": np.zeros(B, _f32)}
        self._check_rc(self._L.mrp_ppo_get_staged(self._h, B, *[None if a is None else a.ctypes.data for a in out.values()]))
        return {k: a for k, a in out.items() if a is not None}

    def state(self):
        """``(m, v)``: host copies of Adam's moments, flat float32 (synchronises the device)."""
        m, v = np.zeros(self.n_params, _f32), np.zeros(self.n_params, _f32)
        self._check_rc(self._L.mrp_ppo_get_state(self._h, m.ctypes.data, v.ctypes.data))
        return m, v
