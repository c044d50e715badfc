"""Device policy: stable-baselines3's ``ActorCriticPolicy`` with ``MlpExtractor`` -- forward pass,
diagonal-Gaussian sampling, log-prob, value and action clipping -- for every lane in one HIP launch
(``k_policy`` in ``csrc/mrp_policy.hip``, ``mrp_policy_*`` in ``include/mrp.h``).

``policy_ref`` is the numpy statement of the rule and the definition the kernel matches bit for bit:

* architecture: ``S`` shared trunk layers, then ``P`` policy-tower and ``V`` value-tower layers, each
  ``Linear + activation`` (``tanh`` or ``relu``), a linear action head, a linear value head and a
  state-independent ``log_std``.  ``S + max(P, V) <= 4``, widths and ``obs_dim`` 1..256, ``act_dim``
  1..16; ``S = P = V = 0`` puts the heads straight on the observation;
* linear layer: ``y[j] = fma(x[K-1], W[j][K-1], ... fma(x[0], W[j][0], b[j]))``, a float32 fused
  multiply-add chain in ascending ``k`` from the bias (``fma32`` restates the fma exactly);
* ``tanh_ref``: this build's float32 tanh (``csrc/mrp_math.h`` ``tanh_f32``), operation for operation;
  ``relu`` is ``x if x > 0 else +0``;
* distribution: ``action = mean + std * eps`` (``mean`` when deterministic), ``clipped = clip(action,
  -1, 1)``, ``log_prob = sum_i((-(d_i * d_i)) / (2 * (std_i * std_i)) - log_std_i - float32(log(sqrt(2
  pi))))`` with ``d = action - mean`` and ``std = float32(exp(float64(log_std)))``: float32 operations
  in this order, the sum ascending from +0.

stable-baselines3 is not installed where this was written, so parity with SB3 itself is unpinned (as
for ``rollout.gae_ref``): the rule is this restatement.  The module is pure numpy at import;
``DevicePolicy`` imports torch when used.
"""
from __future__ import annotations

import ctypes
import math
import re

import numpy as np

from ._device import Handle, check_tensor, index_of, ptr, stream_of

MAX_WIDTH, MAX_ACT, MAX_DEPTH = 256, 16, 4
ACTIVATIONS = {"tanh": 0, "relu": 1}        # include/mrp.h MRP_POLICY_TANH / MRP_POLICY_RELU
LOG_SQRT_2PI = np.float32(0.9189385332046727)
_f32, _f64 = np.float32, np.float64


# ---- the exact float32 fma ---------------------------------------------------------------------------
def fma32(a, b, c):
    """``fmaf(a, b, c)`` on float32 arrays, exactly: the float64 product of two float32 is exact; the
    sum with ``c`` is taken with TwoSum and rounded to odd when it is inexact, so that the final
    rounding to float32 sees on which side of a midpoint the true value lies (53 >= 2 * 24 + 2).  A
    plain float64 multiply-add followed by the cast rounds twice and is not an fma."""
    a, b, c = (np.asarray(v, _f32).astype(_f64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = np.ascontiguousarray(s).view(np.int64)
        fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        away = (err > 0) == (s > 0)          # the true sum lies further from zero than s
        bits = np.where(fix, bits + np.where(away, 1, -1), bits)
        return bits.view(_f64).astype(_f32)


def linear_ref(x, w, b):
    """float32 [N, K] @ [out, K].T + b as the fma chain of the rule; returns float32 [N, out]."""
    x, w = np.asarray(x, _f32), np.asarray(w, _f32)
    acc = np.broadcast_to(np.asarray(b, _f32), (x.shape[0], w.shape[0])).copy()
    for k in range(w.shape[1]):
        acc = fma32(x[:, k:k + 1], w[None, :, k], acc)
    return acc


# ---- tanh --------------------------------------------------------------------------------------------
_INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
_LN2_HI = float.fromhex("0x1.62e42feep-1")
_LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
_TANH_C = [1.0 / math.factorial(k) for k in range(12)]
# where tanh_f32 changes branch: n steps at |x| = (m + 1/2) ln2 / 2, and |x| >= 20 saturates
TANH_BRANCH_POINTS = tuple((m + 0.5) * math.log(2.0) / 2 for m in range(58)) + (20.0,)


def tanh_ref(x):
    """``tanh_f32`` of ``csrc/mrp_math.h`` on a float32 array, operation for operation (float64
    arithmetic rounded per operation, one rounding to float32; see the comment there)."""
    x = np.ascontiguousarray(x, _f32)
    ux = x.view(np.uint32)
    ax = ux & np.uint32(0x7FFFFFFF)
    nan = ax > np.uint32(0x7F800000)
    xa = ax.view(_f32)
    sat = ~(xa < _f32(20.0))
    with np.errstate(all="ignore"):
        y = -2.0 * np.where(sat, _f32(20.0), xa).astype(_f64)
        n = np.trunc(y * _INV_LN2 - 0.5).astype(np.int64)
        dn = n.astype(_f64)
        r = (y - dn * _LN2_HI) - dn * _LN2_LO
        q = np.full_like(r, _TANH_C[11])
        for k in range(10, 1, -1):
            q = q * r + _TANH_C[k]
        p = r + (r * r) * q
        E = ((1023 + n) << 52).view(_f64) * (1.0 + p)
        num = np.where(n == 0, -p, 1.0 - E)
        den = np.where(n == 0, 2.0 + p, 1.0 + E)
        r0 = (_f32(1.0) / den.astype(_f32)).astype(_f64)
        r1 = r0 * (2.0 - den * r0)
        r2 = r1 * (2.0 - den * r1)
        t = np.where(sat, _f32(1.0), (num * r2).astype(_f32)).astype(_f32)
    out = (t.view(np.uint32) & np.uint32(0x7FFFFFFF)) | (ux & np.uint32(0x80000000))
    return np.where(nan, ux, out).astype(np.uint32).view(_f32)


def _activate(x, activation):
    # relu is `x > 0 ? x : +0` (mrp_math.h fmax_): -0 and NaN give +0
    return tanh_ref(x) if activation == "tanh" else np.where(x > 0, x, _f32(0.0)).astype(_f32)


# ---- parameters --------------------------------------------------------------------------------------
class PolicyParams:
    """The arrays of one policy, float32 in torch's ``[out, in]`` layout: ``shared`` / ``pi`` / ``vf``
    are lists of ``(weight, bias)``, ``action`` and ``value`` the heads' ``(weight, bias)``.  Raises
    ``ValueError`` for shapes that do not chain or lie outside the limits.  ``std`` is
    ``float32(exp(float64(log_std)))`` unless given: parameters exported from the device after a PPO
    step carry the device's ``std`` bits (``ppo.exp_ref``)."""

    def __init__(self, shared, pi, vf, action, value, log_std, activation="tanh", std=None):
        f = lambda wb: (np.ascontiguousarray(wb[0], _f32), np.ascontiguousarray(wb[1], _f32))  # noqa: E731
        self.shared, self.pi, self.vf = [f(x) for x in shared], [f(x) for x in pi], [f(x) for x in vf]
        self.action, self.value = f(action), f(value)
        self.log_std = np.ascontiguousarray(log_std, _f32).reshape(-1)
        self.activation = activation
        if activation not in ACTIVATIONS:
            raise ValueError(f"policy: activation {activation!r} is neither 'tanh' nor 'relu'")
        for w, b in self.shared + self.pi + self.vf + [self.action, self.value]:
            if w.ndim != 2 or b.shape != (w.shape[0],):
                raise ValueError(f"policy: a layer has weight {w.shape} and bias {b.shape}")
        first = (self.shared + self.pi + [self.action])[0][0]
        self.obs_dim, self.act_dim = int(first.shape[1]), int(self.action[0].shape[0])

        def chain(layers, k, what):
            for w, _ in layers:
                if w.shape[1] != k:
                    raise ValueError(f"policy: {what} layer takes {w.shape[1]} inputs, the layer before it gives {k}")
                k = w.shape[0]
            return k
        kt = chain(self.shared, self.obs_dim, "a trunk")
        kp, kv = chain(self.pi, kt, "a policy-tower"), chain(self.vf, kt, "a value-tower")
        chain([self.action], kp, "the action head's")
        chain([self.value], kv, "the value head's")
        if self.value[0].shape[0] != 1:
            raise ValueError(f"policy: the value head has {self.value[0].shape[0]} outputs, expected 1")
        if self.log_std.shape != (self.act_dim,):
            raise ValueError(f"policy: log_std is {self.log_std.shape}, expected ({self.act_dim},)")
        check_arch(self.obs_dim, self.act_dim, len(self.shared), len(self.pi), len(self.vf), self.widths)
        self.std = np.exp(self.log_std.astype(_f64)).astype(_f32)
        if std is not None:
            self.std = np.ascontiguousarray(std, _f32).reshape(-1).copy()
            if self.std.shape != (self.act_dim,):
                raise ValueError(f"policy: std is {self.std.shape}, expected ({self.act_dim},)")

    @property
    def widths(self):
        return [int(w.shape[0]) for w, _ in self.shared + self.pi + self.vf]


def check_arch(obs_dim, act_dim, n_shared, n_pi, n_vf, widths):
    """The limits of the rule (and of ``mrp_policy_create``); ``ValueError`` outside them."""
    if not 1 <= obs_dim <= MAX_WIDTH:
        raise ValueError(f"policy: obs_dim {obs_dim} outside 1..{MAX_WIDTH}")
    if not 1 <= act_dim <= MAX_ACT:
        raise ValueError(f"policy: act_dim {act_dim} outside 1..{MAX_ACT}")
    if min(n_shared, n_pi, n_vf) < 0 or n_shared + max(n_pi, n_vf) > MAX_DEPTH:
        raise ValueError(f"policy: {n_shared} shared + max({n_pi}, {n_vf}) tower layers, at most {MAX_DEPTH} in a row")
    if len(widths) != n_shared + n_pi + n_vf:
        raise ValueError(f"policy: {len(widths)} widths for {n_shared + n_pi + n_vf} layers")
    for w in widths:
        if not 1 <= w <= MAX_WIDTH:
            raise ValueError(f"policy: layer width {w} outside 1..{MAX_WIDTH}")


def random_params(obs_dim, act_dim, shared, pi, vf, activation, seed, bias_scale, log_std, negzero_bias=False):
    """A synthetic network for tests and benches: towers of the widths ``shared`` / ``pi`` / ``vf``, drawn
    from ``np.random.default_rng(seed)`` layer by layer (trunk, policy tower, value tower, action head,
    value head), per layer the weights ``N(0, 1 / in)`` and then the bias ``N(0, bias_scale^2)``.
    ``negzero_bias`` makes every weight negative and every bias -0: a row of +0 then gives products of
    -0, which leave a bias of -0 alone."""
    rng = np.random.default_rng(seed)

    def lin(k, n):
        w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(_f32)
        b = (rng.standard_normal(n) * bias_scale).astype(_f32)
        if negzero_bias:
            w, b = -np.abs(w), np.full(n, -0.0, _f32)
        return w, b

    def tower(k, widths):
        out = []
        for n in widths:
            out.append(lin(k, n))
            k = n
        return out, k
    s, kt = tower(obs_dim, shared)
    p, kp = tower(kt, pi)
    v, kv = tower(kt, vf)
    return PolicyParams(s, p, v, lin(kp, act_dim), lin(kv, 1), log_std, activation)


def params_from_state_dict(sd, activation="tanh"):
    """``PolicyParams`` from an SB3 ``ActorCriticPolicy`` ``state_dict`` (torch tensors or arrays):
    ``mlp_extractor.{shared_net,policy_net,value_net}.N.{weight,bias}`` in ascending ``N``,
    ``action_net.*``, ``value_net.*`` and ``log_std``; the layer counts, widths and dims follow from
    the shapes."""
    arr = lambda t: np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, _f32)  # noqa: E731

    def tower(name):
        pat = re.compile(r"^mlp_extractor\." + name + r"\.(\d+)\.weight$")
        idx = sorted(int(m.group(1)) for m in map(pat.match, sd) if m)
        return [(arr(sd[f"mlp_extractor.{name}.{i}.weight"]), arr(sd[f"mlp_extractor.{name}.{i}.bias"])) for i in idx]
    for key in ("action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias", "log_std"):
        if key not in sd:
            raise ValueError(f"policy: the state_dict has no {key!r}")
    return PolicyParams(tower("shared_net"), tower("policy_net"), tower("value_net"),
                        (arr(sd["action_net.weight"]), arr(sd["action_net.bias"])),
                        (arr(sd["value_net.weight"]), arr(sd["value_net.bias"])), arr(sd["log_std"]), activation)


# ---- the rule ----------------------------------------------------------------------------------------
def features_ref(params, obs, which):
    """The input of the action head (``which="pi"``) or of the value head (``"vf"``), float32 [N, K]."""
    x = np.ascontiguousarray(obs, _f32)
    for w, b in params.shared + (params.pi if which == "pi" else params.vf):
        x = _activate(linear_ref(x, w, b), params.activation)
    return x


def values_ref(params, obs):
    """The value output alone (trunk, value tower, value head): float32 [N]."""
    return linear_ref(features_ref(params, obs, "vf"), *params.value)[:, 0]


def policy_ref(params, obs, eps=None, deterministic=False):
    """The rule of the module docstring on float32 ``obs`` [N, obs_dim] and noise ``eps`` [N, act_dim]
    (unused when ``deterministic``).  Returns ``(actions, clipped, values, log_probs)``, float32
    [N, A], [N, A], [N], [N]; ``actions`` are the unclipped samples SB3 stores, ``clipped`` what steps
    the env.  Parity with SB3 itself is unpinned (see the module docstring)."""
    mean = linear_ref(features_ref(params, obs, "pi"), *params.action)
    values = values_ref(params, obs)
    std, log_std = params.std[None, :], params.log_std[None, :]
    if deterministic:
        actions = mean.copy()
    else:
        actions = mean + std * np.ascontiguousarray(eps, _f32).reshape(mean.shape)
    lo = np.where(actions > _f32(-1.0), actions, _f32(-1.0))           # fmax_(a, -1), then fmin_(., 1)
    clipped = np.where(lo < _f32(1.0), lo, _f32(1.0))
    d = actions - mean
    terms = ((-(d * d)) / (_f32(2.0) * (std * std)) - log_std) - LOG_SQRT_2PI
    log_probs = np.zeros(mean.shape[0], _f32)
    for i in range(mean.shape[1]):
        log_probs = log_probs + terms[:, i]
    return actions.astype(_f32), clipped.astype(_f32), values, log_probs


# ---- flat parameter order ----------------------------------------------------------------------------
def _layers(params):
    return params.shared + params.pi + params.vf + [params.action, params.value]


def flatten_params(params):
    """The flat float32 vector of SB3's ``parameters()`` order: ``log_std``, then every layer's
    ``weight`` (row-major ``[out][in]``) and ``bias`` -- trunk, policy tower, value tower, heads."""
    parts = [params.log_std]
    for w, b in _layers(params):
        parts += [w.ravel(), b]
    return np.concatenate(parts).astype(_f32)


def unflatten_params(like, flat, std=None):
    """``PolicyParams`` of ``like``'s architecture from a flat vector (``std``: see ``PolicyParams``)."""
    flat = np.ascontiguousarray(flat, _f32)
    pos = [like.act_dim]

    def take(shape):
        n = int(np.prod(shape))
        out = flat[pos[0]:pos[0] + n].reshape(shape).copy()
        pos[0] += n
        return out
    layers = [(take(w.shape), take(b.shape)) for w, b in _layers(like)]
    S, Pn = len(like.shared), len(like.pi)
    nl = S + Pn + len(like.vf)
    return PolicyParams(layers[:S], layers[S:S + Pn], layers[S + Pn:nl], layers[nl], layers[nl + 1],
                        flat[:like.act_dim].copy(), like.activation, std=std)


def state_dict_from_params(params):
    """Arrays under SB3's parameter names: the inverse of ``params_from_state_dict``."""
    sd = {"log_std": params.log_std.copy()}
    for name, tower in (("shared_net", params.shared), ("policy_net", params.pi), ("value_net", params.vf)):
        for i, (w, b) in enumerate(tower):     # Linear modules sit at the even indices, activations between them
            sd[f"mlp_extractor.{name}.{2 * i}.weight"], sd[f"mlp_extractor.{name}.{2 * i}.bias"] = w.copy(), b.copy()
    for name, (w, b) in (("action_net", params.action), ("value_net", params.value)):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = w.copy(), b.copy()
    return sd


# ---- the device class --------------------------------------------------------------------------------
class DevicePolicy(Handle):
    """``policy_ref`` on the device, one launch per ``act`` / ``values`` call, bit for bit.

    ``from_state_dict`` loads an SB3 ``state_dict``, ``from_arrays`` plain numpy arrays; ``DevicePolicy(
    obs_dim, act_dim, n_shared, n_pi, n_vf, widths)`` alone creates a policy without parameters
    (``set_params`` loads them; ``act`` before that raises ``ValueError``).  The device counter RNG is
    keyed by ``(seed, lane_offset + lane, counter)``; ``counter`` advances with every sampling ``act``
    that draws its own noise."""

    _DESTROY, _LAST_ERROR, _VALUE_ERRORS = "mrp_policy_destroy", "mrp_policy_last_error", (-1, -3)

    def __init__(self, obs_dim, act_dim, n_shared, n_pi, n_vf, widths, activation="tanh", device=0, seed=0, lane_offset=0):
        import torch
        widths = [int(w) for w in widths]
        if activation not in ACTIVATIONS:
            raise ValueError(f"policy: activation {activation!r} is neither 'tanh' nor 'relu'")
        check_arch(obs_dim, act_dim, n_shared, n_pi, n_vf, widths)
        self.obs_dim, self.act_dim, self.arch, self.widths = int(obs_dim), int(act_dim), (n_shared, n_pi, n_vf), widths
        self.activation = activation
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        self.seed, self.lane_offset, self.counter = int(seed), int(lane_offset), 0
        self.params = None
        warr = (ctypes.c_int * max(1, len(widths)))(*widths)
        self._open("mrp_policy_create", index_of(self.device), self.obs_dim, self.act_dim, n_shared, n_pi, n_vf, warr,
                   ACTIVATIONS[activation])
        self.n_params = int(self._L.mrp_policy_n_params(self._h))

    @classmethod
    def from_params(cls, params, device=0, seed=0, lane_offset=0):
        p = cls(params.obs_dim, params.act_dim, len(params.shared), len(params.pi), len(params.vf), params.widths,
                params.activation, device, seed, lane_offset)
        p.set_params(params)
        return p

    @classmethod
    def from_state_dict(cls, sd, activation="tanh", device=0, seed=0, lane_offset=0):
        """From an SB3 ``ActorCriticPolicy.state_dict()`` (see ``params_from_state_dict``)."""
        return cls.from_params(params_from_state_dict(sd, activation), device, seed, lane_offset)

    @classmethod
    def from_arrays(cls, shared, pi, vf, action, value, log_std, activation="tanh", device=0, seed=0, lane_offset=0):
        """From numpy arrays in torch's ``[out, in]`` layout: lists of ``(weight, bias)`` per tower and
        the two heads' ``(weight, bias)`` (see ``PolicyParams``)."""
        return cls.from_params(PolicyParams(shared, pi, vf, action, value, log_std, activation), device, seed, lane_offset)

    def set_params(self, params) -> None:
        """Load a ``PolicyParams`` of this policy's architecture (synchronises the device)."""
        if ((params.obs_dim, params.act_dim, (len(params.shared), len(params.pi), len(params.vf)), params.widths, params.activation)
                != (self.obs_dim, self.act_dim, tuple(self.arch), self.widths, self.activation)):
            raise ValueError("DevicePolicy.set_params: the parameters belong to another architecture")
        flat = flatten_params(params)
        self._check_rc(self._L.mrp_policy_set_params(self._h, flat.ctypes.data, params.std.ctypes.data))
        self.params = params

    def get_params(self):
        """The device's parameters as a ``PolicyParams`` (``std`` included), e.g. after ``DevicePPO``
        steps: the inverse of ``set_params`` (synchronises the device)."""
        if self.params is None:
            raise ValueError("DevicePolicy.get_params: no parameters yet (set_params)")
        flat, std = np.zeros(self.n_params, _f32), np.zeros(self.act_dim, _f32)
        self._check_rc(self._L.mrp_policy_get_params(self._h, flat.ctypes.data, std.ctypes.data))
        return unflatten_params(self.params, flat, std=std)

    def state_dict(self):
        """The device's parameters as arrays under SB3's names: the inverse of ``params_from_state_dict``."""
        return state_dict_from_params(self.get_params())

    def _obs(self, obs):
        import torch
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError("DevicePolicy: obs must be a [N, obs_dim] CUDA tensor")
        check_tensor("DevicePolicy", "obs", obs, self.device, torch.float32, (obs.shape[0], self.obs_dim))
        if obs.shape[0] < 1:
            raise ValueError("DevicePolicy: obs holds no lane")
        return int(obs.shape[0])

    def act(self, obs, eps=None, deterministic=False, out=None, eps_out=None):
        """One launch on the current torch stream: float32 [N, obs_dim] ``obs``; ``eps`` float32
        [N, act_dim] noise (e.g. ``torch.randn``) or None for the device counter RNG, whose counter
        then advances; ``out``: an optional ``(actions, clipped, values, log_probs)`` tuple of
        preallocated tensors, returned as they are; ``eps_out`` optionally receives the noise used.
        An output whose memory overlaps an input's or another output's anywhere raises ``ValueError``.
        Returns ``(actions [N, A], clipped [N, A], values [N], log_probs [N])``."""
        import torch
        N, A, f32 = self._obs(obs), self.act_dim, torch.float32
        if out is None:
            new = lambda *s: torch.empty(s, dtype=f32, device=self.device)  # noqa: E731
            out = (new(N, A), new(N, A), new(N), new(N))
        if len(out) != 4:
            raise ValueError("DevicePolicy.act: out is (actions, clipped, values, log_probs)")
        named = list(zip(("actions", "clipped", "values", "log_probs"), out, ((N, A), (N, A), (N,), (N,))))
        named += [("eps", eps, (N, A)), ("eps_out", eps_out, (N, A))]
        for name, t, shape in named:
            if t is not None:
                check_tensor("DevicePolicy", name, t, self.device, f32, shape)
        self._check_rc(self._L.mrp_policy_act_device(self._h, stream_of(self.device), N, ptr(obs), ptr(eps), self.seed,
                                                     self.lane_offset, self.counter, int(bool(deterministic)), ptr(out[0]),
                                                     ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(eps_out)))
        if eps is None and not deterministic:
            self.counter += 1
        return tuple(out)

    def values(self, obs, out=None):
        """The value output alone in one launch (trunk, value tower, value head): the same bits as
        ``act``'s values.  Returns float32 [N] (``out`` when given)."""
        import torch
        N = self._obs(obs)
        if out is None:
            out = torch.empty(N, dtype=torch.float32, device=self.device)
        check_tensor("DevicePolicy", "out", out, self.device, torch.float32, (N,))
        self._check_rc(self._L.mrp_policy_values_device(self._h, stream_of(self.device), N, ptr(obs), ptr(out)))
        return out
