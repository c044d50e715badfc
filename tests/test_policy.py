"""CPU checks of the device policy's rule (gym_puzzles_amd/policy.py): the exact-fma scheme, the
tanh rule, the linear layer and the distribution against float64, the SB3 state_dict loader and
the argument limits.  No device is used here; tests/test_policy_gpu.py pins the kernel to the rule."""
from __future__ import annotations

import hashlib
import math
from fractions import Fraction

import numpy as np
import pytest
from ppo_cases import ARCHS, bits, make_batch, make_params

from gym_puzzles_amd import policy as P

U = 2.0 ** -24          # float32 unit roundoff
TANH_ULPS = 0.501       # measured maximum of tanh_ref (DESIGN.md "Device policy"): 0.5 ulp + 2^-25, asserted below


# ---- the fma scheme ----------------------------------------------------------------------------------
def _fma_exact(a, b, c):
    """fmaf by rational arithmetic: the exact a * b + c rounded once to float32 (round to nearest even)."""
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        # IEEE: an exact zero sum is +0 unless both addends are -0
        prod_neg = math.copysign(1.0, float(a)) * math.copysign(1.0, float(b)) < 0
        return np.float32(-0.0 if (prod_neg and math.copysign(1.0, float(c)) < 0) else 0.0)
    sign, m = (-1, -v) if v < 0 else (1, v)
    e = math.frexp(float(m))[1] - 1                   # 2^e <= m < 2^(e+1), after the two corrections
    while Fraction(2) ** (e + 1) <= m:
        e += 1
    while Fraction(2) ** e > m:
        e -= 1
    e = max(e, -126)                                  # subnormal results share the spacing 2^-149
    q = Fraction(2) ** (e - 23)                       # the spacing of float32 at m
    n, rem = divmod(m, q)
    n = int(n)
    if rem * 2 > q or (rem * 2 == q and n & 1):
        n += 1
    return np.float32(sign * float(n * q))


def _fma_triples():
    rng = np.random.default_rng(11)
    n = 3000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    # near-midpoint cases: c has an odd last bit and a * b = half an ulp of c times (1 - i^2 2^-46), a hair
    # below the midpoint: an fma rounds down to c, while a float64 multiply-add first rounds the sum onto
    # the midpoint and then to even, away from c
    m, i = rng.integers(0, 1 << 22, 1000), rng.integers(1, 1 << 10, 1000)
    sgn = np.where(rng.integers(0, 2, 1000) == 1, -1.0, 1.0)
    c[:1000] = (sgn * ((1 << 23) + 2 * m + 1) * 2.0 ** -23).astype(np.float32)
    a[:1000] = (sgn * 2.0 ** -24 * (1 + i * 2.0 ** -23)).astype(np.float32)
    b[:1000] = (1 - i * 2.0 ** -23).astype(np.float32)
    # zeros and signs
    a[-8:] = [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 2.0, 3.0]
    b[-8:] = [1.0, 1.0, -1.0, 0.0, 1.0, 1.0, 0.5, 1.0 / 3]
    c[-8:] = [-0.0, -0.0, 0.0, -0.0, -1.0, 1.0, -1.0, -1.0]
    return a, b, c


def test_fma_scheme_is_an_fma():
    a, b, c = _fma_triples()
    got = P.fma32(a, b, c)
    if hasattr(math, "fma"):
        want = np.array([np.float32(math.fma(float(x), float(y), float(z))) for x, y, z in zip(a, b, c)], np.float32)
    else:
        want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(bits(got), bits(want))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(bits(naive), bits(want)), "the triples include cases where double rounding shows"


# ---- tanh --------------------------------------------------------------------------------------------
def _around(points, ulps):
    out = []
    for x in points:
        b = int(np.float32(x).view(np.uint32))
        out.append(np.arange(max(b - ulps, 0), b + ulps + 1, dtype=np.uint32).view(np.float32))
    return np.concatenate(out)


def _tanh_sweep():
    rng = np.random.default_rng(5)
    near0 = np.arange(0, 1 << 16, dtype=np.uint32).view(np.float32)           # +0 and the smallest subnormals up
    branch = _around(P.TANH_BRANCH_POINTS, 300)
    wide = rng.uniform(-12.0, 12.0, 700_000).astype(np.float32)
    small = (rng.uniform(-1.0, 1.0, 300_000) * 10.0 ** rng.uniform(-30, 0, 300_000)).astype(np.float32)
    x = np.concatenate([near0, branch, wide, small])
    return np.concatenate([x, -x])


def _ulps(got32, x32):
    ref = np.tanh(x32.astype(np.float64))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(got32.astype(np.float64) - ref) / ulp


def test_tanh_properties():
    x = np.sort(np.concatenate([np.linspace(-21, 21, 400_001), np.linspace(-0.01, 0.01, 200_001)]).astype(np.float32))
    t = P.tanh_ref(x)
    assert np.array_equal(bits(P.tanh_ref(-x)), bits(-t)), "odd"
    assert (np.diff(t) >= 0).all(), "monotone"
    assert (np.abs(t) <= 1).all() and (t[x >= 9.5] == 1).all() and (t[x <= -9.5] == -1).all()
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 1e30, -1e30, 20.0, np.float32(20.0) - np.spacing(np.float32(19.0))], np.float32)
    want = np.array([0.0, -0.0, 1.0, -1.0, 1.0, -1.0, 1.0, 1.0], np.float32)
    assert np.array_equal(bits(P.tanh_ref(sp)), bits(want))
    nans = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)
    assert np.array_equal(bits(P.tanh_ref(nans)), bits(nans)), "NaN comes back unchanged"


def test_tanh_accuracy():
    """Maximum error in float32 ulps against float64 np.tanh; the yardstick is float32 np.tanh on the
    same sweep (the rule may take up to twice that), and the measured maximum is pinned."""
    x = _tanh_sweep()
    ours, numpy32 = _ulps(P.tanh_ref(x), x).max(), _ulps(np.tanh(x), x).max()
    print(f"tanh_ref max {ours:.6f} ulp, float32 np.tanh max {numpy32:.6f} ulp over {x.size} inputs")
    assert ours <= 2 * numpy32
    assert ours <= TANH_ULPS


# ---- linear layer and network against float64 ---------------------------------------------------------
def test_linear_layer_against_float64():
    rng = np.random.default_rng(2)
    for N, K, M in ((7, 1, 3), (5, 27, 40), (3, 256, 33)):
        x, w, b = (rng.standard_normal(s).astype(np.float32) for s in ((N, K), (M, K), (M,)))
        got = P.linear_ref(x, w, b).astype(np.float64)
        x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
        bound = (K + 2) * U * (np.abs(x64) @ np.abs(w64).T + np.abs(b64))
        assert (np.abs(got - (x64 @ w64.T + b64)) <= bound).all()
    # the chain starts from the bias and keeps the sign of zero
    # (products of -0 leave a bias of -0 alone, one product of +0 turns it into +0)
    w = np.array([[-1, -1, -1], [-1, 1, -1]], np.float32)
    z = P.linear_ref(np.zeros((1, 3), np.float32), w, np.array([-0.0, -0.0], np.float32))
    assert np.array_equal(bits(z), bits(np.array([[-0.0, 0.0]], np.float32)))


def _sb3_tree(obs_dim, act_dim, shared, pi, vf, activation, seed):
    """A torch module tree with stable-baselines3's parameter names (ActorCriticPolicy + MlpExtractor)."""
    import torch
    from torch import nn
    torch.manual_seed(seed)
    act = nn.Tanh if activation == "tanh" else nn.ReLU

    def seq(k, widths):
        mods = []
        for w in widths:
            mods += [nn.Linear(k, w), act()]
            k = w
        return nn.Sequential(*mods), k

    class Extractor(nn.Module):
        def __init__(self):
            super().__init__()
            self.shared_net, kt = seq(obs_dim, shared)
            self.policy_net, self.kp = seq(kt, pi)
            self.value_net, self.kv = seq(kt, vf)

    class Tree(nn.Module):
        def __init__(self):
            super().__init__()
            self.mlp_extractor = Extractor()
            self.action_net = nn.Linear(self.mlp_extractor.kp, act_dim)
            self.value_net = nn.Linear(self.mlp_extractor.kv, 1)
            self.log_std = nn.Parameter(torch.linspace(-0.7, 0.3, act_dim))

        def forward(self, obs):
            t = self.mlp_extractor.shared_net(obs)
            return (self.action_net(self.mlp_extractor.policy_net(t)), self.value_net(self.mlp_extractor.value_net(t))[:, 0])
    return Tree()


def _forward64_with_bound(params, obs):
    """float64 forward of the rule's network with the a-priori float32 error bound carried alongside:
    e_out = |W| e_in + (K + 2) u (|W| (|x| + e_in) + |b|); the activation is 1-Lipschitz and tanh_ref adds
    its measured ulp bound."""
    def lin(wb, x, e):
        w64, b64, K = wb[0].astype(np.float64), wb[1].astype(np.float64), wb[0].shape[1]
        aw = np.abs(w64).T
        return x @ w64.T + b64, e @ aw + (K + 2) * U * ((np.abs(x) + e) @ aw + np.abs(b64))

    def through(layers, x, e):
        for wb in layers:
            y, e = lin(wb, x, e)
            if params.activation == "tanh":
                x = np.tanh(y)
                e = e + TANH_ULPS * 2.0 ** -23 * np.abs(x)     # an ulp of float32 at t is at most 2^-23 |t|
            else:
                x = np.maximum(y, 0.0)
        return x, e
    x0 = obs.astype(np.float64)
    t, et = through(params.shared, x0, np.zeros_like(x0))
    xp, ep = through(params.pi, t, et)
    xv, ev = through(params.vf, t, et)
    mean, em = lin(params.action, xp, ep)
    val, evl = lin(params.value, xv, ev)
    return mean, em, val[:, 0], evl[:, 0]


@pytest.mark.parametrize("arch", [(0, 2, 2), (2, 0, 0), (1, 1, 1)])
def test_loader_and_forward_against_the_torch_tree(arch):
    import torch
    S, Pn, V = arch
    widths = {(0, 2, 2): ([], [64, 64], [64, 64]), (2, 0, 0): ([256, 256], [], []), (1, 1, 1): ([40], [24], [8])}[arch]
    tree = _sb3_tree(28, 6, *widths, "tanh", seed=S * 7 + Pn)
    params = P.params_from_state_dict(tree.state_dict(), "tanh")
    assert (len(params.shared), len(params.pi), len(params.vf)) == arch
    assert params.widths == widths[0] + widths[1] + widths[2] and (params.obs_dim, params.act_dim) == (28, 6)
    obs = np.random.default_rng(3).standard_normal((9, 28)).astype(np.float32)
    with torch.no_grad():
        tm, tv = tree.double()(torch.from_numpy(obs).double())
    mean64, em, val64, ev = _forward64_with_bound(params, obs)
    assert np.allclose(mean64, tm.numpy(), rtol=0, atol=1e-12) and np.allclose(val64, tv.numpy(), rtol=0, atol=1e-12)
    actions, _, values, _ = P.policy_ref(params, obs, deterministic=True)
    assert em.max() < 1e-3 and ev.max() < 1e-3, "the bound itself stays far below a transposed weight's O(1) error"
    assert (np.abs(actions.astype(np.float64) - tm.numpy()) <= em).all()
    assert (np.abs(values.astype(np.float64) - tv.numpy()) <= ev).all()
    assert np.array_equal(bits(P.values_ref(params, obs)), bits(values))


def test_log_prob_and_clipped_against_float64():
    rng = np.random.default_rng(8)
    tree = _sb3_tree(5, 15, [], [16], [16], "relu", seed=1)
    params = P.params_from_state_dict(tree.state_dict(), "relu")
    obs = rng.standard_normal((50, 5)).astype(np.float32)
    eps = (rng.standard_normal((50, 15)) * 2).astype(np.float32)
    mean = P.policy_ref(params, obs, deterministic=True)[0].astype(np.float64)
    actions, clipped, _, logp = P.policy_ref(params, obs, eps)
    std, ls = params.std.astype(np.float64), params.log_std.astype(np.float64)
    a64 = mean + std * eps
    ba = 2 * U * (np.abs(mean) + np.abs(std * eps))
    assert (np.abs(actions - a64) <= ba).all()
    assert (np.abs(clipped - np.clip(a64, -1, 1)) <= ba).all() and (np.abs(clipped) <= 1).all()
    assert (clipped[np.abs(actions) <= 1] == actions[np.abs(actions) <= 1]).all() and (np.abs(actions) > 1).any()
    # from the float32 actions: d, d * d, std * std, the quotient and two subtractions round once each
    d = actions.astype(np.float64) - mean
    q = -(d * d) / (2 * std * std)
    C = float(P.LOG_SQRT_2PI)
    terms = q - ls - C
    per_term = 6 * U * np.abs(q) + 2 * U * (np.abs(q) + np.abs(ls) + C)
    bound = per_term.sum(1) + 15 * U * (np.abs(terms) + per_term).sum(1)
    assert (np.abs(logp - terms.sum(1)) <= bound).all()
    assert bound.max() < 1e-3
    # deterministic: the action is the mean and every d is zero
    a_det, _, _, lp_det = P.policy_ref(params, obs, deterministic=True)
    assert np.allclose(lp_det, (-ls - C).sum(), rtol=0, atol=15 * 4 * U * (np.abs(ls) + C).sum())


def test_argument_errors():
    f = np.float32
    W = lambda o, i: np.zeros((o, i), f)  # noqa: E731
    b = lambda o: np.zeros(o, f)  # noqa: E731
    ok = P.PolicyParams([], [], [], (W(6, 28), b(6)), (W(1, 28), b(1)), b(6))
    assert (ok.obs_dim, ok.act_dim, ok.widths) == (28, 6, [])
    assert np.array_equal(ok.std, np.ones(6, f))
    bad = [
        lambda: P.PolicyParams([], [], [], (W(17, 28), b(17)), (W(1, 28), b(1)), b(17)),                  # act_dim 17
        lambda: P.PolicyParams([], [], [], (W(6, 257), b(6)), (W(1, 257), b(1)), b(6)),                    # obs_dim 257
        lambda: P.PolicyParams([(W(257, 8), b(257))], [], [], (W(2, 257), b(2)), (W(1, 257), b(1)), b(2)),  # width 257
        lambda: P.PolicyParams([(W(8, 8), b(8))] * 3, [(W(8, 8), b(8))] * 2, [], (W(2, 8), b(2)), (W(1, 8), b(1)), b(2)),  # depth 5
        lambda: P.PolicyParams([(W(8, 4), b(8))], [], [], (W(2, 9), b(2)), (W(1, 8), b(1)), b(2)),          # does not chain
        lambda: P.PolicyParams([], [], [], (W(2, 4), b(2)), (W(2, 4), b(2)), b(2)),                        # value head of 2
        lambda: P.PolicyParams([], [], [], (W(2, 4), b(2)), (W(1, 4), b(1)), b(3)),                        # log_std length
        lambda: P.PolicyParams([], [], [], (W(2, 4), b(2)), (W(1, 4), b(1)), b(2), activation="gelu"),
        lambda: P.check_arch(0, 1, 0, 0, 0, []),
        lambda: P.check_arch(4, 0, 0, 0, 0, []),
        lambda: P.check_arch(4, 2, 1, 0, 0, [0]),
        lambda: P.check_arch(4, 2, 1, 4, 0, [8] * 5),
        lambda: P.params_from_state_dict({"action_net.weight": W(2, 4)}),
    ]
    for case in bad:
        with pytest.raises(ValueError):
            case()
    P.check_arch(256, 16, 2, 2, 2, [256] * 6)
    P.check_arch(1, 1, 0, 1, 0, [1])


# ---- the synthetic network ---------------------------------------------------------------------------
# sha256 over flatten_params(...) and log_std, in turn, of the parameters that the tests, the benches and the
# data-parallel worker run on.  Every bitwise test compares device and rule on the same parameters, so a drifted
# generator would pass them all while changing which cases are covered.
PINNED = {
    # ppo_cases.make_params at seeds 0, 3, 4 and at seed 4 with negzero_bias
    "sb3-default": "e4181dedf47859f053e6bc833b7e7ea3c62d5a06fc884577e2c9f9eddbadd15a",
    "reference-config": "49108dbbb7e2af362e434b7278a315f8a47021c0f373484b0cb170190ba754c3",
    "odd-k-wide-head": "844e6b201f2cc4243f248dff417e8e2e6ceb647a5effe5ba9338fe3605c47444",
    "heads-only": "9ecaba34bc4ce0082d9ec46512833e966938c9939754163f41f72a20838fc236",
    "one-by-one": "7a4676670171c297c1103961b88411924df2d187e7cce58e3b9b4bd09b635b0c",
    "width-one-inside": "42f9bd4a92c275783a2c4907a59c7da3413565e0c37fc91b8795912dd6fa7fd4",
    "width-one-towers": "52ace16eb62929dac105b45ec1a0212a30cc871bd36f88e946c336a5d173227e",
    # the benches' two architectures (tools/trainbench.py bench_params) at seed len(name)
    "sb3_default_pi64x2_vf64x2": "d154e36d20b3c8c739c33d52551f9f999e0b8b836a69844c28ecaa49996020cb",
    "reference_shared256x2": "3aabc5f86607d61cf4d2a96fcd5da9e5ba8d5b5801d9e1071ea5da195f88b663",
    # tools/ppo_ddp_worker.py's ranks 0 and 1
    "ddp-worker-seed-10": "477e9123b652a5ddc6bee1ae208d10afb28f89b2336c8c567502d7fb31dabc97",
    "ddp-worker-seed-11": "75d4f81f8d07a77a3b8ff4c96817765287ae8b173c3c54ff837da3a708f8940c",
    # the five arrays of make_batch(make_params(sb3-default, seed 3), 33)
    "make_batch": "e29bfd0e658bd0feccca5ec412c510e540053899f87d032a3edbec85e1717055",
}


def test_random_params_are_pinned():
    def digest(arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()
    of = lambda params: [P.flatten_params(params), params.log_std]  # noqa: E731
    got = {}
    for name, arch in ARCHS.items():
        runs = [make_params(arch, seed) for seed in (0, 3, 4)] + [make_params(arch, 4, negzero_bias=True)]
        got[name] = digest([a for params in runs for a in of(params)])
    bench_log_std = np.linspace(-0.5, 0.0, 6).astype(np.float32)
    for name, shared, pi, vf in (("sb3_default_pi64x2_vf64x2", [], [64, 64], [64, 64]), ("reference_shared256x2", [256, 256], [], [])):
        got[name] = digest(of(P.random_params(28, 6, shared, pi, vf, "tanh", len(name), 0.1, bench_log_std)))
    for seed in (10, 11):
        got[f"ddp-worker-seed-{seed}"] = digest(of(P.random_params(28, 6, [], [64, 64], [64, 64], "tanh", seed, 0.1, bench_log_std)))
    got["make_batch"] = digest(make_batch(make_params(ARCHS["sb3-default"], seed=3), 33))
    assert got == PINNED
    zero = make_params(ARCHS["odd-k-wide-head"], 4, negzero_bias=True)
    assert all((w < 0).all() and np.signbit(b).all() and not b.any() for w, b in P._layers(zero))
