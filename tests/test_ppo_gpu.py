"""GPU checks of the device PPO update (csrc/mrp_ppo.hip through gym_puzzles_amd.ppo.DevicePPO): every
output equals the numpy rule (ppo_grad_ref / adam_ref / ppo_train_ref / exp_ref) on bit patterns."""
from __future__ import annotations

import numpy as np
import pytest
from ppo_cases import ARCHS, HP, exp_inputs, make_batch, make_params, on_device, same

from gym_puzzles_amd import policy as P
from gym_puzzles_amd import ppo as R

pytestmark = pytest.mark.gpu

NAMES = ("sb3-default", "reference-config", "odd-k-wide-head", "heads-only", "one-by-one", "width-one-inside", "width-one-towers")
BATCHES = (1, 31, 33, 256, 257, 600)   # partial tiles, a second workgroup, the chunk edge, a short chunk after two full ones


def _ppo(params, max_batch, **kw):
    pol = P.DevicePolicy.from_params(params)
    return pol, R.DevicePPO(pol, batch_size=max_batch, **HP, **kw)


def test_exp_on_the_device(gpu_lib):
    from gym_puzzles_amd import _native
    _, x = exp_inputs()
    assert x.size >= 500_000 and np.isnan(x).any() and np.isinf(x).any()
    out = np.zeros_like(x)
    assert gpu_lib.mrp_selftest_exp(0, _native._p(x), _native._p(out), x.size) == 0
    same(out, R.exp_ref(x), "exp_f32 on the device against exp_ref")


_CASES = {}


def _case(name):
    """(params, the largest minibatch): once per architecture, never changed."""
    if name not in _CASES:
        params = make_params(ARCHS[name], seed=3)
        _CASES[name] = (params, make_batch(params, 257 if name == "reference-config" else max(BATCHES)))
    return _CASES[name]


@pytest.mark.parametrize("name", NAMES)
def test_bitwise_grad(gpu_lib, name):
    params, batch = _case(name)
    sizes = [B for B in BATCHES if B <= batch[0].shape[0]]
    pol, ppo = _ppo(params, max(sizes))
    assert ppo.n_params == R.flatten_params(params).size
    for B in sizes:
        sub = tuple(a[:B] for a in batch)
        want_g, want_s = R.ppo_grad_ref(params, *sub, **HP)
        g, s = ppo.grad(*on_device(sub))
        same(s, want_s, f"{name} B={B} statistics")
        same(g, want_g, f"{name} B={B} flat gradient")
    same(R.flatten_params(pol.get_params()), R.flatten_params(params), "grad leaves the parameters alone")
    ppo.close()
    pol.close()


def zero_case(name):
    """The forward tests' zero case carried backward: biases of -0 and all-negative weights, observation
    rows of +0 and of -0, two observation columns of +-1.5e-38 (normal numbers whose products with the
    tiny deltas of advantages near 1e-9 underflow to zeros of the product's sign), samples with adv = +0
    and -0, and returns equal to the values (the value path's deltas are zeros)."""
    params = make_params(ARCHS[name], seed=4, negzero_bias=True)
    B = 40
    rng = np.random.default_rng(1)
    obs = rng.standard_normal((B, params.obs_dim)).astype(np.float32)
    if params.activation == "relu":
        # all-negative weights leave a relu network dead behind its first layer (every later pre-activation
        # is <= 0, every delta a zero, every sum from +0 a +0).  So that the sign-of-zero path is exercised
        # there too, only the first layer keeps negative weights, the later layers and the heads take |w|,
        # and the observations are negative: the first layer's units are live and its deltas are not zeros
        pos = lambda wb: (np.abs(wb[0]), wb[1])  # noqa: E731
        layers = [[wb if (i == 0 and t == 0) else pos(wb) for i, wb in enumerate(tw)]
                  for t, tw in enumerate((params.shared, params.pi, params.vf))]
        params = P.PolicyParams(*layers, pos(params.action), pos(params.value), params.log_std, "relu")
        obs = -np.abs(obs)
    obs[3], obs[36] = 0.0, -0.0
    obs[:, 0], obs[:, params.obs_dim // 2] = 1.5e-38, -1.5e-38
    eps = rng.standard_normal((B, params.act_dim)).astype(np.float32)
    actions, _, values, lp = P.policy_ref(params, obs, eps)
    offs = rng.uniform(-0.4, 0.4, B)
    offs[-4:] = 0.0                # the chunk's last samples are unclipped: their deltas are not zeros
    old = (lp.astype(np.float64) - offs).astype(np.float32)
    adv = (np.where(np.arange(B) % 2 == 0, 1.0, -1.0) * rng.uniform(0.2, 2.0, B) * 1e-9).astype(np.float32)
    adv[::4] = 0.0
    adv[5] = -0.0
    return params, (obs, actions, old, adv, values.copy())


@pytest.mark.parametrize("name", ["sb3-default", "odd-k-wide-head", "heads-only"])
def test_zeros_and_negative_zeros_backward(gpu_lib, name):
    """The gradient's zeros keep their signs: a chain that starts from +0 ends in -0 only where its last
    product underflows from below, and a pad term fma(0, 0, acc) behind it would turn that -0 into +0."""
    params, batch = zero_case(name)
    want_g, want_s = R.ppo_grad_ref(params, *batch, **HP)
    assert (np.signbit(want_g) & (want_g == 0)).any(), "the case holds negative zeros"
    assert ((want_g == 0) & ~np.signbit(want_g)).any() and (want_g != 0).any()
    pol, ppo = _ppo(params, batch[0].shape[0])
    g, s = ppo.grad(*on_device(batch))
    same(g, want_g, f"{name} flat gradient")
    same(s, want_s, f"{name} statistics")
    ppo.close()
    pol.close()


@pytest.mark.parametrize("name,max_norm", [("sb3-default", 0.5), ("odd-k-wide-head", 1e6)])
def test_three_steps(gpu_lib, name, max_norm):
    """Three consecutive steps equal adam_ref on ppo_grad_ref: parameters, std, m and v; the gradient
    norm lies above max_grad_norm in one case and below in the other; act afterwards uses the new
    parameters; a second DevicePPO on the same inputs gives identical bits."""
    import torch
    params = make_params(ARCHS[name], seed=7)
    B = 300
    batches = [make_batch(params, B, seed=20 + i) for i in range(3)]
    lr = 1e-3
    runs = []
    for _ in range(2):
        pol, ppo = _ppo(params, B, learning_rate=lr, max_grad_norm=max_norm)
        stats = [ppo.step(*on_device(b)).clone() for b in batches]
        runs.append((pol, ppo, stats))
    state, cur = R.AdamState(R.flatten_params(params).size), params
    coefs = []
    for i, b in enumerate(batches):
        grad, _ = R.ppo_grad_ref(cur, *b, **HP)
        coefs.append(float(R.clip_coef_ref(grad, max_norm)))
        cur, want_s = R.ppo_step_ref(cur, state, b, lr=lr, max_grad_norm=max_norm, **HP)
        same(runs[0][2][i], want_s, f"step {i + 1} statistics")
    assert all(c < 1 for c in coefs) if max_norm == 0.5 else all(c == 1 for c in coefs), coefs
    pol, ppo, _ = runs[0]
    assert ppo.t == 3 and state.t == 3
    got = pol.get_params()
    same(R.flatten_params(got), R.flatten_params(cur), "parameters after three steps")
    same(got.std, cur.std, "std")
    same(got.std, R.exp_ref(got.log_std), "std is exp_ref(log_std)")
    m, v = ppo.state()
    same(m, state.m, "m")
    same(v, state.v, "v")
    sd = pol.state_dict()
    same(R.flatten_params(P.params_from_state_dict(sd, params.activation)), R.flatten_params(cur), "state_dict")
    # act after step uses the new parameters
    rng = np.random.default_rng(5)
    obs = rng.standard_normal((70, params.obs_dim)).astype(np.float32)
    eps = rng.standard_normal((70, params.act_dim)).astype(np.float32)
    out = pol.act(torch.from_numpy(obs).cuda(), eps=torch.from_numpy(eps).cuda())
    for g, w, what in zip(out, P.policy_ref(got, obs, eps), ("actions", "clipped", "values", "log_probs")):
        same(g, w, f"act after step: {what}")
    # the second run
    pol2, ppo2, stats2 = runs[1]
    same(R.flatten_params(pol2.get_params()), R.flatten_params(got), "a second run: parameters")
    same(torch.stack(stats2), torch.stack(runs[0][2]).cpu().numpy(), "a second run: statistics")
    for a, b in zip(ppo2.state(), (m, v)):
        same(a, b, "a second run: moments")
    for p_, o_, _ in runs:
        o_.close()
        p_.close()


def test_train_end_to_end(gpu_lib):
    """collect_rollouts on MultiRobotPuzzle-v0 (64 lanes x 16 steps, TimeLimit 5, the default
    architecture), then train: the final parameters equal ppo_train_ref replayed on the host copies of
    the buffer with the permutations of an identically seeded generator; with normalize_advantage,
    train equals calling step with the torch-normalised advantages; a second rollout runs."""
    import torch
    from gym_puzzles_amd import DeviceRolloutBuffer, MultiRobotPuzzleVecEnv
    from gym_puzzles_amd.rollout import collect_rollouts
    N, T = 64, 16
    dev = torch.device("cuda", 0)
    env = MultiRobotPuzzleVecEnv("MultiRobotPuzzle-v0", N, seed=3, max_episode_steps=5)
    O, A = env.observation_space.shape[0], env.action_space.shape[0]
    params = make_params(ARCHS["sb3-default"], seed=6)
    pol = P.DevicePolicy.from_params(params, seed=77)
    buf = DeviceRolloutBuffer(T, N, (O,), A, device=0, gamma=0.99, gae_lambda=0.95)
    obs0 = torch.from_numpy(env.reset()).to(dev)
    start0 = torch.ones(N, dtype=torch.uint8, device=dev)
    nxt = collect_rollouts(env, pol, buf, obs0, start0)
    h = lambda t: t.reshape(T * N, *t.shape[2:]).cpu().numpy()  # noqa: E731
    data = (h(buf.observations), h(buf.actions), h(buf.log_probs), h(buf.advantages), h(buf.returns))
    hp = dict(HP, max_grad_norm=0.5)
    ppo = R.DevicePPO(pol, learning_rate=3e-4, n_epochs=2, batch_size=256, normalize_advantage=False, **hp)
    gen = torch.Generator(device="cpu").manual_seed(123)
    stats = ppo.train(buf, generator=gen)
    assert tuple(stats.shape) == (8, 5) and ppo.t == 8
    gen2 = torch.Generator(device="cpu").manual_seed(123)
    epochs = []
    for _ in range(2):
        perm = torch.randperm(T * N, generator=gen2).numpy()
        epochs.append((perm % T) * N + perm // T)           # DeviceRolloutBuffer.get's row-major position
    state = R.AdamState(ppo.n_params)
    want, want_stats = R.ppo_train_ref(params, state, data, epochs, 256, lr=3e-4, **hp)
    got = pol.get_params()
    same(stats, want_stats, "train statistics")
    same(R.flatten_params(got), R.flatten_params(want), "parameters after train")
    same(got.std, want.std, "std after train")
    # normalize_advantage: train equals step on the torch-normalised advantages
    pa = P.DevicePolicy.from_params(params)
    pb = P.DevicePolicy.from_params(params)
    ta = R.DevicePPO(pa, n_epochs=1, batch_size=256, normalize_advantage=True, **hp)
    tb = R.DevicePPO(pb, n_epochs=1, batch_size=256, **hp)
    ta.train(buf, generator=torch.Generator(device="cpu").manual_seed(9))
    for o, a, _, lp, adv, ret in buf.get(256, torch.Generator(device="cpu").manual_seed(9)):
        tb.step(o, a, lp, (adv - adv.mean()) / (adv.std() + 1e-8), ret)
    same(R.flatten_params(pa.get_params()), R.flatten_params(pb.get_params()), "normalize_advantage")
    assert not np.array_equal(R.flatten_params(pa.get_params()), R.flatten_params(params))
    # a second rollout with the trained policy
    collect_rollouts(env, pol, buf, *nxt)
    for t in (buf.actions, buf.values, buf.log_probs, buf.advantages, buf.returns):
        assert torch.isfinite(t).all()
    for x in (ta, tb, ppo, pa, pb, pol, env):
        x.close()


def test_inputs_are_not_written_and_argument_errors(gpu_lib):
    import torch
    params, batch = _case("sb3-default")
    B = 40
    sub = tuple(a[:B] for a in batch)
    pol, ppo = _ppo(params, B)
    d = on_device(sub)
    ppo.grad(*d)
    ppo.step(*d)
    for t, a, what in zip(d, sub, ("obs", "actions", "old_log_probs", "advantages", "returns")):
        same(t, a, f"{what} after the launches")
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    obs, act, old, adv, ret = d
    bad_calls = [
        lambda: ppo.grad(obs.cpu(), act, old, adv, ret),                       # device
        lambda: ppo.grad(obs, act, old.double(), adv, ret),                    # dtype
        lambda: ppo.grad(obs, z(B, 5), old, adv, ret),                         # shape
        lambda: ppo.grad(obs, act, old, z(B + 1), ret),
        lambda: ppo.grad(z(B, 56)[:, ::2], act, old, adv, ret),                # contiguity
        lambda: ppo.step(obs, act, old, adv, z(2 * B)[::2]),
        lambda: ppo.step(z(B + 1, 28), z(B + 1, 6), z(B + 1), z(B + 1), z(B + 1)),   # B > max_batch
        lambda: ppo.step(z(0, 28), z(0, 6), z(0), z(0), z(0)),
        lambda: ppo.grad(obs, act, old, adv, ret, out=z(ppo.n_params + 1)),
        lambda: ppo.grad(obs, act, old, adv, ret, stats_out=z(4)),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    five = z(5)
    with pytest.raises(ValueError, match="alias"):
        ppo.grad(z(5, 28), z(5, 6), five, z(5), z(5), stats_out=five)            # an output aliases an input
    big = z(B + 8)                                                               # an output inside an input's allocation
    with pytest.raises(ValueError, match="alias"):
        ppo.grad(obs, act, old, big[:B], ret, stats_out=big[B - 2:B + 3])
    with pytest.raises(ValueError, match="alias"):
        ppo.step(obs, act, old, adv, big[4:B + 4], stats_out=big[:5])
    both = z(ppo.n_params + 3)
    with pytest.raises(ValueError, match="overlap"):
        ppo.grad(obs, act, old, adv, ret, out=both[:ppo.n_params], stats_out=both[ppo.n_params - 2:])
    empty = P.DevicePolicy(28, 6, 0, 2, 2, [64, 64, 64, 64])
    e_ppo = R.DevicePPO(empty, batch_size=B, **HP)
    with pytest.raises(ValueError, match="set_params"):
        e_ppo.step(*d)
    with pytest.raises(ValueError, match="set_params"):
        empty.get_params()
    with pytest.raises(ValueError):
        R.DevicePPO(pol, batch_size=0)
    # parameters loaded later are picked up
    empty.set_params(params)
    g, _ = e_ppo.grad(*d)
    g0, _ = ppo_fresh_grad(params, d, B)
    same(g, g0, "gradient after a late set_params")
    for x in (e_ppo, ppo, empty, pol):
        x.close()


def test_calls_after_the_policy_is_closed_are_refused(gpu_lib):
    """mrp_ppo keeps its policy's pointer and reads it in every call: after ``pol.close()`` that is freed
    memory, so DevicePPO checks the policy's handle first."""
    params, batch = _case("sb3-default")
    B = 40
    d = on_device(tuple(a[:B] for a in batch))
    pol, ppo = _ppo(params, B)
    ppo.step(*d)
    pol.close()
    with pytest.raises(ValueError, match="closed"):
        ppo.step(*d)
    with pytest.raises(ValueError, match="closed"):
        ppo.grad(*d)
    with pytest.raises(ValueError, match="closed"):
        ppo.state()
    with pytest.raises(ValueError, match="DevicePolicy is closed"):
        pol.act(d[0])
    ppo.close()
    ppo.close()
    with pytest.raises(ValueError, match="DevicePPO is closed|DevicePolicy is closed"):
        ppo.step(*d)


def ppo_fresh_grad(params, d, B):
    pol, ppo = _ppo(params, B)
    g, s = ppo.grad(*d)
    out = (g.cpu().numpy(), s.cpu().numpy())
    ppo.close()
    pol.close()
    return out
