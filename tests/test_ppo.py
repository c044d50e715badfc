"""CPU checks of the PPO update's numpy rule (gym_puzzles_amd/ppo.py): exp_ref's accuracy, ppo_grad_ref
against SB3's loss written literally in float64 torch and differentiated by autograd, adam_ref and the
clip against torch.optim.Adam with clip_grad_norm_, and ppo_train_ref's bookkeeping."""
from __future__ import annotations

import math

import numpy as np
import pytest

from gym_puzzles_amd import policy as P
from gym_puzzles_amd import ppo as R

U = 2.0 ** -24          # unit roundoff of float32
EXP_ULPS = 0.501

# obs, act, (S, P, V), widths, activation: three of tests/test_policy_gpu.py's ARCHS
ARCHS = {
    "sb3-default": (28, 6, (0, 2, 2), [64, 64, 64, 64], "tanh"),
    "odd-k-wide-head": (27, 15, (1, 1, 1), [40, 24, 8], "relu"),
    "heads-only": (69, 4, (0, 0, 0), [], "tanh"),
}
BATCHES = (1, 33, 300)


def make_params(arch, seed=0, negzero_bias=False):
    obs_dim, act_dim, (S, Pn, V), widths, activation = arch
    rng = np.random.default_rng(seed)

    def lin(k, n):
        w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
        b = (rng.standard_normal(n) * 0.3).astype(np.float32)
        if negzero_bias:
            w, b = -np.abs(w), np.full(n, -0.0, np.float32)
        return w, b

    def tower(k, ws):
        out = []
        for n in ws:
            out.append(lin(k, n))
            k = n
        return out, k
    shared, kt = tower(obs_dim, widths[:S])
    pi, kp = tower(kt, widths[S:S + Pn])
    vf, kv = tower(kt, widths[S + Pn:])
    log_std = np.linspace(-0.8, 0.2, act_dim).astype(np.float32)
    return P.PolicyParams(shared, pi, vf, lin(kp, act_dim), lin(kv, 1), log_std, activation)


def make_batch(params, B, seed=5, clip=0.2):
    """A minibatch whose ratios fall inside (case 0), above (1) and below (2) the clip range, each with
    both advantage signs when B allows: sample n is case n % 3 with the sign of (n // 3) % 2."""
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((B, params.obs_dim)).astype(np.float32)
    eps = rng.standard_normal((B, params.act_dim)).astype(np.float32)
    actions, _, values, lp = P.policy_ref(params, obs, eps)
    n = np.arange(B)
    case, sign = n % 3, np.where((n // 3) % 2 == 0, 1.0, -1.0)
    offs = np.where(case == 0, rng.uniform(-0.1, 0.1, B), np.where(case == 1, 0.4, -0.4)) + rng.uniform(-0.02, 0.02, B)
    old = (lp.astype(np.float64) - offs).astype(np.float32)          # ratio = exp(offs)
    adv = (sign * rng.uniform(0.2, 2.0, B)).astype(np.float32)
    ret = (values + rng.standard_normal(B)).astype(np.float32)
    return obs, actions, old, adv, ret


# ---- exp ---------------------------------------------------------------------------------------------
def exp_inputs():
    rng = np.random.default_rng(11)
    sweep = np.linspace(-104, 89, 200_001).astype(np.float32)
    near = []
    for n in range(-151, 130):              # where n = nearest(x / ln 2) steps
        b = int(np.float32(abs((n + 0.5) * math.log(2.0))).view(np.uint32))
        a = np.arange(b - 2000, b + 2001, dtype=np.uint32).view(np.float32)
        near.append(a if n + 0.5 > 0 else -a)
    thresholds = []
    for x in (88.72284, -87.33655, -103.27893, -103.97208, 89.0, -104.0):   # overflow, subnormal, underflow, the clamps
        b = int(np.float32(abs(x)).view(np.uint32))
        a = np.arange(b - 2000, b + 2001, dtype=np.uint32).view(np.float32)
        thresholds.append(a if x > 0 else -a)
    subn = rng.uniform(-103.9, -87.4, 20_000).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-10, -1e-10, 200.0, -200.0, 3e38, -3e38], np.float32)
    special = np.concatenate([special, np.array([0x7F800001, 0xFFC00123, 0x7FC00000, 0xFF800001], np.uint32).view(np.float32)])
    rand = rng.integers(0, 1 << 32, 50_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return sweep, np.concatenate([sweep, np.concatenate(near), np.concatenate(thresholds), subn, special, rand])


def test_exp_ref_accuracy_and_monotone():
    sweep, x = exp_inputs()
    got = R.exp_ref(x)
    nan = np.isnan(x)
    assert nan.any() and (got.view(np.uint32)[nan] == x.view(np.uint32)[nan]).all(), "NaN payloads come back unchanged"
    xf, gf = x[~nan], got[~nan].astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        ref = np.exp(xf.astype(np.float64))
    over = ref >= 2.0 ** 128 * (1 - 2.0 ** -25)
    assert over.any() and np.isinf(gf[over]).all() and not np.isinf(gf[ref < 3.4028234e38]).any()
    r32 = np.minimum(ref, 3.4e38).astype(np.float32)
    ulp = np.maximum(np.spacing(np.abs(r32)).astype(np.float64), 2.0 ** -149)    # subnormal results: the fixed spacing
    err = np.abs(gf[~over] - ref[~over]) / ulp[~over]
    print(f"exp_ref max {err.max():.6f} ulp over {x.size} inputs")
    assert err.max() <= EXP_ULPS
    sub = (gf > 0) & (gf < 1.1754944e-38)
    assert sub.sum() > 1000 and (gf[ref < 2.0 ** -150 * (1 - 1e-9)] == 0).all() and (gf == 0).any()
    assert R.exp_ref(np.float32([0.0, -0.0])).tolist() == [1.0, 1.0]
    e = R.exp_ref(sweep)
    assert (e[1:] >= e[:-1]).all(), "monotone over the sweep"


# ---- the rule is PPO ---------------------------------------------------------------------------------
def torch_policy(params):
    """The network as a float64 torch module tree under SB3's parameter names."""
    import torch
    from torch import nn
    act = nn.Tanh if params.activation == "tanh" else nn.ReLU

    def seq(layers):
        mods = []
        for w, _ in layers:
            mods += [nn.Linear(w.shape[1], w.shape[0]), act()]
        return nn.Sequential(*mods)

    class Extractor(nn.Module):
        def __init__(self):
            super().__init__()
            self.shared_net, self.policy_net, self.value_net = seq(params.shared), seq(params.pi), seq(params.vf)

    class Policy(nn.Module):
        def __init__(self):
            super().__init__()
            self.log_std = nn.Parameter(torch.zeros(params.act_dim))
            self.mlp_extractor = Extractor()
            self.action_net = nn.Linear(params.action[0].shape[1], params.act_dim)
            self.value_net = nn.Linear(params.value[0].shape[1], 1)

        def evaluate_actions(self, obs, actions):
            trunk = self.mlp_extractor.shared_net(obs)
            mean = self.action_net(self.mlp_extractor.policy_net(trunk))
            values = self.value_net(self.mlp_extractor.value_net(trunk))
            dist = torch.distributions.Normal(mean, torch.ones_like(mean) * self.log_std.exp())
            return values.flatten(), dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)
    model = Policy().double()
    sd = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in R.state_dict_from_params(params).items()}
    model.load_state_dict(sd)
    return model


WRONG = ("no-clamp", "value-factor", "entropy-sign", "log-std-term")


def sb3_loss(model, batch, clip, ent_coef, vf_coef, wrong=None):
    """SB3's PPO.train() loss, literally.  ``wrong`` (one of WRONG) plants one mistake of the kind the
    bound has to reject: the clamp left out, the value loss's factor 2 lost, the entropy term's sign
    flipped, the -log_std term of the log-prob dropped from the gradient."""
    import torch
    import torch.nn.functional as F
    obs, actions, old, adv, ret = (torch.from_numpy(np.asarray(a, np.float64)) for a in batch)
    values, log_prob, entropy = model.evaluate_actions(obs, actions)
    if wrong == "log-std-term":
        log_prob = log_prob + model.log_std.sum() - model.log_std.sum().detach()
    if wrong == "entropy-sign":
        ent_coef = -ent_coef
    if wrong == "value-factor":
        vf_coef = vf_coef / 2
    ratio = torch.exp(log_prob - old)
    policy_loss_1 = adv * ratio
    policy_loss_2 = adv * (ratio if wrong == "no-clamp" else torch.clamp(ratio, 1 - clip, 1 + clip))
    policy_loss = -torch.min(policy_loss_1, policy_loss_2).mean()
    clip_fraction = torch.mean((torch.abs(ratio - 1) > clip).double())
    value_loss = F.mse_loss(ret, values)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    log_ratio = log_prob - old
    approx_kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
    stats = [policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction]
    return loss, np.array([float(s.detach()) for s in stats]), ratio.detach().numpy()


def majorant(params, batch, clip, ent_coef, vf_coef):
    """The a-priori error scale of every gradient entry: the rule's own backward pass in float64 with
    every signed sum replaced by the sum of absolute values (|W|, |x|, |delta|, |act'| <= 1), so a
    float32 rounding of relative size U anywhere moves an entry by at most U times this.  Returns the
    flat majorant, the sensitivity factor and the operation count of the longest chain."""
    obs, actions, old, adv, ret = (np.asarray(a, np.float64) for a in batch)
    B = obs.shape[0]
    f = (lambda x: np.tanh(x)) if params.activation == "tanh" else (lambda x: np.maximum(x, 0))
    ab = lambda wb: (np.abs(wb[0].astype(np.float64)), np.abs(wb[1].astype(np.float64)))  # noqa: E731

    def fwd(layers, x):
        """The float64 activations of a tower and their absolute values (the layers' inputs' majorants)."""
        xs = []
        for w, b in layers:
            x = f(x @ w.astype(np.float64).T + b)
            xs.append(np.abs(x))
        return x, xs
    trunk, xs_sh = fwd(params.shared, obs)
    fp, xs_pi = fwd(params.pi, trunk)
    fv, xs_vf = fwd(params.vf, trunk)
    wa, ba = ab(params.action)
    wv, bv = ab(params.value)
    mean = fp @ params.action[0].astype(np.float64).T + params.action[1]
    v = (fv @ params.value[0].astype(np.float64).T + params.value[1])[:, 0]
    mean_a, v_a = np.abs(fp) @ wa.T + ba, (np.abs(fv) @ wv.T + bv)[:, 0]
    std = np.exp(params.log_std.astype(np.float64))
    widths = [w.shape[1] for w, _ in params.shared + params.pi + params.vf + [params.action, params.value]]
    depth = len(params.shared) + max(len(params.pi), len(params.vf)) + 1
    # the longest chains: forward (the fan-ins of the layers in a row, the log-prob sum and exp) and
    # backward (the fan-outs back down, a chunk of samples, the chunks)
    n_fwd = sum(widths) + 2 * depth + 4 * params.act_dim + 8
    n_bwd = sum(widths) + 2 * depth + min(B, R.CHUNK) + -(-B // R.CHUNK) + 16
    d = actions - mean
    # |d| and |v - ret| with the forward pass's a-priori absolute error (test_policy.py's forward bound)
    d_a = np.abs(d) + n_fwd * U * (np.abs(actions) + mean_a)
    dvr_a = np.abs(v - ret) + n_fwd * U * (v_a + np.abs(ret))
    terms_a = (d_a * d_a) / (2 * std * std) + np.abs(params.log_std) + 1.0
    lp = (-(d * d) / (2 * std * std) - params.log_std - 0.9189385332046727).sum(1)
    ratio = np.exp(lp - old)
    g_a = np.abs(adv) * ratio / B
    dmean_a = g_a[:, None] * d_a / (std * std)
    ls_a = g_a[:, None] * (d_a * d_a / (std * std) + 1) + abs(ent_coef)
    dv_a = (2 * vf_coef * dvr_a / B)[:, None]
    grads = {}

    def bwd(layers, s_a, inputs_a, key):
        for i in range(len(layers) - 1, -1, -1):
            grads[key, i] = (s_a.T @ inputs_a[i], s_a.sum(0))        # |act'| <= 1
            s_a = s_a @ np.abs(layers[i][0].astype(np.float64))
        return s_a
    grads["action", 0] = (dmean_a.T @ np.abs(fp), dmean_a.sum(0))
    grads["value", 0] = (dv_a.T @ np.abs(fv), dv_a.sum(0))
    s_pi = bwd(params.pi, dmean_a @ wa, [np.abs(trunk)] + xs_pi[:-1], "pi")
    s_vf = bwd(params.vf, dv_a @ wv, [np.abs(trunk)] + xs_vf[:-1], "vf")
    bwd(params.shared, s_pi + s_vf, [np.abs(obs)] + xs_sh[:-1], "shared")
    parts = [ls_a.sum(0)]
    for key, n in (("shared", len(params.shared)), ("pi", len(params.pi)), ("vf", len(params.vf)), ("action", 1), ("value", 1)):
        for i in range(n):
            parts += [grads[key, i][0].ravel(), grads[key, i][1]]
    # sensitivity: a relative perturbation of the log-prob terms moves the ratio (and every policy
    # gradient) by the size of the terms; one of an activation moves tanh' = 1 - t^2 by at most 2
    # and a forward error of the mean moves d = action - mean, whose relative change |mean_a / d| enters
    # dmean and the log_std term; that part is carried in d_a above
    amp = 3.0 + terms_a.sum(1).max() + np.abs(lp - old).max()
    return np.concatenate(parts), amp, n_bwd + amp * n_fwd


_GRAD_CASES = {}


def grad_case(name, B):
    if (name, B) not in _GRAD_CASES:
        params = make_params(ARCHS[name], seed=3)
        batch = make_batch(params, B)
        _GRAD_CASES[name, B] = (params, batch, R.ppo_grad_ref(params, *batch, clip_range=0.2, ent_coef=0.01, vf_coef=0.5))
    return _GRAD_CASES[name, B]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", list(ARCHS))
def test_rule_is_ppo(name, B):
    """ppo_grad_ref against autograd on SB3's loss in float64.  The bound is a priori: every float32
    operation of the rule carries a relative rounding of at most U; the longest dependency chain has
    n_ops operations; the sum of the absolute values of everything that is added into a gradient
    entry is `majorant`'s; `amp` bounds how much a relative error of the forward pass is amplified on
    its way through exp and act', so an entry's error is at most (n_bwd + amp * n_fwd) * U * majorant
    to first order.  A wrong sign, factor, index or missing term moves some tensor by
    percent of its largest entry, which the last assertion keeps far above the bound."""
    import torch
    clip, ent_coef, vf_coef = 0.2, 0.01, 0.5
    params, batch, (grad, stats) = grad_case(name, B)
    model = torch_policy(params)
    names = [n for n, _ in model.named_parameters()]
    assert names == list(R.state_dict_from_params(params)), "the flat order is SB3's parameters() order"
    loss, want_stats, ratio = sb3_loss(model, batch, clip, ent_coef, vf_coef)
    loss.backward()
    want = np.concatenate([p.grad.numpy().ravel() for p in model.parameters()])
    assert grad.shape == want.shape and grad.dtype == np.float32 and stats.shape == (5,)
    if B >= 33:
        case, pos = np.arange(B) % 3, batch[3] > 0
        for c, test in ((0, np.abs(ratio - 1) < clip), (1, ratio > 1 + clip), (2, ratio < 1 - clip)):
            assert test[case == c].all() and (pos & test).any() and (~pos & test).any()
    maj, amp, n_ops = majorant(params, batch, clip, ent_coef, vf_coef)
    bound = n_ops * U * maj
    err = np.abs(grad.astype(np.float64) - want)
    worst = (err / np.maximum(bound, 1e-300)).max()
    print(f"{name} B={B}: max |grad error| {err.max():.3e}, max error / bound {worst:.4f}, max bound / max |grad| "
          f"{bound.max() / np.abs(want).max():.3e}")
    assert (err <= bound).all()
    # the bound separates rounding from a wrong formula (a wrong sign, factor, index or a missing term moves
    # entries by tens of percent of the largest one on these asymmetric inputs): it stays below 5 percent of
    # the largest gradient entry (at B = 300 the entries are signed sums that cancel while the majorant adds)
    assert bound.max() < 5e-2 * np.abs(want).max()
    # and explicitly: one planted mistake at a time moves some entry of the float64 gradient by more than twice
    # the bound, so a rule with that mistake (itself within the bound of the mistaken gradient) could not
    # pass the assertion above (with one sample, in the clip range, the clamp cannot show)
    for wrong in WRONG:
        if wrong == "no-clamp" and B == 1:
            continue
        model.zero_grad()
        sb3_loss(model, batch, clip, ent_coef, vf_coef, wrong=wrong)[0].backward()
        mistaken = np.concatenate([p.grad.numpy().ravel() for p in model.parameters()])
        excess = (np.abs(want - mistaken) / np.maximum(bound, 1e-300)).max()
        print(f"{name} B={B}: planted {wrong}: max |difference| / bound {excess:.1f}")
        assert excess > 2, wrong
    obs, actions, old, adv, ret = batch
    scale = np.array([np.abs(adv).max() * ratio.max(), 4 * np.abs(ret).max() ** 2 + 4 * stats[1], abs(want_stats[2]),
                      ratio.max() + np.abs(np.log(ratio)).max() + 1, 1.0])
    serr = np.abs(stats.astype(np.float64) - want_stats)
    print(f"{name} B={B}: stats error {serr}")
    assert (serr <= n_ops * U * scale).all()
    assert stats[4] == np.float32(want_stats[4]), "no ratio lies near the clip boundary: the clip fraction is exact"


def test_evaluate_is_the_forward_rule():
    """The rule's evaluate step gives policy_ref's values and log-probs bit for bit on the actions
    policy_ref sampled, so on unchanged parameters the ratio is exactly 1 and approx_kl exactly 0."""
    for name in ARCHS:
        params = make_params(ARCHS[name], seed=2)
        rng = np.random.default_rng(4)
        obs = rng.standard_normal((37, params.obs_dim)).astype(np.float32)
        eps = rng.standard_normal((37, params.act_dim)).astype(np.float32)
        actions, _, values, lp = P.policy_ref(params, obs, eps)
        v, got_lp, ent = R.evaluate_actions_ref(params, obs, actions)
        assert np.array_equal(v.view(np.uint32), values.view(np.uint32)), name
        assert np.array_equal(got_lp.view(np.uint32), lp.view(np.uint32)), name
        assert np.array_equal(v.view(np.uint32), P.values_ref(params, obs).view(np.uint32))
        want_ent = (0.5 + 0.5 * math.log(2 * math.pi) + params.log_std.astype(np.float64)).sum()
        assert abs(float(ent) - want_ent) <= 4 * params.act_dim * U * (np.abs(params.log_std).sum() + 1.5 * params.act_dim)
        adv = rng.standard_normal(37).astype(np.float32)
        _, stats = R.ppo_grad_ref(params, obs, actions, lp, adv, values)
        assert stats[3] == 0 and stats[4] == 0 and stats[1] == 0, "ratio 1: approx_kl, clip fraction; returns = values"
        assert stats[0] == np.float32(R._chunk_sum64(-adv) * (1.0 / 37))


def test_grad_ties_and_boundaries():
    """adv = 0 (pl1 == pl2 == 0: the first branch, g = -0 * ... stays a zero) and B = 1."""
    params = make_params(ARCHS["heads-only"], seed=1)
    obs, actions, old, adv, ret = make_batch(params, 7)
    adv[:] = 0.0
    grad, stats = R.ppo_grad_ref(params, obs, actions, old, adv, ret, vf_coef=0.0)
    A = params.act_dim
    assert (grad[A:] == 0).all() and (grad[:A] == 0).all() and stats[0] == 0


# ---- Adam and the clip -------------------------------------------------------------------------------
def test_adam_ref_and_clip():
    import torch
    rng = np.random.default_rng(2)
    n, lr, max_norm = 300, 3e-4, 0.5
    p0 = rng.standard_normal(n).astype(np.float32)
    gs = [rng.standard_normal(n).astype(np.float32) * s for s in (1.0, 0.01, 0.2)]      # norms ~17, ~0.17, ~3.5
    norms = [float(np.linalg.norm(g.astype(np.float64))) for g in gs]
    assert norms[0] > max_norm > norms[1]
    tp = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([tp], lr=lr, eps=1e-5)
    st = R.AdamState(n)
    p = p0.copy()
    for step, g in enumerate(gs):
        tp.grad = torch.from_numpy(g.astype(np.float64)).clone()
        torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        p_before = p
        p, coef = R.adam_ref(p, g, st, lr, max_norm)
        assert st.t == step + 1 and p.dtype == np.float32 and coef.dtype == np.float32
        if norms[step] < max_norm:
            assert coef == np.float32(1.0), "below the threshold the gradients are multiplied by exactly 1"
        else:
            assert abs(float(coef) - max_norm / (norms[step] + 1e-6)) <= 2 * U * float(coef)
        want = tp.detach().numpy()
        # a priori: the update is lr * O(1) per step (|m / (sqrt(v) + eps)| <= 1 / (1 - b1) worst case, ~1
        # typically); 12 float32 operations with relative rounding U act on the update, one on |p| per step
        upd = np.abs(want - p_before.astype(np.float64)) + lr
        bound = (step + 1) * (2 * U * np.abs(want) + 40 * U * upd * 10)
        err = np.abs(p.astype(np.float64) - want)
        print(f"step {step + 1}: coef {coef}, max error {err.max():.3e}, max error / bound {(err / bound).max():.4f}")
        assert (err <= bound).all()
        assert bound.max() < 0.02 * lr + 4 * U * np.abs(want).max(), "the bound is far below a step's size"
    state = opt.state[tp]
    assert np.abs(st.m - state["exp_avg"].numpy()).max() <= 40 * U * np.abs(state["exp_avg"].numpy()).max()
    assert np.abs(st.v - state["exp_avg_sq"].numpy()).max() <= 40 * U * np.abs(state["exp_avg_sq"].numpy()).max()


def test_clip_coef_order():
    """The sum of squares is 256 interleaved float64 partials, then the partials ascending."""
    g = (np.random.default_rng(0).standard_normal(1000) * 3).astype(np.float32)
    sq = g.astype(np.float64) ** 2
    parts = [0.0] * 256
    for e in range(1000):
        parts[e % 256] += sq[e]
    total = 0.0
    for t in range(256):
        total += parts[t]
    assert R.clip_coef_ref(g, 0.5) == np.float32(0.5 / (math.sqrt(total) + 1e-6))


# ---- bookkeeping -------------------------------------------------------------------------------------
def test_train_ref_bookkeeping():
    params = make_params(ARCHS["odd-k-wide-head"], seed=8)
    total, bs = 50, 16
    data = make_batch(params, total, seed=9)
    rng = np.random.default_rng(1)
    epochs = [rng.permutation(total) for _ in range(2)]
    hp = dict(lr=1e-3, ent_coef=0.01)
    state = R.AdamState(R.flatten_params(params).size)
    got, stats = R.ppo_train_ref(params, state, data, epochs, bs, **hp)
    assert state.t == 2 * 4 and stats.shape == (8, 5)        # 16 + 16 + 16 + 2 per epoch
    # the same steps by hand, in the order the rule promises
    st2 = R.AdamState(R.flatten_params(params).size)
    cur, k = params, 0
    for order in epochs:
        for s in (0, 16, 32, 48):
            idx = order[s:s + 16]
            cur, s_k = R.ppo_step_ref(cur, st2, tuple(a[idx] for a in data), **hp)
            assert np.array_equal(s_k.view(np.uint32), stats[k].view(np.uint32))
            k += 1
    assert np.array_equal(R.flatten_params(cur).view(np.uint32), R.flatten_params(got).view(np.uint32))
    assert not np.array_equal(R.flatten_params(got), R.flatten_params(params))
    assert np.array_equal(got.std.view(np.uint32), R.exp_ref(got.log_std).view(np.uint32))
    # state_dict round trip
    sd = R.state_dict_from_params(got)
    back = P.params_from_state_dict(sd, got.activation)
    assert np.array_equal(R.flatten_params(back), R.flatten_params(got))
    assert (len(back.shared), len(back.pi), len(back.vf)) == (1, 1, 1)
    again = R.unflatten_params(params, R.flatten_params(got), std=got.std)
    assert np.array_equal(again.std, got.std) and np.array_equal(R.flatten_params(again), R.flatten_params(got))
    with pytest.raises(ValueError):
        P.PolicyParams(got.shared, got.pi, got.vf, got.action, got.value, got.log_std, got.activation, std=np.ones(3))


def test_names_and_abi():
    import gym_puzzles_amd as G
    from gym_puzzles_amd import _native
    from gym_puzzles_amd import build as b
    for name in ("ppo_grad_ref", "adam_ref", "ppo_train_ref", "exp_ref"):
        assert hasattr(G, name)
    for name in ("mrp_ppo_create", "mrp_ppo_destroy", "mrp_ppo_last_error", "mrp_ppo_grad_device", "mrp_ppo_step_device",
                 "mrp_policy_get_params", "mrp_selftest_exp"):
        assert name in _native.EXPORTED, name
    assert b.PPO_SOURCES[0][0] == "mrp_ppo.hip" and b.UNITS[-1] == b.PPO_SOURCES[0] and "mrp_policy_net.h" in b.HEADERS
    assert R.CHUNK == 256
