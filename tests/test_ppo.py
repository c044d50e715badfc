"""CPU checks of the PPO update's numpy rule (gym_puzzles_amd/ppo.py): exp_ref's accuracy, ppo_grad_ref
against SB3's loss written literally in float64 torch and differentiated by autograd, adam_ref and the
clip against torch.optim.Adam with clip_grad_norm_, and ppo_train_ref's bookkeeping."""
from __future__ import annotations

import math

import numpy as np
import pytest
from ppo_cases import ARCHS, BATCHES, WRONG, U, exp_inputs, majorant, make_batch, make_params, sb3_loss, torch_policy

from gym_puzzles_amd import policy as P
from gym_puzzles_amd import ppo as R

EXP_ULPS = 0.501
NAMES = ("sb3-default", "odd-k-wide-head", "heads-only")


# ---- exp ---------------------------------------------------------------------------------------------
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
_GRAD_CASES = {}


def grad_case(name, B):
    if (name, B) not in _GRAD_CASES:
        params = make_params(ARCHS[name], seed=3)
        batch = make_batch(params, B)
        _GRAD_CASES[name, B] = (params, batch, R.ppo_grad_ref(params, *batch, clip_range=0.2, ent_coef=0.01, vf_coef=0.5))
    return _GRAD_CASES[name, B]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", NAMES)
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
    for name in NAMES:
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
