"""CPU checks of the PPO rule's options (gym_puzzles_amd/ppo.py): clip_range_vf against SB3's loss written
literally in float64 torch and differentiated by autograd, normalize_adv_ref against float64 torch and its
summation order, kl_stop_ref's strict comparison, and ppo_train_ref's target_kl stop against the loop
written by hand."""
from __future__ import annotations

import numpy as np
import pytest
from ppo_cases import (ARCHS, BATCHES, CV, KL_CASES, TRAIN_BATCH, TRAIN_EPOCHS, TRAIN_TOTAL, U, bits, kl_run, make_batch, make_old_values, make_params,
                       normalize_by_hand, torch_policy, train_data)

from gym_puzzles_amd import policy as P
from gym_puzzles_amd import ppo as R

NAMES = ("sb3-default", "odd-k-wide-head", "heads-only")
WRONG_VF = ("passes-where-clipped", "centred-on-zero")


# ---- clip_range_vf -----------------------------------------------------------------------------------
def sb3_loss_vf(model, batch, old_values, cv, clip, ent_coef, vf_coef, wrong=None):
    """SB3's PPO.train() loss with clip_range_vf, literally: ``values_pred = old_values + clamp(values -
    old_values, -clip_range_vf, clip_range_vf)``.  ``wrong`` plants one mistake: the gradient passed where the
    prediction is clipped (a straight-through clamp), or the clamp centred on 0 instead of old_values."""
    import torch
    import torch.nn.functional as F
    obs, actions, old, adv, ret = (torch.from_numpy(np.asarray(a, np.float64)) for a in batch)
    old_v = torch.from_numpy(np.asarray(old_values, np.float64))
    values, log_prob, entropy = model.evaluate_actions(obs, actions)
    values_pred = old_v + torch.clamp(values - old_v, -cv, cv)
    if wrong == "passes-where-clipped":
        values_pred = values + (values_pred - values).detach()
    if wrong == "centred-on-zero":
        values_pred = torch.clamp(values, -cv, cv)
    ratio = torch.exp(log_prob - old)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    value_loss = F.mse_loss(ret, values_pred)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    return loss, float(value_loss.detach()), values.detach().numpy(), values_pred.detach().numpy()


def majorant_vf(params, batch, old_values, cv, clip, ent_coef, vf_coef):
    """tests/ppo_cases.py's ``majorant`` with the value path's ``|v - ret|`` replaced by ``|vp - ret|`` (vp the
    clamped prediction) and widened by the three extra roundings of ``v - old_v``, the clamp's sum and ``vp -
    ret``: ``3 U (|v| + |old_v|)``.  A clipped sample's gradient is zero in both; the majorant keeps its
    term, which only widens the bound."""
    obs, actions, old, adv, ret = (np.asarray(a, np.float64) for a in batch)
    old_v = np.asarray(old_values, np.float64)
    B = obs.shape[0]
    f = (lambda x: np.tanh(x)) if params.activation == "tanh" else (lambda x: np.maximum(x, 0))
    ab = lambda wb: (np.abs(wb[0].astype(np.float64)), np.abs(wb[1].astype(np.float64)))  # noqa: E731

    def fwd(layers, x):
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
    n_fwd = sum(widths) + 2 * depth + 4 * params.act_dim + 8
    n_bwd = sum(widths) + 2 * depth + min(B, R.CHUNK) + -(-B // R.CHUNK) + 16
    d = actions - mean
    d_a = np.abs(d) + n_fwd * U * (np.abs(actions) + mean_a)
    vp = old_v + np.clip(v - old_v, -cv, cv)
    dvr_a = np.abs(vp - ret) + n_fwd * U * (v_a + np.abs(ret)) + 3 * U * (np.abs(v) + np.abs(old_v))
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
            grads[key, i] = (s_a.T @ inputs_a[i], s_a.sum(0))
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
    amp = 3.0 + terms_a.sum(1).max() + np.abs(lp - old).max()
    return np.concatenate(parts), n_bwd + amp * n_fwd


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_clip_range_vf_is_sb3(name, B):
    """ppo_grad_ref(clip_range_vf=) against autograd on SB3's loss in float64, under test_ppo.py's a-priori
    bound (n_bwd + amp * n_fwd) * U * majorant with the value path's majorant restated for the clamp."""
    clip, ent_coef, vf_coef = 0.2, 0.01, 0.5
    params = make_params(ARCHS[name], seed=3)
    batch = make_batch(params, B)
    old_v, cls = make_old_values(params, batch)
    grad, stats = R.ppo_grad_ref(params, *batch, clip_range=clip, ent_coef=ent_coef, vf_coef=vf_coef, old_values=old_v, clip_range_vf=CV)
    model = torch_policy(params)
    loss, want_vl, v64, vp64 = sb3_loss_vf(model, batch, old_v, CV, clip, ent_coef, vf_coef)
    loss.backward()
    want = np.concatenate([p.grad.numpy().ravel() for p in model.parameters()])
    # the classes are what they are meant to be, well away from the clamp's corners, under both signs of vp - ret
    dv = v64 - old_v
    for c, test in ((0, np.abs(dv) <= 0.51 * CV), (1, dv >= 1.49 * CV), (2, dv <= -1.49 * CV)):
        assert test[cls == c].all()
        if B >= 33:
            sign = (vp64 - batch[4]) > 0
            assert (sign & (cls == c)).any() and (~sign & (cls == c)).any(), f"class {c} holds both signs of vp - ret"
    maj, n_ops = majorant_vf(params, batch, old_v, CV, clip, ent_coef, vf_coef)
    bound = n_ops * U * maj
    err = np.abs(grad.astype(np.float64) - want)
    print(f"{name} B={B}: max |grad error| {err.max():.3e}, max error / bound {(err / np.maximum(bound, 1e-300)).max():.4f}, "
          f"max bound / max |grad| {bound.max() / np.abs(want).max():.3e}")
    assert (err <= bound).all()
    assert bound.max() < 5e-2 * np.abs(want).max()
    assert abs(float(stats[1]) - want_vl) <= n_ops * U * (4 * np.abs(batch[4]).max() ** 2 + 4 * want_vl)
    for wrong in WRONG_VF:
        if B == 1:
            continue                      # the one sample lies inside the range, where neither mistake shows
        model.zero_grad()
        sb3_loss_vf(model, batch, old_v, CV, clip, ent_coef, vf_coef, wrong=wrong)[0].backward()
        mistaken = np.concatenate([p.grad.numpy().ravel() for p in model.parameters()])
        excess = (np.abs(want - mistaken) / np.maximum(bound, 1e-300)).max()
        print(f"{name} B={B}: planted {wrong}: max |difference| / bound {excess:.1f}")
        assert excess > 2, wrong
    # without the option the rule is what it was: old_values alone changes nothing
    g0, s0 = R.ppo_grad_ref(params, *batch, clip_range=clip, ent_coef=ent_coef, vf_coef=vf_coef)
    g1, s1 = R.ppo_grad_ref(params, *batch, clip_range=clip, ent_coef=ent_coef, vf_coef=vf_coef, old_values=old_v)
    assert np.array_equal(bits(g0), bits(g1)) and np.array_equal(bits(s0), bits(s1))
    with pytest.raises(ValueError):
        R.ppo_grad_ref(params, *batch, clip_range_vf=CV)


def tie_case(name, B, cv=0.25, seed=3):
    """A minibatch whose every sample sits exactly on the clamp's edge: ``v - old_v == +cv`` (even n) or
    ``-cv`` (odd n) in float32.  Returns (params, batch, old_values at the tie, old_values just outside, cv)."""
    params = make_params(ARCHS[name], seed=seed)
    obs, actions, old, adv, ret = make_batch(params, 4 * B + 64, seed=6)
    v = P.values_ref(params, obs)
    sgn = np.where(np.arange(v.size) % 2 == 0, 1.0, -1.0).astype(np.float32)
    old_v = (v - sgn * np.float32(cv)).astype(np.float32)
    exact = np.flatnonzero((v - old_v) == sgn * np.float32(cv))
    keep = np.concatenate([exact[exact % 2 == 0][:(B + 1) // 2], exact[exact % 2 == 1][:B // 2]])
    keep.sort()
    assert keep.size == B, "enough samples whose tie is exact in float32"
    batch = tuple(a[keep] for a in (obs, actions, old, adv, ret))
    tie = old_v[keep]
    outside = (tie - sgn[keep] * np.float32(1e-3)).astype(np.float32)        # |v - old_v| just above cv
    return params, batch, tie, outside, cv


def test_clip_range_vf_ties_pass_the_gradient():
    """dv == +-cv exactly: the prediction is unclipped in value and the gradient passes (torch's clamp
    backward is inclusive), so the gradient equals the one under a range twice as wide bit for bit; just
    outside, the value path's gradient is zero."""
    params, batch, tie, outside, cv = tie_case("sb3-default", 33)
    dv = P.values_ref(params, batch[0]) - tie
    assert (dv[::2] == np.float32(cv)).any() and (dv == -np.float32(cv)).any() and (np.abs(dv) == np.float32(cv)).all()
    g_tie, s_tie = R.ppo_grad_ref(params, *batch, old_values=tie, clip_range_vf=cv)
    g_wide, s_wide = R.ppo_grad_ref(params, *batch, old_values=tie, clip_range_vf=2 * cv)
    assert np.array_equal(bits(g_tie), bits(g_wide)) and np.array_equal(bits(s_tie), bits(s_wide))
    g_out, _ = R.ppo_grad_ref(params, *batch, old_values=outside, clip_range_vf=cv)
    assert g_tie[-1] != 0 and g_out[-1] == 0, "the value head's bias gradient is the sum of dvalue"
    n_head = params.value[0].size + 1          # the value head is last in the flat order
    assert (g_out[-n_head:] == 0).all() and (g_tie[-n_head:] != 0).all()


# ---- normalize_adv_ref -------------------------------------------------------------------------------
NORM_SIZES = (2, 3, 31, 256, 257, 600, 4096)


def test_normalize_adv_ref_accuracy():
    import torch
    worst = 0.0
    for B in NORM_SIZES:
        for k, scale in enumerate(np.logspace(-3, 3, 20)):
            rng = np.random.default_rng(1000 * B + k)
            adv = ((rng.standard_normal(B) + rng.uniform(-2, 2)) * scale).astype(np.float32)
            got = R.normalize_adv_ref(adv)
            assert got.dtype == np.float32 and got.shape == (B,)
            a = torch.from_numpy(adv.astype(np.float64))
            want = ((a - a.mean()) / (a.std() + 1e-8)).numpy()
            ulp = np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
            worst = max(worst, float((np.abs(got.astype(np.float64) - want) / ulp).max()))
    print(f"normalize_adv_ref: max error {worst:.6f} float32 ulp against float64 torch")
    assert worst <= 0.501


def order_case():
    """600 advantages around 1 with +2^60 as the last sample of chunk 0 and -2^60 as the first of chunk 1:
    summed chunk by chunk, each chunk's small terms are absorbed by its large one and the mean is 0; in
    one sequential sum the large terms cancel first and chunk 1's small terms survive."""
    adv = (np.random.default_rng(0).standard_normal(600) + 1).astype(np.float32)
    adv[255], adv[256] = 2.0 ** 60, -2.0 ** 60
    return adv


def test_normalize_adv_ref_order_and_one_sample():
    """Chunks of 256 sequential, then the chunks sequential: pinned by an input on which one sequential
    sum over all samples gives other bits."""
    adv = order_case()
    got = R.normalize_adv_ref(adv)
    assert np.array_equal(bits(got), bits(normalize_by_hand(adv, 256)))
    assert not np.array_equal(bits(got), bits(normalize_by_hand(adv, 600))), "the input tells the chunk order from a flat sum"
    one = np.float32([3.25])
    out = R.normalize_adv_ref(one)
    assert np.array_equal(bits(out), bits(one)) and out is not one


def test_kl_stop_ref_is_strict():
    assert not R.kl_stop_ref(np.float32(0.75), 0.5)
    assert R.kl_stop_ref(np.nextafter(np.float32(0.75), np.float32(1)), 0.5)
    assert not R.kl_stop_ref(np.float32(0.0), 0.0) and R.kl_stop_ref(np.float32(1e-45), 0.0)
    assert not R.kl_stop_ref(np.float32(np.nan), 0.5)


# ---- ppo_train_ref with target_kl --------------------------------------------------------------------
def test_train_ref_target_kl():
    d = train_data()
    per_epoch = -(-TRAIN_TOTAL // TRAIN_BATCH)
    assert per_epoch == 5 and TRAIN_TOTAL - 4 * TRAIN_BATCH == 88
    stops = {}
    for case, (lr, target_kl) in KL_CASES.items():
        got, stats, state = kl_run(case)
        stop = stats.shape[0] - 1
        stops[case] = stop
        print(f"{case}: lr {lr}, target_kl {target_kl}: stops at minibatch {stop}, approx_kl {stats[:, 3]}")
        assert stats[0, 3] == 0, "unchanged parameters: the first minibatch's approx_kl is exactly 0"
        assert 0 < stop < TRAIN_EPOCHS * per_epoch - 1, "strictly after the first and before the last minibatch"
        assert R.kl_stop_ref(stats[stop, 3], target_kl) and not any(R.kl_stop_ref(k, target_kl) for k in stats[:stop, 3])
        assert state.t == stop
        # the loop by hand: `stop` applied steps, then one evaluation that is not applied
        st2 = R.AdamState(state.m.size)
        cur, k = d["params"], 0
        for order in d["epochs"]:
            for s in range(0, TRAIN_TOTAL, TRAIN_BATCH):
                if k > stop:
                    break
                mb = tuple(a[order[s:s + TRAIN_BATCH]] for a in d["data"])
                if k == stop:
                    _, s_k = R.ppo_grad_ref(cur, *mb, ent_coef=0.01)
                else:
                    cur, s_k = R.ppo_step_ref(cur, st2, mb, lr=lr, ent_coef=0.01)
                assert np.array_equal(bits(s_k), bits(stats[k])), (case, k)
                k += 1
        assert k == stop + 1 and st2.t == stop
        assert np.array_equal(bits(R.flatten_params(cur)), bits(R.flatten_params(got)))
        assert np.array_equal(bits(st2.m), bits(state.m)) and np.array_equal(bits(st2.v), bits(state.v))
    assert 0 < stops["first-epoch"] % per_epoch and stops["first-epoch"] < per_epoch, "mid-epoch, in the first epoch"
    assert stops["second-epoch"] >= per_epoch, "in an epoch after the first"
    # a target never reached is no target
    s_a, s_b = R.AdamState(R.flatten_params(d["params"]).size), R.AdamState(R.flatten_params(d["params"]).size)
    a, sa = R.ppo_train_ref(d["params"], s_a, d["data"], d["epochs"][:1], TRAIN_BATCH, lr=3e-4, target_kl=1e9)
    b, sb = R.ppo_train_ref(d["params"], s_b, d["data"], d["epochs"][:1], TRAIN_BATCH, lr=3e-4)
    assert np.array_equal(bits(R.flatten_params(a)), bits(R.flatten_params(b))) and np.array_equal(bits(sa), bits(sb)) and s_a.t == 5


def test_names_and_abi_of_the_options():
    import gym_puzzles_amd as G
    from gym_puzzles_amd import _native
    from gym_puzzles_amd import build as b
    for name in ("normalize_adv_ref", "kl_stop_ref", "ppo_train_ref", "ppo_grad_ref"):
        assert hasattr(G, name)
    for name in ("mrp_ppo_begin_device", "mrp_ppo_minibatch_device", "mrp_ppo_progress", "mrp_ppo_get_staged"):
        assert name in _native.EXPORTED, name
    assert b.UNITS[-1] == b.PPO_SOURCES[0] == ("mrp_ppo.hip", "mrp_ppo.hip.o", None)
