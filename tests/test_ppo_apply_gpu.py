"""GPU checks of data-parallel PPO's apply phase in one process (csrc/mrp_ppo.hip: mrp_ppo_apply_device with
k_ppo_combine, mrp_ppo_set_state; DevicePPO.apply / set_state and train() through a GradExchange at world size
1): everything equals the numpy rule (gym_puzzles_amd/ppo.py combine_ref + adam_ref) on bit patterns."""
from __future__ import annotations

import numpy as np
import pytest
from ppo_cases import (ARCHS, HP, KL_CASES, PER_EPOCH, PERM_SEED, TRAIN_BATCH, TRAIN_EPOCHS, TRAIN_TOTAL, kl_run, make_batch, make_params, on_device,
                       perm_gen, same, same_run, snapshot, train_buffer)

from gym_puzzles_amd import policy as P
from gym_puzzles_amd import ppo as R
from gym_puzzles_amd.dist import GradExchange, Shard

pytestmark = pytest.mark.gpu

LR = 1e-3
NORMS = (0.01, 1e6, 0.01)      # max_grad_norm of the three steps: the gradient norm lies above, below, above


def _zeros(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.float32, device="cuda")


def _ref_step(cur, state, parts, n_params, max_norm):
    """combine_ref + adam_ref on the host copy of ``parts``: (new params, statistics row, clip factor)."""
    h = parts.cpu().numpy()
    grad, row = R.combine_ref(h[:, :n_params], h[:, n_params:n_params + 5])
    flat, coef = R.adam_ref(R.flatten_params(cur), grad, state, LR, max_norm)
    return R.unflatten_params(cur, flat, std=R.exp_ref(flat[:cur.act_dim])), row, float(coef)


def _check_state(pol, ppo, cur, state, what):
    got = pol.get_params()
    m, v = ppo.state()
    same(R.flatten_params(got), R.flatten_params(cur), f"{what}: parameters")
    same(got.std, cur.std, f"{what}: std")
    same(m, state.m, f"{what}: m")
    same(v, state.v, f"{what}: v")


# ---- apply against the rule --------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 33, 257))
@pytest.mark.parametrize("name", ["heads-only", "sb3-default", "width-one-towers"])
def test_apply_is_combine_and_adam(gpu_lib, name, B):
    """R local gradients by grad() on R different minibatches, written straight into the rows of ``parts``,
    then apply: three successive steps for R in (1, 2, 3, 4), the stride minimal (n_params + 5) for odd R
    and padded for even R, the padding NaN (it is never read).  sb3-default's 12 493 parameters are no
    multiple of the workgroup size, so the grid's tail holds parameters and the five statistics."""
    import torch
    params = make_params(ARCHS[name], seed=3)
    batches = [on_device(make_batch(params, B, seed=30 + i)) for i in range(4)]
    n = R.flatten_params(params).size
    if name == "sb3-default":
        assert n == 12493 and n % 64 and n % 256
    for ranks in (1, 2, 3, 4):
        pol = P.DevicePolicy.from_params(params)
        ppo = R.DevicePPO(pol, learning_rate=LR, batch_size=B, **HP)
        stride = n + 5 if ranks % 2 else -(-(n + 5) // 64) * 64 + 64
        parts = torch.full((ranks, stride), float("nan"), dtype=torch.float32, device="cuda")
        state, cur, coefs = R.AdamState(n), params, []
        for step, max_norm in enumerate(NORMS):
            for r in range(ranks):
                ppo.grad(*batches[(r + step) % 4], out=parts[r, :n], stats_out=parts[r, n:n + 5])
            ppo.max_grad_norm = max_norm
            stats = ppo.apply(parts)
            cur, row, coef = _ref_step(cur, state, parts, n, max_norm)
            coefs.append(coef)
            what = f"{name} B={B} R={ranks} step {step + 1}"
            same(stats, row, f"{what}: statistics row")
            _check_state(pol, ppo, cur, state, what)
            assert torch.isnan(parts[:, n + 5:]).all(), "the padding is not written"
        assert coefs[0] < 1 and coefs[1] == 1 and coefs[2] < 1, coefs
        assert (ppo.t, ppo.n_applied, ppo.stopped) == (3, 1, False) and state.t == 3
        ppo.close()
        pol.close()


# ---- hand-made parts ---------------------------------------------------------------------------------
def _hand_parts(n, stride, seed=2):
    """Three ranks' rows: small random gradients and statistics, with +2^60, 1, -2^60 in two rank orders
    (the sums are 0 and 1), rows of -0 (the sum stays -0 through the multiply) and x, -x, +0 (the sum is +0)
    both among the parameters, across the end of the first workgroup, and among the five statistics."""
    rng = np.random.default_rng(seed)
    h = np.full((3, stride), np.nan, np.float32)
    h[:, :n + 5] = (rng.standard_normal((3, n + 5)) * 0.01).astype(np.float32)
    big = np.float32(2.0 ** 60)
    for at in (0, 254, n):
        h[:, at], h[:, at + 1] = (big, 1.0, -big), (big, -big, 1.0)
        h[:, at + 2], h[:, at + 3] = -0.0, (7.5, -7.5, 0.0)
    h[:, n + 4] = -0.0
    return h


def test_apply_hand_made_parts(gpu_lib):
    import torch
    params = make_params(ARCHS["heads-only"], seed=3)
    n = R.flatten_params(params).size
    assert n > 300
    h = _hand_parts(n, n + 5 + 59)
    grad, row = R.combine_ref(h[:, :n], h[:, n:n + 5])
    assert grad[0] == 0 and grad[1] == np.float32(1.0) * np.float32(1.0 / 3) and np.signbit(grad[2]) and not np.signbit(grad[3])
    assert row[0] == 0 and row[1] == grad[1] and np.signbit(row[2]) and row[2] == 0 and not np.signbit(row[3]) and np.signbit(row[4])
    parts = torch.from_numpy(h).cuda()
    pol = P.DevicePolicy.from_params(params)
    ppo = R.DevicePPO(pol, learning_rate=LR, batch_size=8, max_grad_norm=1e6, **HP)
    stats = ppo.apply(parts)
    state = R.AdamState(n)
    cur, want_row, coef = _ref_step(params, state, parts, n, 1e6)
    assert coef == 1.0
    same(stats, want_row, "hand-made parts: the statistics row, signed zeros and the rank order included")
    same(stats, row, "the row")
    _check_state(pol, ppo, cur, state, "hand-made parts")
    same(parts, h, "parts is not written")
    # the other rank order of the same rows gives other bits
    swapped = torch.from_numpy(np.ascontiguousarray(h[[0, 2, 1]])).cuda()
    pol2 = P.DevicePolicy.from_params(params)
    ppo2 = R.DevicePPO(pol2, learning_rate=LR, batch_size=8, max_grad_norm=1e6, **HP)
    stats2 = ppo2.apply(swapped).cpu().numpy()
    assert stats2[0] == np.float32(1.0) * np.float32(1.0 / 3) and stats2[1] == 0
    assert pol2.get_params().log_std[0] != pol.get_params().log_std[0]
    # the predicate: approx_kl above 1.5 * target_kl = 0 stops the call before anything is written
    ppo2.target_kl = 0.0
    before = snapshot(pol2, ppo2)
    kl_parts = torch.from_numpy(h).cuda()
    kl_parts[:, n + 3] = 0.25
    out = torch.full((5,), 7.0, dtype=torch.float32, device="cuda")
    ppo2.apply(kl_parts, stats_out=out)
    want_out = R.combine_ref(kl_parts.cpu().numpy()[:, :n], kl_parts.cpu().numpy()[:, n:n + 5])[1]
    same(out, want_out, "the stopping call's combined row is recorded")
    assert (ppo2.t, ppo2.n_applied, ppo2.stopped) == (1, 0, True)
    same_run(snapshot(pol2, ppo2), before, "a stopped apply")
    for x in (ppo, ppo2, pol, pol2):
        x.close()


# ---- train() through the exchange at world size 1 ----------------------------------------------------
def _exchange(ppo_n_params, lanes):
    import torch
    return GradExchange(Shard(0, 1, lanes), ppo_n_params + 5, torch.device("cuda", 0))


@pytest.mark.parametrize("mode", ["device", "torch"])
def test_dist_train_at_world_one_equals_plain_train(gpu_lib, mode):
    """One rank through the two-phase path (local gradient into exchange.mine, the copy-only exchange,
    apply with R = 1) equals plain train() bitwise: with normalize_advantage, and under a target_kl that
    stops in the first epoch."""
    d, buf = train_buffer()
    n = R.flatten_params(d["params"]).size
    lr, target_kl = KL_CASES["first-epoch"]
    for kl, norm in ((None, True), (target_kl, False)):
        kw = dict(learning_rate=lr, n_epochs=TRAIN_EPOCHS, batch_size=TRAIN_BATCH, normalize_advantage=norm, target_kl=kl,
                  minibatch=mode, **HP)
        runs = []
        for dist_path in (False, True):
            pol = P.DevicePolicy.from_params(d["params"])
            ppo = R.DevicePPO(pol, exchange=_exchange(n, buf.n_lanes) if dist_path else None, **kw)
            stats = ppo.train(buf, generator=perm_gen())
            runs.append((snapshot(pol, ppo), stats.cpu().numpy(), (ppo.t, ppo.n_applied, ppo.stopped)))
            ppo.close()
            pol.close()
        what = f'"{mode}" target_kl={kl}'
        same_run(runs[1][0], runs[0][0], f"{what}: the dist path against plain train")
        same(runs[1][1], runs[0][1], f"{what}: statistics")
        assert runs[1][2] == runs[0][2], what
        if kl is not None:
            want, want_stats, state = kl_run("first-epoch")
            stop = want_stats.shape[0] - 1
            assert runs[1][2] == (stop, stop, True)
            same_run(runs[1][0], (R.flatten_params(want), want.std, state.m, state.v), f"{what}: against ppo_train_ref")
        else:
            assert runs[1][2] == (TRAIN_EPOCHS * PER_EPOCH, TRAIN_EPOCHS * PER_EPOCH, False)


def test_dist_train_predicate_and_a_following_train(gpu_lib):
    """target_kl = 0 on log-probs moved by 0.5: the first minibatch's apply stops the call.  Nothing after
    it is written: the parameters and moments, the later statistics rows, and exchange.mine, which still
    holds minibatch 0's local gradient and statistics.  A following train() works."""
    import torch
    d, buf = train_buffer()
    buf.log_probs.add_(0.5)
    n = R.flatten_params(d["params"]).size
    ex = _exchange(n, buf.n_lanes)
    pol = P.DevicePolicy.from_params(d["params"])
    ppo = R.DevicePPO(pol, learning_rate=LR, n_epochs=TRAIN_EPOCHS, batch_size=TRAIN_BATCH, normalize_advantage=False, target_kl=0.0,
                      minibatch="device", exchange=ex, **HP)
    stats = ppo.train(buf, generator=perm_gen()).cpu().numpy()
    assert (ppo.t, ppo.n_applied, ppo.stopped) == (0, 0, True)
    obs, actions, lp, adv, ret = d["data"]
    idx = d["epochs"][0][:TRAIN_BATCH]
    g0, s0 = R.ppo_grad_ref(d["params"], obs[idx], actions[idx], (lp + np.float32(0.5))[idx], adv[idx], ret[idx], **HP)
    assert s0[3] > 0
    same(stats[0], s0, "the stopping minibatch's row")
    assert not stats[1:].any(), "the rows after the stop stay zero"
    mine = ex.mine.cpu().numpy()
    same(mine[:n], g0, "exchange.mine holds minibatch 0's gradient")
    same(mine[n:n + 5], s0, "and its statistics")
    assert not mine[n + 5:].any()
    same(ex.parts.cpu().numpy()[0], mine, "parts is the copy of mine")
    zeros = np.zeros(n, np.float32)
    same_run(snapshot(pol, ppo), (R.flatten_params(d["params"]), d["params"].std, zeros, zeros), "a stopped train")
    # a following train on the same object, against plain train on fresh parameters
    ppo.target_kl, ppo.n_epochs = None, 1
    stats2 = ppo.train(buf, generator=perm_gen(PERM_SEED + 1))
    pol_b = P.DevicePolicy.from_params(d["params"])
    ppo_b = R.DevicePPO(pol_b, learning_rate=LR, n_epochs=1, batch_size=TRAIN_BATCH, normalize_advantage=False, minibatch="device", **HP)
    stats_b = ppo_b.train(buf, generator=perm_gen(PERM_SEED + 1))
    same(stats2, stats_b.cpu().numpy(), "a following train: statistics")
    same_run(snapshot(pol, ppo), snapshot(pol_b, ppo_b), "a following train")
    assert ppo.t == ppo_b.t == PER_EPOCH and not ppo.stopped
    assert TRAIN_TOTAL == buf.n_steps * buf.n_lanes and torch.isfinite(stats2).all()
    for x in (ppo, ppo_b, pol, pol_b):
        x.close()


# ---- set_state and arguments -------------------------------------------------------------------------
def test_set_state_round_trip_and_argument_errors(gpu_lib):
    params = make_params(ARCHS["sb3-default"], seed=3)
    n = R.flatten_params(params).size
    rng = np.random.default_rng(8)
    m, v = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) ** 2).astype(np.float32)
    m[0], m[1] = -0.0, 1e-42
    pol = P.DevicePolicy.from_params(params)
    ppo = R.DevicePPO(pol, learning_rate=LR, batch_size=8, **HP)
    ppo.set_state(m, v, 11)
    gm, gv = ppo.state()
    same(gm, m, "m after set_state")
    same(gv, v, "v after set_state")
    assert ppo.t == 11
    # the loaded state is the one the next step uses
    h = _hand_parts(n, n + 5)
    import torch
    ppo.max_grad_norm = 1e6
    ppo.apply(torch.from_numpy(h).cuda())
    state = R.AdamState(n)
    state.m, state.v, state.t = m.copy(), v.copy(), 11
    cur, _, _ = _ref_step(params, state, torch.from_numpy(h), n, 1e6)
    _check_state(pol, ppo, cur, state, "a step from a loaded state")
    assert ppo.t == 12
    with pytest.raises(ValueError):
        ppo.set_state(m[:-1], v, 0)
    with pytest.raises(ValueError):
        ppo.set_state(m, np.zeros(n + 1, np.float32), 0)
    before = snapshot(pol, ppo)
    good = _zeros(2, n + 5)
    bad_calls = [
        lambda: ppo.apply(_zeros(0, n + 5)),                         # R = 0
        lambda: ppo.apply(_zeros(65, n + 5)),                        # R = 65
        lambda: ppo.apply(_zeros(2, n + 4)),                         # a short stride
        lambda: ppo.apply(good.cpu()),                               # device
        lambda: ppo.apply(good.double()),                            # dtype
        lambda: ppo.apply(_zeros(2, 2 * (n + 5))[:, ::2]),           # contiguity
        lambda: ppo.apply(good.reshape(-1)),                         # shape
        lambda: ppo.apply(good, stats_out=_zeros(4)),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="R outside"):
        ppo.apply(_zeros(65, n + 5))
    with pytest.raises(ValueError, match="part_stride"):
        ppo.apply(_zeros(2, n + 4))
    with pytest.raises(ValueError, match="alias"):
        ppo.apply(good, stats_out=good[1, n:n + 5])                  # inside the last row
    with pytest.raises(ValueError, match="alias"):
        ppo.apply(good, stats_out=good[0, :5])
    big = _zeros(2 * (n + 5) + 5)
    ppo.apply(big[:2 * (n + 5)].reshape(2, n + 5), stats_out=big[2 * (n + 5):])     # adjacent is allowed
    assert ppo.t == 13
    with pytest.raises(ValueError):
        R.DevicePPO(pol, exchange=GradExchange(Shard(0, 1, 4), n, torch.device("cuda", 0)))   # too few floats
    same(ppo.state()[0], (np.float32(0.9) * before[2] + np.float32(0.0)).astype(np.float32), "a zero gradient decays m; the refused calls changed nothing")
    pol.close()
    with pytest.raises(ValueError, match="closed"):
        ppo.apply(good)
    with pytest.raises(ValueError, match="closed"):
        ppo.set_state(m, v, 0)
    ppo.close()
