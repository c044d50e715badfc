"""Data-parallel PPO executed: 2 ranks as fresh processes on the one GPU of the box.

tools/ppo_ddp_worker.py runs under torch.distributed.run on the gloo backend, both ranks on device 0, with
dist.GradExchange(host_stage=True): RCCL refuses two ranks on one device, so the gradient exchange is staged
through pinned host memory; everything else is the code a multi-GPU run executes (sync_from, the ranks' own
rollouts at their lane offsets, the local phase, the exchange, mrp_ppo_apply_device).  Each rank dumps its
buffer, sample orders and final state; here, on the CPU, the two final states must be bit-identical and equal
ppo.ppo_train_dist_ref replayed on the dumped buffers.  This shows correctness only: no multi-rank RCCL
exchange runs here.

This file sorts before the other GPU test files on purpose, and this pytest process never touches the GPU in
it: the ranks are started (fork + exec of a fresh interpreter) before this process has initialised the GPU.
"""
from __future__ import annotations

import numpy as np
import pytest
from ppo_cases import ARCHS, bits, make_params
from ranks import torchrun


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_ranks_train_identically_and_equal_the_rule(tmp_path):
    from gym_puzzles_amd import ppo as R
    out = tmp_path / "ranks"
    torchrun("tools/ppo_ddp_worker.py", 2, "--out", out, env=dict(MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    ranks = [np.load(out / f"rank{k}.npz") for k in range(2)]
    a, b = ranks
    assert int(a["lane_offset"]) == 0 and int(b["lane_offset"]) == 8
    # sync_from: both ranks start from rank 0's parameters, std, moments and step count
    for key in ("flat0", "std0", "m0", "v0"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    assert int(a["t0"]) == int(b["t0"]) == 3 and a["m0"].any() and a["v0"].any()
    # the ranks' rollouts differ (their own lanes, their own noise), their final states do not
    assert not np.array_equal(a["obs"], b["obs"]) and not np.array_equal(a["perms"], b["perms"])
    for key in ("flat", "std", "m", "v", "stats"):
        assert np.array_equal(bits(a[key]), bits(b[key])), f"the ranks' {key} differ"
    assert int(a["t"]) == int(b["t"]) == 3 + 8 and int(a["n_applied"]) == int(b["n_applied"]) == 8
    assert int(a["stopped"]) == int(b["stopped"]) == 0
    assert a["stats"].shape == (8, 5) and not np.array_equal(a["flat"], a["flat0"])
    # the replay by the rule
    like = make_params(ARCHS["sb3-default"], seed=0)
    assert R.flatten_params(like).size == a["flat0"].size
    params = R.unflatten_params(like, a["flat0"], std=a["std0"].copy())
    state = R.AdamState(a["flat0"].size)
    state.m, state.v, state.t = a["m0"].copy(), a["v0"].copy(), 3
    datas = [(k["obs"], k["actions"], k["log_probs"], k["advantages"], k["returns"]) for k in ranks]
    want, want_stats = R.ppo_train_dist_ref(params, state, datas, 2, 32, [list(k["perms"]) for k in ranks], normalize_advantage=True,
                                            target_kl=1e9, lr=1e-3, clip_range=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)
    assert state.t == 11
    for got, ref, what in ((a["stats"], want_stats, "statistics"), (a["flat"], R.flatten_params(want), "parameters"),
                           (a["std"], want.std, "std"), (a["m"], state.m, "m"), (a["v"], state.v, "v")):
        bad = np.flatnonzero(bits(got).ravel() != bits(ref).ravel())
        assert bad.size == 0, f"{what}: {bad.size} of {ref.size} differ from ppo_train_dist_ref, first at {bad[:5]}"
