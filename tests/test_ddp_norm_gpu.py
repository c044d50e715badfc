"""Data-parallel VecNormalize executed: 2 ranks as fresh processes on the one GPU of the box.

tools/norm_ddp_worker.py runs under torch.distributed.run on the gloo backend, both ranks on device 0, with the
float64 exchange staged through pinned host memory (host_stage=True: RCCL refuses two ranks on one device);
everything else is the code a multi-GPU run executes (the rank agreement check, mrp_norm_local_device, the
exchange, mrp_norm_apply_device).  Each rank takes its lane slice of inputs written here and dumps, per call, its
outputs, its statistics and the gathered parts.  Here, on the CPU: (a) the two ranks' statistics are the same
bits after every call, (b) moments_combine_ref + rms_merge_ref on the dumped parts and the previous statistics
reproduce them, (c) the concatenated outputs pass vecnorm_exact.judge against the exact rule over all 2 L lanes,
(d) ranks that disagree on norm_obs both raise ValueError and nothing hangs.  This shows correctness only: no
multi-rank RCCL exchange runs here.

In (b) a NaN statistic is compared as NaN, not by its bits: the sign and payload of a NaN that arithmetic
produces are the processor's (x86 gives the negative default NaN, the GPU the positive one), not the rule's.

This file sorts before the in-process GPU test files on purpose, and this pytest process never touches the GPU
in it: the ranks are started (fork + exec of a fresh interpreter) before this process has initialised the GPU.
"""
from __future__ import annotations

import json

import numpy as np
import pytest
import vecnorm_exact as ve
from ranks import torchrun

STAT_KEYS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")


def _launch(tmp_path, *extra):
    out = tmp_path / "ranks"
    torchrun("tools/norm_ddp_worker.py", 2, "--plan", tmp_path / "plan.json", "--out", out, *extra,
             env=dict(MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    return out


def _stats_dict(vec, D):
    return {"obs_mean": vec[:D], "obs_var": vec[D:2 * D], "obs_count": vec[2 * D], "ret_mean": vec[2 * D + 1],
            "ret_var": vec[2 * D + 2], "ret_count": vec[2 * D + 3]}


def _stats_vec(st):
    return np.concatenate([np.atleast_1d(np.asarray(st[k], np.float64)) for k in STAT_KEYS])


def _cases():
    """(lanes per rank, D, constructor arguments, inputs over 2 L lanes, script)"""
    from vecnorm_dist import two_rank_nonfinite_inputs
    return [(1, 28, ve.CLIPPED, ve.make_inputs(2, 28, 6001), ve.plain_script()),
            (65, 3, ve.DEFAULTS, two_rank_nonfinite_inputs(), ve.plain_script()),
            (257, 7, ve.DEFAULTS, ve.make_inputs(514, 7, 6003, n_steps=8, with_reward64=True), ve.eval_script())]


def _write_plan(tmp_path, cases):
    data, plan = {}, {"inputs": str(tmp_path / "inputs.npz"), "cases": []}
    for i, (L, D, args, inputs, script) in enumerate(cases):
        data[f"c{i}_obs0"] = inputs["obs0"]
        for k, s in enumerate(inputs["steps"]):
            for name, v in s.items():
                if v is not None:
                    data[f"c{i}_s{k}_{name}"] = v
        plan["cases"].append({"lanes_per_rank": L, "obs_dim": D, "args": args, "script": [list(op) for op in script]})
    np.savez(plan["inputs"], **data)
    with open(tmp_path / "plan.json", "w") as f:
        json.dump(plan, f)


def _same_or_both_nan(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_two_ranks_hold_one_set_of_statistics(tmp_path):
    from vecnorm_dist import column0, replay_update
    cases = _cases()
    _write_plan(tmp_path, cases)
    out = _launch(tmp_path)
    ranks = [np.load(out / f"rank{k}.npz") for k in range(2)]
    # sync_from(0): rank 1 started from the initial statistics and holds rank 0's loaded ones afterwards, bit for bit
    a, b = ranks
    assert a["sync_before"][6] == 1e6 + 0.5 and b["sync_before"][6] == 1e-4 and a["sync_before"][2] == 1e-300
    for k in ranks:
        assert np.array_equal(k["sync_after"].view(np.uint64), a["sync_before"].view(np.uint64)), "sync_from"
    for i, (L, D, args, inputs, script) in enumerate(cases):
        calls = [op for op in script if op[0] != "training"]
        training, prev, got = True, None, []
        t = 0
        for op in script:
            if op[0] == "training":
                training = op[1]
                continue
            w = f"case {i} call {t}"
            sa, sb = (k[f"c{i}_t{t}_stats"] for k in ranks)
            assert sa.shape == (2 * D + 4,) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64)), f"{w}: (a) statistics differ"
            pa, pb = (k[f"c{i}_t{t}_parts"] for k in ranks)
            assert pa.shape == (2, 64 * -(-2 * (D + 1) // 64)) and np.array_equal(pa.view(np.uint64), pb.view(np.uint64)), f"{w}: parts"
            # (b) the rule on the gathered parts and the previous statistics
            if prev is None:
                prev = _stats_vec({"obs_mean": np.zeros(D), "obs_var": np.ones(D), "obs_count": 1e-4, "ret_mean": 0.0,
                                   "ret_var": 1.0, "ret_count": 1e-4})
            with np.errstate(all="ignore"):
                want = _stats_vec(replay_update(_stats_dict(prev, D), pa, L, obs=training, ret=training and op[0] == "step"))
            assert _same_or_both_nan(sa, want), f"{w}: (b) the replay of the rule differs at {np.flatnonzero(sa != want)}"
            if not training:
                assert np.array_equal(sa.view(np.uint64), prev.view(np.uint64)), f"{w}: statistics moved in evaluation mode"
            prev = sa
            rec = {"stats": _stats_dict(sa, D)}
            for k in ("obs_out", "reward_out", "term_out", "ep_return", "ep_len"):
                if f"c{i}_t{t}_{k}" in ranks[0]:
                    rec[k] = np.concatenate([ranks[0][f"c{i}_t{t}_{k}"], ranks[1][f"c{i}_t{t}_{k}"]])
            got.append(rec)
            t += 1
        assert t == len(calls)
        # (c) the exact rule over all 2 L lanes
        if i != 1:
            exact = ve.exact_records(("ddp", i), inputs, args, script)
            worst = ve.judge(got, exact, *ve.clips(args), where=f"case {i}")
            print(f"two ranks, case {i}, worst error / bound:", {k: float(f"{v:.3g}") for k, v in worst.items()})
            continue
        # the non-finite case: NaN exactly where numpy's rule over the 130 lanes has it, on rank 0's lanes too;
        # column 0 within the exact bounds; counts and Monitor as numpy's
        from oracle.vecnorm_ref import VecNormalizeRef
        ref = ve.run_script(ve.RefAdapter(VecNormalizeRef(2 * L, D)), inputs, script)
        exact = ve.exact_records(("ddp-col0",), column0(inputs), args, script)
        for t, (g, q, e) in enumerate(zip(got, ref, exact)):
            flat = lambda x: {**{k: v for k, v in x.items() if k != "stats" and v is not None}, **x["stats"]}  # noqa: E731
            fg, fq = flat(g), flat(q)
            for k in fg:
                a, b = np.asarray(fg[k], np.float64), np.asarray(fq[k], np.float64)
                if k in ("term_out", "ep_return", "ep_len"):
                    m = inputs["steps"][t - 1]["done"].astype(bool)
                    a, b = a[m], b[m]
                assert np.array_equal(np.isnan(a), np.isnan(b)), f"case 1 call {t}: NaN positions of {k}"
                assert np.array_equal(np.isinf(a), np.isinf(b)), f"case 1 call {t}: infinities of {k}"
                if k in ("ep_return", "ep_len", "obs_count", "ret_count"):
                    assert np.array_equal(a, b, equal_nan=True), f"case 1 call {t}: {k}"
            assert np.isnan(g["obs_out"][:L, 1]).all() == (t >= 2), "rank 0's lanes follow the NaN that entered on rank 1"
            for k in ("obs_mean", "obs_var"):
                ve.check_stats(g["stats"][k][:1], e["stats"][k], e["stat_bounds"][k], f"case 1 call {t} {k}")
            z, prop, tot = e["obs"]
            ve.check_outputs(np.ascontiguousarray(g["obs_out"][:, :1]), z, tot, 10.0, f"case 1 call {t} obs_out", prop=prop)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_ranks_that_disagree_on_norm_obs_both_raise(tmp_path):
    """(d): rank 1 has norm_obs off.  The agreement check raises ValueError on both ranks before anything is
    enqueued; both exit (the launch has its own time limit, and the ranks' process group one of 60 s)."""
    _write_plan(tmp_path, [])
    out = _launch(tmp_path, "--mismatch")
    for k in range(2):
        msg = (out / f"mismatch{k}.txt").read_text()
        assert "DeviceVecNormalize.reset" in msg and "differs across ranks" in msg and "True" in msg and "False" in msg, msg
