"""One rank of a data-parallel DeviceVecNormalize run, for tests/test_ddp_norm_gpu.py:

    python -m torch.distributed.run --nproc-per-node=2 tools/norm_ddp_worker.py --plan DIR/plan.json --out DIR/ranks

Every rank uses device 0 and the gloo backend with the exchange of the column moments staged through pinned
host memory (host_stage=True; RCCL refuses two ranks on one device), so this shows correctness only.  The plan
lists cases {"lanes_per_rank", "obs_dim", "args", "script"} and an .npz of inputs over all world * lanes_per_rank
lanes with keys c<i>_obs0 and c<i>_s<k>_{obs,reward,done,term,reward64}; a script is a list of ["reset"],
["step", k] and ["training", flag].  A rank takes its lane slice of every input, runs each case through
DeviceVecNormalize(shard=...) and writes DIR/ranks/rank<r>.npz with, per call t of case i,
c<i>_t<t>_{obs_out,reward_out,term_out,ep_return,ep_len,stats,parts}: its outputs, the statistics vector
(obs mean, obs var, obs count, return mean, var, count) and the gathered parts as the exchange left them.
Last, rank 0 loads statistics with set_stats and every rank calls sync_from(0): sync_before / sync_after are the
statistics vectors around that call.

With --mismatch rank 1 builds its normaliser with norm_obs off: the first call must raise ValueError on every
rank before anything is enqueued; a rank then writes DIR/ranks/mismatch<r>.txt with the message and exits 0,
and exits 1 if nothing was raised.
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from gym_puzzles_amd import DeviceVecNormalize  # noqa: E402
from gym_puzzles_amd.dist import shard_from_env  # noqa: E402

STAT_KEYS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")


def stats_vector(norm):
    st = norm.get_stats()
    return np.concatenate([np.atleast_1d(np.asarray(st[k], np.float64)) for k in STAT_KEYS])


def run_case(i, case, data, shard, dev, out):
    L, D = case["lanes_per_rank"], case["obs_dim"]
    lanes = slice(shard.lane_offset, shard.lane_offset + L)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a[lanes])).to(dev)  # noqa: E731
    norm = DeviceVecNormalize(L, D, 0, shard=shard, host_stage=True, **case["args"])
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    t = 0
    for op in case["script"]:
        if op[0] == "training":
            norm.training = bool(op[1])
            continue
        rec = {}
        if op[0] == "reset":
            rec["obs_out"] = z(L, D)
            norm.reset(up(data[f"c{i}_obs0"]), rec["obs_out"])
        else:
            key = f"c{i}_s{op[1]}_"
            r64 = up(data[key + "reward64"]) if key + "reward64" in data else None
            rec.update(obs_out=z(L, D), reward_out=z(L), term_out=z(L, D), ep_return=z(L, dt=torch.float64), ep_len=z(L, dt=torch.int32))
            norm.step(up(data[key + "obs"]), up(data[key + "reward"]), up(data[key + "done"]), rec["obs_out"], rec["reward_out"],
                      up(data[key + "term"]), rec["term_out"], rec["ep_return"], rec["ep_len"], r64)
        for k, v in rec.items():
            out[f"c{i}_t{t}_{k}"] = v.cpu().numpy()
        out[f"c{i}_t{t}_stats"] = stats_vector(norm)
        out[f"c{i}_t{t}_parts"] = norm.exchange.parts.cpu().numpy()
        t += 1
    norm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--mismatch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("norm_ddp_worker: no HIP device visible")
    with open(args.plan) as f:
        plan = json.load(f)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    os.makedirs(args.out, exist_ok=True)
    try:
        if args.mismatch:
            L, D = 4, 3
            norm = DeviceVecNormalize(L, D, 0, shard=shard_from_env(L), host_stage=True)
            norm.norm_obs = rank != 1
            try:
                norm.reset(torch.zeros(L, D, device=dev), torch.zeros(L, D, device=dev))
            except ValueError as e:
                with open(os.path.join(args.out, f"mismatch{rank}.txt"), "w") as f:
                    f.write(str(e))
                norm.close()
                return
            sys.exit("norm_ddp_worker: the ranks' norm_obs differ and nothing was raised")
        out = {}
        with np.load(plan["inputs"]) as z:
            data = {k: z[k] for k in z.files}
        for i, case in enumerate(plan["cases"]):
            run_case(i, case, data, shard_from_env(case["lanes_per_rank"]), dev, out)
        # sync_from: rank 0 loads statistics (a resumed run), every rank takes them
        norm = DeviceVecNormalize(4, 3, 0, shard=shard_from_env(4), host_stage=True)
        if rank == 0:
            norm.set_stats({"obs_mean": [0.5, -2.0, 1e-300], "obs_var": [2.0, 0.25, 3.0], "obs_count": 1e6 + 0.5, "ret_mean": -0.75,
                            "ret_var": 1.5, "ret_count": 12345.0})
        out["sync_before"] = stats_vector(norm)
        norm.sync_from(0)
        out["sync_after"] = stats_vector(norm)
        norm.close()
        np.savez(os.path.join(args.out, f"rank{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
