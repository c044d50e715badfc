"""One rank of a data-parallel PPO iteration, for tests/test_ddp_ppo_gpu.py:

    python -m torch.distributed.run --nproc-per-node=2 tools/ppo_ddp_worker.py --out DIR

Every rank uses device 0 and the gloo backend with the gradient exchange staged through pinned host memory
(RCCL refuses two ranks on one device), so this shows correctness only.  A rank builds MultiRobotPuzzle-v0
with 8 lanes at its lane_offset and a DevicePolicy (towers 64, 64) from parameters of its own, takes rank 0's
parameters and optimiser state with sync_from(0), collects a 16-step rollout and trains 2 epochs at batch 32
(minibatch="device", normalize_advantage, a target_kl never reached).  It writes DIR/rank<r>.npz: the state
after sync_from, the buffer's fields (row-major [T * N]), the epochs' sample orders, and the final flat
parameters, std, m, v, t and statistics, for a replay by ppo.ppo_train_dist_ref on the host.
"""
import argparse
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
from trainbench import bench_params  # noqa: E402

from gym_puzzles_amd import DeviceRolloutBuffer, MultiRobotPuzzleVecEnv  # noqa: E402
from gym_puzzles_amd import policy as P  # noqa: E402
from gym_puzzles_amd import ppo as R  # noqa: E402
from gym_puzzles_amd.dist import GradExchange, shard_from_env  # noqa: E402
from gym_puzzles_amd.rollout import collect_rollouts  # noqa: E402

LANES, T, EPOCHS, BATCH = 8, 16, 2, 32
HP = dict(learning_rate=1e-3, clip_range=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppo_ddp_worker: no HIP device visible")
    shard = shard_from_env(LANES)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=shard.rank, world_size=shard.world, timeout=datetime.timedelta(seconds=60))
    try:
        env = MultiRobotPuzzleVecEnv("MultiRobotPuzzle-v0", LANES, seed=3, lane_offset=shard.lane_offset, max_episode_steps=5)
        O, A = env.observation_space.shape[0], env.action_space.shape[0]
        pol = P.DevicePolicy.from_params(bench_params([], [64, 64], [64, 64], 10 + shard.rank, obs_dim=O, act_dim=A), seed=77, lane_offset=shard.lane_offset)
        n = pol.n_params
        ppo = R.DevicePPO(pol, n_epochs=EPOCHS, batch_size=BATCH, normalize_advantage=True, target_kl=1e9, minibatch="device",
                          exchange=GradExchange(shard, n + 5, dev, host_stage=True), **HP)
        if shard.rank == 0:          # an optimiser state worth broadcasting
            rng = np.random.default_rng(1)
            ppo.set_state((rng.standard_normal(n) * 1e-3).astype(np.float32), (rng.standard_normal(n) ** 2 * 1e-6).astype(np.float32), 3)
        ppo.sync_from(0)
        start = pol.get_params()
        m0, v0 = ppo.state()
        out = {"flat0": R.flatten_params(start), "std0": start.std, "m0": m0, "v0": v0, "t0": np.int64(ppo.t)}
        buf = DeviceRolloutBuffer(T, LANES, (O,), A, device=0, gamma=0.99, gae_lambda=0.95)
        obs0 = torch.from_numpy(env.reset()).to(dev)
        collect_rollouts(env, pol, buf, obs0, torch.ones(LANES, dtype=torch.uint8, device=dev))
        fields = buf.flat_fields()
        for name, f in zip(("obs", "actions", "values", "log_probs", "advantages", "returns"), fields):
            out[name] = f.cpu().numpy()
        seed = 100 + shard.rank
        stats = ppo.train(buf, generator=torch.Generator(device="cpu").manual_seed(seed))
        g = torch.Generator(device="cpu").manual_seed(seed)
        perms = []
        for _ in range(EPOCHS):
            perm = torch.randperm(T * LANES, generator=g).numpy()
            perms.append((perm % T) * LANES + perm // T)
        end = pol.get_params()
        m, v = ppo.state()
        out.update(perms=np.stack(perms), flat=R.flatten_params(end), std=end.std, m=m, v=v, t=np.int64(ppo.t),
                   n_applied=np.int64(ppo.n_applied), stopped=np.int64(ppo.stopped), stats=stats.cpu().numpy(),
                   lane_offset=np.int64(shard.lane_offset))
        os.makedirs(args.out, exist_ok=True)
        np.savez(os.path.join(args.out, f"rank{shard.rank}.npz"), **out)
        dist.barrier()
        for x in (ppo, pol, env):
            x.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
