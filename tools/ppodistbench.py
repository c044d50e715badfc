"""What the data-parallel split of DevicePPO.train() costs per minibatch on one GPU: the local phase / exchange /
apply path (mrp_ppo_minibatch_device with d_grad, dist.GradExchange, mrp_ppo_apply_device) against the plain
minibatch="device" loop, and what the collective itself adds.

One process, the nccl backend at world size 1: with GradExchange(force_collective=True) the RCCL
all_gather_into_tensor runs on device tensors on the current stream.  The procedure, architectures and buffer
rows are tools/ppotrainbench.py's (v0 dims, towers 64, 64 and a trunk of 256, 256, minibatches of 128 and 4096,
a 6 x 4096 and a 128 x 4096 buffer cut to at most --max-minibatches minibatches per call, normalize_advantage,
learning rate 0, one epoch per call).  Per repetition the three cases are timed one after the other
(interleaved), as host wall time from the call to a final synchronisation, divided by the minibatches:

    plain        train(), minibatch="device"
    copy         the dist path with the copy-only exchange (world size 1: mine -> parts[0])
    collective   the dist path with the forced collective

The cost of the split (one more kernel, a second library call, one device copy) is copy - plain; the cost of
the collective is collective - copy.  No multi-rank exchange over xGMI runs here.  Before anything is timed
the tool asserts that both dist paths equal plain train() bitwise on a small buffer.

    python tools/ppodistbench.py [--repeats 25] [--warmup 3] [--out profiles/ppo_dist_bench.json]

Needs a HIP device: without one nothing is timed and no file is written.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
from trainbench import ACT, ARCHS, OBS, bench_params, bits, fill_buffer, lib_sha256, summary, write_json  # noqa: E402

from gym_puzzles_amd import policy as P  # noqa: E402
from gym_puzzles_amd import ppo as R  # noqa: E402
from gym_puzzles_amd.dist import GradExchange, Shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--max-minibatches", type=int, default=64, help="minibatches per timed call at most (the buffer is cut to fit)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_dist_bench.json"))
args = ap.parse_args()
if args.repeats < 20:
    ap.error("--repeats: at least 20")
if not torch.cuda.is_available():
    sys.exit("ppodistbench: no HIP device visible; nothing measured")

BATCHES = (128, 4096)
BUFFERS = ((6, 4096), (128, 4096))
HP = dict(clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)
CASES = ("plain", "copy", "collective")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29517")
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)


def make_ppo(params, case, B, lr):
    pol = P.DevicePolicy.from_params(params)
    ex = None if case == "plain" else GradExchange(Shard(0, 1, 1), pol.n_params + 5, dev, force_collective=case == "collective")
    return pol, R.DevicePPO(pol, learning_rate=lr, n_epochs=1, batch_size=B, normalize_advantage=True, minibatch="device", exchange=ex, **HP)


def self_check(params):
    buf = fill_buffer(params, 5, 60, seed=4, dev=dev)
    runs = []
    for case in CASES:
        pol, ppo = make_ppo(params, case, 128, 3e-4)
        stats = ppo.train(buf, generator=torch.Generator(device="cpu").manual_seed(1)).cpu().numpy()
        got = pol.get_params()
        runs.append([R.flatten_params(got), got.std, *ppo.state(), stats])
        ppo.close()
        pol.close()
    return all(np.array_equal(bits(x), bits(y)) for run in runs[1:] for x, y in zip(run, runs[0]))


def one_call(ppo, buf, gen, n_minibatches):
    t0 = time.perf_counter()
    ppo.train(buf, generator=gen)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / n_minibatches


res = {"device": torch.cuda.get_device_name(dev), "obs_dim": OBS, "act_dim": ACT, "repeats": args.repeats, "warmup": args.warmup,
       "libmrp_sha256": lib_sha256(), "hyperparameters": dict(HP, learning_rate=0.0, normalize_advantage=True, n_epochs=1),
       "backend": "nccl (RCCL) at world size 1; the collective case forces all_gather_into_tensor on device tensors",
       "not_measured": "no multi-rank RCCL exchange over xGMI has run", "rows": []}
for name, shared, pi, vf in ARCHS:
    params = bench_params(shared, pi, vf, seed=len(name))
    same = self_check(params)
    assert same, f"{name}: train() through the exchange differs from plain train()"
    for T, N in BUFFERS:
        for B in BATCHES:
            rows = min(T, max(1, args.max_minibatches * B // N))
            n_mb = -(-rows * N // B)
            buf = fill_buffer(params, rows, N, seed=3, dev=dev)
            objs = {case: make_ppo(params, case, B, 0.0) for case in CASES}
            gens = {case: torch.Generator(device="cpu").manual_seed(7) for case in CASES}
            for _ in range(args.warmup):
                for case in CASES:
                    one_call(objs[case][1], buf, gens[case], n_mb)
            wall = {case: [] for case in CASES}
            for _ in range(args.repeats):
                for case in CASES:           # interleaved: one call of each case per repetition
                    wall[case].append(one_call(objs[case][1], buf, gens[case], n_mb))
            row = {"arch": name, "buffer": [T, N], "rows_timed": rows, "batch": B, "minibatches_per_call": n_mb,
                   "dist_paths_equal_plain_train": same}
            for case in CASES:
                row[case] = {"wall_ms_per_minibatch": summary(wall[case])}
            m = {case: row[case]["wall_ms_per_minibatch"]["median"] for case in CASES}
            row["split_cost_ms"] = m["copy"] - m["plain"]
            row["collective_cost_ms"] = m["collective"] - m["copy"]
            for pol, ppo in objs.values():
                ppo.close()
                pol.close()
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
dist.destroy_process_group()
write_json(res, args.out)
