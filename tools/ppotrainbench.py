"""What a whole DevicePPO.train() call costs per minibatch: the device gather and advantage normalisation
(minibatch="device": one mrp_ppo_minibatch_device call per minibatch, 8 or 9 launches) against
minibatch="torch" (six index_select gathers, the torch normalisation and the six fused launches: about 17).

For the v0 dims (obs 28, act 6), the two architectures of tools/ppobench.py (towers 64, 64 and a trunk of
256, 256), minibatches of 128 and 4096, a 4096 x 6 rollout buffer (the reference config's) and a 128 x 4096
one, with normalize_advantage (SB3's default), one epoch per call.  Each train() call is timed twice over:
with device events around the call (the device's time from the first launch to the last) and as host wall
time from the call to a final synchronisation; both divided by the number of minibatches.  At B = 128 the
loop may be bound by the host's enqueueing, which the second figure shows.  The figures are the median
and min-max over `--repeats` calls after `--warmup` untimed ones, the convention of tools/ppobench.py.

    torch     minibatch="torch", no options: the code path train() had before the device gather existed
    device    minibatch="device"
    skipped   minibatch="device" after the stop: target_kl = 0 and old log-probs moved off the policy's, so
              the first minibatch stops the call and every later one is a predicated no-op (its kernels
              load `stopped` and return); the cost per skipped minibatch (the call's one evaluated
              minibatch is in the figure: with few minibatches per call it is an upper bound)

The learning rate is 0 so that every repetition does the same work on the same parameters.  Before
anything is timed the tool asserts that a "device" train() with normalize_advantage equals ppo_train_ref
bitwise on a small buffer: parameters, std and statistics.

    python tools/ppotrainbench.py [--repeats 25] [--warmup 3] [--out profiles/ppo_train_bench.json]

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
from trainbench import ACT, ARCHS, OBS, bench_params, bits, fill_buffer, lib_sha256, summary, write_json  # noqa: E402

from gym_puzzles_amd import policy as P  # noqa: E402
from gym_puzzles_amd import ppo as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--max-minibatches", type=int, default=64, help="minibatches per timed call at most (the buffer is cut to fit)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_train_bench.json"))
args = ap.parse_args()
if args.repeats < 20:
    ap.error("--repeats: at least 20")
if not torch.cuda.is_available():
    sys.exit("ppotrainbench: no HIP device visible; nothing measured")

BATCHES = (128, 4096)
BUFFERS = ((6, 4096), (128, 4096))          # n_steps x n_lanes: the reference config's rollout, and a long one
HP = dict(clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)
dev = torch.device("cuda", 0)


def self_check(params):
    T, N, bs = 5, 60, 128
    buf = fill_buffer(params, T, N, seed=4, dev=dev)
    pol = P.DevicePolicy.from_params(params)
    ppo = R.DevicePPO(pol, learning_rate=3e-4, n_epochs=2, batch_size=bs, normalize_advantage=True, minibatch="device", **HP)
    stats = ppo.train(buf, generator=torch.Generator(device="cpu").manual_seed(1)).cpu().numpy()
    g = torch.Generator(device="cpu").manual_seed(1)
    epochs = []
    for _ in range(2):
        perm = torch.randperm(T * N, generator=g).numpy()
        epochs.append((perm % T) * N + perm // T)
    h = lambda t: t.reshape(T * N, *t.shape[2:]).cpu().numpy()  # noqa: E731
    data = (h(buf.observations), h(buf.actions), h(buf.log_probs), h(buf.advantages), h(buf.returns))
    want, want_stats = R.ppo_train_ref(params, R.AdamState(ppo.n_params), data, epochs, bs, lr=3e-4, normalize_advantage=True, **HP)
    got = pol.get_params()
    same = bool(np.array_equal(bits(R.flatten_params(got)), bits(R.flatten_params(want))) and np.array_equal(bits(got.std), bits(want.std))
                and np.array_equal(bits(stats), bits(want_stats)))
    ppo.close()
    pol.close()
    return same


def timed(ppo, buf, n_minibatches):
    """(device ms, host wall ms) per minibatch of one train() call, `--repeats` times."""
    gen = torch.Generator(device="cpu").manual_seed(7)
    for _ in range(args.warmup):
        ppo.train(buf, generator=gen)
    torch.cuda.synchronize(dev)
    dev_ms, wall_ms = [], []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        ppo.train(buf, generator=gen)
        e1.record()
        torch.cuda.synchronize(dev)
        wall_ms.append((time.perf_counter() - t0) * 1e3 / n_minibatches)
        dev_ms.append(e0.elapsed_time(e1) / n_minibatches)
    return dev_ms, wall_ms


res = {"device": torch.cuda.get_device_name(dev), "obs_dim": OBS, "act_dim": ACT, "repeats": args.repeats, "warmup": args.warmup,
       "libmrp_sha256": lib_sha256(), "hyperparameters": dict(HP, learning_rate=0.0, normalize_advantage=True, n_epochs=1),
       "baseline": 'minibatch="torch" with no option set runs the code path train() had before the device gather existed',
       "rows": []}
for name, shared, pi, vf in ARCHS:
    params = bench_params(shared, pi, vf, seed=len(name))
    same = self_check(params)
    assert same, f'{name}: train(minibatch="device") differs from ppo_train_ref'
    for T, N in BUFFERS:
        for B in BATCHES:
            # cut the buffer's rows so that a timed call holds at most --max-minibatches minibatches
            rows = min(T, max(1, args.max_minibatches * B // N))
            n_mb = -(-rows * N // B)
            buf = fill_buffer(params, rows, N, seed=3, dev=dev)
            far = fill_buffer(params, rows, N, seed=3, dev=dev, lp_shift=0.5)
            row = {"arch": name, "buffer": [T, N], "rows_timed": rows, "batch": B, "minibatches_per_call": n_mb,
                   "device_equals_ppo_train_ref": same}
            for key, mode, kl, b in (("torch", "torch", None, buf), ("device", "device", None, buf), ("skipped", "device", 0.0, far)):
                pol = P.DevicePolicy.from_params(params)
                ppo = R.DevicePPO(pol, learning_rate=0.0, n_epochs=1, batch_size=B, normalize_advantage=True, minibatch=mode,
                                  target_kl=kl, **HP)
                d_ms, w_ms = timed(ppo, b, n_mb)
                if kl is not None:
                    assert ppo.stopped and ppo.n_applied == 0, "the first minibatch stops the call"
                row[key] = {"device_ms_per_minibatch": summary(d_ms), "wall_ms_per_minibatch": summary(w_ms)}
                ppo.close()
                pol.close()
            t, d = row["torch"], row["device"]
            row["torch_over_device"] = {k: t[k]["median"] / d[k]["median"] for k in ("device_ms_per_minibatch", "wall_ms_per_minibatch")}
            spread = max(x[k]["min_max"][1] - x[k]["min_max"][0] for x in (t, d) for k in ("wall_ms_per_minibatch",))
            row["device_ahead_by_more_than_the_spread"] = bool(t["wall_ms_per_minibatch"]["median"] - d["wall_ms_per_minibatch"]["median"] > spread)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
write_json(res, args.out)
