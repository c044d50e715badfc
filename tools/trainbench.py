"""What the training stack's benches share (ppobench, ppotrainbench, ppodistbench, policybench, gaebench,
normdistbench): the two bench architectures' parameters, a filled rollout buffer, the event-pair timing loop,
the median / min-max summary, the bit-pattern view and the JSON result with the library's sha256."""
import hashlib
import json
import os
import statistics

import numpy as np
import torch

from gym_puzzles_amd import policy as P
from gym_puzzles_amd._native import LIB_PATH
from gym_puzzles_amd.rollout import DeviceRolloutBuffer

OBS, ACT = 28, 6        # the v0 dims
ARCHS = (("sb3_default_pi64x2_vf64x2", [], [64, 64], [64, 64]), ("reference_shared256x2", [256, 256], [], []))
med = statistics.median


def bench_params(shared, pi, vf, seed, activation="tanh", obs_dim=OBS, act_dim=ACT):
    return P.random_params(obs_dim, act_dim, shared, pi, vf, activation, seed, 0.1, np.linspace(-0.5, 0.0, act_dim).astype(np.float32))


def fill_buffer(params, T, N, seed, dev, lp_shift=0.0):
    """A full buffer of plausible samples: the policy's own actions, values and log-probs (plus lp_shift)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    buf = DeviceRolloutBuffer(T, N, (OBS,), ACT, device=dev)
    pol = P.DevicePolicy.from_params(params)
    buf.observations.copy_(torch.randn(T, N, OBS, generator=g))
    for t in range(T):
        a, _, v, lp = pol.act(buf.observations[t].contiguous(), eps=torch.randn(N, ACT, generator=g).to(dev))
        buf.actions[t].copy_(a)
        buf.values[t].copy_(v)
        buf.log_probs[t].copy_(lp + lp_shift)
    buf.advantages.copy_(torch.randn(T, N, generator=g))
    buf.returns.copy_(buf.values + torch.randn(T, N, generator=g).to(dev))
    buf.pos, buf.full = T, True
    torch.cuda.synchronize(dev)
    pol.close()
    return buf


def device_ms(fn, inner, warmup, repeats, dev):
    """Milliseconds per call of ``fn``: device events around ``inner`` back-to-back calls, ``repeats`` times
    after ``warmup`` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        out.append(e0.elapsed_time(e1) / inner)
    return out


def summary(xs):
    return {"median": med(xs), "min_max": [min(xs), max(xs)]}


def bits(a, dtype=np.float32):
    """The unsigned view of an array or tensor converted to ``dtype``; ``dtype=None`` keeps the type it has."""
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def lib_sha256():
    with open(os.environ.get("MRP_LIB") or LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def write_json(res, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
