"""What the rollout buffer's GAE costs: mrp_gae_device against the torch loop it replaces.

For each shape (T rows x N lanes) three things compute the same advantages and returns from the same
seeded inputs, TimeLimit bootstrap included:

    kernel      gym_puzzles_amd.rollout.gae_device: one launch of k_gae
    torch_loop  the recurrence as the loop of torch operations a user would write without the kernel,
                float64 accumulator included, so that its result equals gae_ref (asserted, bitwise)
    host        gae_ref in numpy, with the copies of the inputs to the host and of the results back

The first two are timed with device events around `--inner` back-to-back runs (kernel) or one run
(torch loop) per repetition, the third with a host clock around work that ends in a device
synchronise; each figure is the median over `--repeats` repetitions after `--warmup` untimed ones.
`kernel_GBps` is the bytes one launch has to move, (4 reads + 2 writes) * 4 B + 2 B per element, over
the kernel's time: information only (at 4096 x 6 one wave is mostly idle).

    python tools/gaebench.py [--repeats 25] [--warmup 5] [--inner 20] [--out profiles/gae_bench.json]

Shapes: 128 x 4096 (the project's lane count) and 4096 x 6 (the reference's ppo-mrp-v0.json: n_steps
4096, 6 envs).  Needs a HIP device: without one nothing is timed and no file is written.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from trainbench import bits, device_ms, lib_sha256, med, write_json  # noqa: E402

from gym_puzzles_amd.rollout import gae_device, gae_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--inner", type=int, default=20, help="kernel launches per timed repetition")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gae_bench.json"))
args = ap.parse_args()
if args.repeats < 20:
    ap.error("--repeats: at least 20")
if not torch.cuda.is_available():
    sys.exit("gaebench: no HIP device visible; nothing measured")

SHAPES = ((128, 4096), (4096, 6))
GAMMA, LAMBDA = 0.99, 0.95
dev = torch.device("cuda", 0)


def inputs(T, N, seed):
    rs = np.random.RandomState(seed)
    r, v = rs.standard_normal((T, N)).astype(np.float32), rs.standard_normal((T, N)).astype(np.float32)
    es = (rs.uniform(size=(T, N)) < 0.05).astype(np.uint8)
    lv, dones = rs.standard_normal(N).astype(np.float32), (rs.uniform(size=N) < 0.05).astype(np.uint8)
    ends = np.concatenate([es[1:], dones[None]])
    trunc = (ends.astype(bool) & (rs.uniform(size=(T, N)) < 0.5)).astype(np.uint8)
    return r, v, es, lv, dones, trunc, rs.standard_normal((T, N)).astype(np.float32)


def torch_loop(r, v, es, lv, dones, trunc, tv, adv):
    """gae_ref in torch operations; a Python scalar times a float32 tensor is a float32 product."""
    T = r.shape[0]
    r = torch.where(trunc.bool(), r + GAMMA * tv, r)
    esf = es.float()
    nnt = 1.0 - dones.double()
    last = (r[T - 1].double() + (GAMMA * lv).double() * nnt) - v[T - 1].double()
    adv[T - 1].copy_(last)
    for s in range(T - 2, -1, -1):
        nnt = 1.0 - esf[s + 1]
        delta = r[s] + GAMMA * v[s + 1] * nnt - v[s]
        last = delta.double() + ((GAMMA * LAMBDA) * nnt).double() * last
        adv[s].copy_(last)
    return adv, adv + v


def host_ms(fn):
    out = []
    for k in range(args.warmup + args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        if k >= args.warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


res = {"device": torch.cuda.get_device_name(dev), "gamma": GAMMA, "gae_lambda": LAMBDA, "repeats": args.repeats,
       "warmup": args.warmup, "kernel_launches_per_repeat": args.inner, "libmrp_sha256": lib_sha256(), "shapes": []}
ok = True
timed = lambda fn, inner: device_ms(fn, inner, args.warmup, args.repeats, dev)  # noqa: E731
for T, N in SHAPES:
    host_in = inputs(T, N, seed=T + N)
    r, v, es, lv, dones, trunc, tv = (torch.from_numpy(a).to(dev) for a in host_in)
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    adv_t = torch.empty_like(r)
    want = gae_ref(host_in[0], host_in[1], host_in[2].astype(np.float32), host_in[3], host_in[4], GAMMA, LAMBDA, host_in[5],
                   host_in[6])

    def kernel():
        gae_device(r, v, es, lv, dones, GAMMA, LAMBDA, trunc, tv, adv, ret)

    def loop():
        return torch_loop(r, v, es, lv, dones, trunc, tv, adv_t)

    def host():
        h = [t.cpu().numpy() for t in (r, v, es, lv, dones, trunc, tv)]
        a, b = gae_ref(h[0], h[1], h[2].astype(np.float32), h[3], h[4], GAMMA, LAMBDA, h[5], h[6])
        return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)

    kernel()
    la, lr = loop()
    same_k = bool(np.array_equal(bits(adv.cpu().numpy()), bits(want[0])) and np.array_equal(bits(ret.cpu().numpy()), bits(want[1])))
    same_t = bool(np.array_equal(bits(la.cpu().numpy()), bits(want[0])) and np.array_equal(bits(lr.cpu().numpy()), bits(want[1])))
    assert same_t, f"{T} x {N}: the torch loop does not reproduce gae_ref; it is not the same computation"
    assert same_k, f"{T} x {N}: mrp_gae_device differs from gae_ref"
    k_ms, t_ms, h_ms = timed(kernel, args.inner), timed(loop, 1), host_ms(host)
    nbytes = T * N * ((4 + 2) * 4 + 2)
    row = {"n_steps": T, "n_lanes": N,
           "ms": {"kernel": med(k_ms), "torch_loop": med(t_ms), "host_gae_ref_with_copies": med(h_ms)},
           "ms_min_max": {"kernel": [min(k_ms), max(k_ms)], "torch_loop": [min(t_ms), max(t_ms)],
                          "host_gae_ref_with_copies": [min(h_ms), max(h_ms)]},
           "torch_loop_over_kernel": med(t_ms) / med(k_ms), "bytes_per_launch": nbytes,
           "kernel_GBps": nbytes / (med(k_ms) * 1e-3) / 1e9, "kernel_equals_gae_ref": same_k,
           "torch_loop_equals_gae_ref": same_t, "kernel_ahead": bool(med(k_ms) < med(t_ms))}
    ok = ok and row["kernel_ahead"]
    res["shapes"].append(row)
res["ok"] = ok
write_json(res, args.out)
sys.exit(0 if ok else 1)
