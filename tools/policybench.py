"""What the device policy costs: the fused mrp_policy_act_device launch against the same network as
torch modules on the device.

For the v0 dims (obs 28, act 6) at 4096 lanes and two architectures -- SB3's default (no trunk, two
towers of 64, 64) and the reference's ppo-mrp-v0.json under SB3 1.x (a trunk of 256, 256, no towers) --
three things are timed from the same seeded parameters, observations and noise:

    act          gym_puzzles_amd.policy.DevicePolicy.act: one launch of k_policy (forward, sample, clip,
                 log-prob, value)
    values       DevicePolicy.values: trunk + value tower + value head only
    torch_act    nn.Linear + activation modules, mean + std * eps, Normal(mean, std).log_prob(a).sum(-1),
                 clamp, and the value net: the composition a user runs without the kernel

Each is timed with device events around `--inner` back-to-back calls per repetition; the figures are
the median and min-max over `--repeats` repetitions after `--warmup` untimed ones.  The tool asserts
that the fused outputs equal policy_ref bitwise on its inputs (every 16th lane: the rule is per lane,
and the numpy fma chain of all 4096 would take minutes); the torch composition is another rounding
of the same network and is only checked to agree to 1e-4.

    python tools/policybench.py [--repeats 25] [--warmup 5] [--inner 20] [--out profiles/policy_bench.json]
                                [--lanes 4096] [--activation tanh|relu]   (diagnostics: other batch sizes, the tanh rule's share)

Needs a HIP device: without one nothing is timed and no file is written.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402
from trainbench import ACT, ARCHS, OBS, bench_params, bits, device_ms, lib_sha256, med, write_json  # noqa: E402

from gym_puzzles_amd import policy as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--inner", type=int, default=20, help="calls per timed repetition")
ap.add_argument("--lanes", type=int, default=4096)
ap.add_argument("--activation", default="tanh", choices=("tanh", "relu"), help="relu shows what the tanh rule costs")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_bench.json"))
args = ap.parse_args()
if args.repeats < 20:
    ap.error("--repeats: at least 20")
if not torch.cuda.is_available():
    sys.exit("policybench: no HIP device visible; nothing measured")

N = args.lanes
dev = torch.device("cuda", 0)


def torch_modules(params):
    def seq(layers):
        mods = []
        for w, b in layers:
            lin = nn.Linear(w.shape[1], w.shape[0])
            lin.weight.data.copy_(torch.from_numpy(w))
            lin.bias.data.copy_(torch.from_numpy(b))
            mods += [lin, nn.Tanh() if params.activation == "tanh" else nn.ReLU()]
        return mods
    trunk = nn.Sequential(*seq(params.shared)).to(dev)
    pi = nn.Sequential(*seq(params.pi), *seq([params.action])[:1]).to(dev)
    vf = nn.Sequential(*seq(params.vf), *seq([params.value])[:1]).to(dev)
    return trunk, pi, vf, torch.from_numpy(params.std).to(dev)


res = {"device": torch.cuda.get_device_name(dev), "obs_dim": OBS, "act_dim": ACT, "n_lanes": N, "activation": args.activation,
       "repeats": args.repeats,
       "warmup": args.warmup, "calls_per_repeat": args.inner, "libmrp_sha256": lib_sha256(), "archs": []}
ok = True
timed = lambda fn: device_ms(fn, args.inner, args.warmup, args.repeats, dev)  # noqa: E731
for name, shared, pi, vf in ARCHS:
    params = bench_params(shared, pi, vf, seed=len(name), activation=args.activation)
    rng = np.random.default_rng(1)
    obs, eps = rng.standard_normal((N, OBS)).astype(np.float32), rng.standard_normal((N, ACT)).astype(np.float32)
    d_obs, d_eps = torch.from_numpy(obs).to(dev), torch.from_numpy(eps).to(dev)
    pol = P.DevicePolicy.from_params(params)
    out = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in ((N, ACT), (N, ACT), (N,), (N,)))
    vout = torch.empty(N, dtype=torch.float32, device=dev)
    trunk, pnet, vnet, std = torch_modules(params)

    def fused():
        pol.act(d_obs, eps=d_eps, out=out)

    def values():
        pol.values(d_obs, out=vout)

    @torch.no_grad()
    def torch_act():
        t = trunk(d_obs)
        mean = pnet(t)
        a = mean + std * d_eps
        lp = torch.distributions.Normal(mean, std).log_prob(a).sum(-1)
        return a, a.clamp(-1.0, 1.0), vnet(t)[:, 0], lp

    fused()
    values()
    sub = slice(0, N, 16)
    want = P.policy_ref(params, obs[sub], eps[sub])
    same = all(np.array_equal(bits(g[sub].cpu().numpy()), bits(w)) for g, w in zip(out, want))
    same = bool(same and np.array_equal(bits(vout[sub].cpu().numpy()), bits(want[2])))
    assert same, f"{name}: the fused launch differs from policy_ref"
    tout = torch_act()
    close = all(bool(torch.allclose(g, t, rtol=1e-4, atol=1e-4)) for g, t in zip(out, tout))
    assert close, f"{name}: the torch composition is not the same network"
    f_ms, v_ms, t_ms = timed(fused), timed(values), timed(torch_act)
    spread = max(max(f_ms) - min(f_ms), max(t_ms) - min(t_ms))
    row = {"arch": name, "ms": {"act": med(f_ms), "values": med(v_ms), "torch_act": med(t_ms)},
           "ms_min_max": {"act": [min(f_ms), max(f_ms)], "values": [min(v_ms), max(v_ms)], "torch_act": [min(t_ms), max(t_ms)]},
           "torch_over_act": med(t_ms) / med(f_ms), "act_equals_policy_ref": same, "torch_agrees_1e-4": close,
           "act_ahead_by_more_than_the_spread": bool(med(t_ms) - med(f_ms) > spread)}
    ok = ok and row["act_ahead_by_more_than_the_spread"]
    res["archs"].append(row)
    pol.close()
res["ok"] = ok
write_json(res, args.out)
sys.exit(0 if ok else 1)
