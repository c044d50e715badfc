"""What the device PPO update costs: one fused DevicePPO.step (forward, losses, backward, grad-norm
clip, Adam: mrp_ppo_step_device) against the same optimiser step as torch modules on the device.

For the v0 dims (obs 28, act 6), the two architectures of tools/policybench.py -- SB3's default (two
towers of 64, 64) and the reference's ppo-mrp-v0.json under SB3 1.x (a trunk of 256, 256) -- and
minibatches of 128 (the reference config's), 4096 and 16384 samples, two things are timed from the
same seeded parameters and minibatch:

    step         gym_puzzles_amd.ppo.DevicePPO.step: six launches, no host synchronisation
    torch_step   nn.Linear + activation modules, Normal.log_prob().sum / entropy, SB3's loss (torch.min,
                 torch.clamp, F.mse_loss), backward, clip_grad_norm_, torch.optim.Adam(eps=1e-5).step:
                 the update a user runs without the kernels

Each is timed with device events around `--inner` back-to-back calls per repetition; the figures are
the median and min-max over `--repeats` repetitions after `--warmup` untimed ones.  Before anything is
timed the tool asserts that one fused step on a 128-sample minibatch equals the numpy rule
(ppo_step_ref) bitwise: parameters, std and statistics.

    python tools/ppobench.py [--repeats 25] [--warmup 5] [--inner 10] [--out profiles/ppo_bench.json]

Needs a HIP device: without one nothing is timed and no file is written.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402
from trainbench import ACT, ARCHS, OBS, bench_params, bits, device_ms, lib_sha256, med, write_json  # noqa: E402

from gym_puzzles_amd import policy as P  # noqa: E402
from gym_puzzles_amd import ppo as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--inner", type=int, default=10, help="steps per timed repetition")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_bench.json"))
args = ap.parse_args()
if args.repeats < 20:
    ap.error("--repeats: at least 20")
if not torch.cuda.is_available():
    sys.exit("ppobench: no HIP device visible; nothing measured")

BATCHES = (128, 4096, 16384)
HP = dict(clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)
LR = 3e-4
dev = torch.device("cuda", 0)


def make_batch(params, B, seed):
    """Device tensors of a plausible minibatch: actions near the mean, ratios around 1, both advantage signs."""
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((B, OBS)).astype(np.float32)
    eps = rng.standard_normal((B, ACT)).astype(np.float32)
    pol = P.DevicePolicy.from_params(params)
    a, _, v, lp = pol.act(torch.from_numpy(obs).to(dev), eps=torch.from_numpy(eps).to(dev))
    old = lp + torch.from_numpy(rng.uniform(-0.3, 0.3, B).astype(np.float32)).to(dev)
    adv = torch.from_numpy(rng.standard_normal(B).astype(np.float32)).to(dev)
    ret = v + torch.from_numpy(rng.standard_normal(B).astype(np.float32)).to(dev)
    batch = tuple(t.contiguous() for t in (torch.from_numpy(obs).to(dev), a, old, adv, ret))
    torch.cuda.synchronize(dev)
    pol.close()
    return batch


class TorchPolicy(nn.Module):
    def __init__(self, params):
        super().__init__()

        def seq(layers):
            mods = []
            for w, b in layers:
                lin = nn.Linear(w.shape[1], w.shape[0])
                lin.weight.data.copy_(torch.from_numpy(w))
                lin.bias.data.copy_(torch.from_numpy(b))
                mods += [lin, nn.Tanh()]
            return nn.Sequential(*mods)
        self.log_std = nn.Parameter(torch.from_numpy(params.log_std.copy()))
        self.shared, self.pi, self.vf = seq(params.shared), seq(params.pi), seq(params.vf)
        self.action_net, self.value_net = seq([params.action])[0], seq([params.value])[0]

    def evaluate_actions(self, obs, actions):
        t = self.shared(obs)
        mean = self.action_net(self.pi(t))
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * self.log_std.exp())
        return self.value_net(self.vf(t)).flatten(), dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)


def torch_stepper(params, batch):
    model = TorchPolicy(params).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=LR, eps=1e-5)
    obs, actions, old, adv, ret = batch

    def step():
        values, log_prob, entropy = model.evaluate_actions(obs, actions)
        ratio = torch.exp(log_prob - old)
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - HP["clip_range"], 1 + HP["clip_range"])).mean()
        value_loss = F.mse_loss(ret, values)
        entropy_loss = -torch.mean(entropy)
        loss = policy_loss + HP["ent_coef"] * entropy_loss + HP["vf_coef"] * value_loss
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), HP["max_grad_norm"])
        opt.step()
    return step


res = {"device": torch.cuda.get_device_name(dev), "obs_dim": OBS, "act_dim": ACT, "repeats": args.repeats, "warmup": args.warmup,
       "steps_per_repeat": args.inner, "libmrp_sha256": lib_sha256(), "hyperparameters": dict(HP, learning_rate=LR), "rows": []}
timed = lambda fn: device_ms(fn, args.inner, args.warmup, args.repeats, dev)  # noqa: E731
for name, shared, pi, vf in ARCHS:
    params = bench_params(shared, pi, vf, seed=len(name))
    # the fused step is the rule, bitwise, on one minibatch
    small = make_batch(params, 128, seed=2)
    pol = P.DevicePolicy.from_params(params)
    ppo = R.DevicePPO(pol, learning_rate=LR, batch_size=128, **HP)
    stats = ppo.step(*small).cpu().numpy()
    got = pol.get_params()
    want, want_stats = R.ppo_step_ref(params, R.AdamState(ppo.n_params), tuple(t.cpu().numpy() for t in small), lr=LR, **HP)
    same = bool(np.array_equal(bits(R.flatten_params(got)), bits(R.flatten_params(want))) and np.array_equal(bits(got.std), bits(want.std))
                and np.array_equal(bits(stats), bits(want_stats)))
    assert same, f"{name}: the fused step differs from ppo_step_ref"
    ppo.close()
    pol.close()
    for B in BATCHES:
        batch = make_batch(params, B, seed=3)
        pol = P.DevicePolicy.from_params(params)
        ppo = R.DevicePPO(pol, learning_rate=LR, batch_size=B, **HP)
        st = torch.empty(5, dtype=torch.float32, device=dev)

        def fused():
            ppo.step(*batch, stats_out=st)

        tstep = torch_stepper(params, batch)
        f_ms, t_ms = timed(fused), timed(tstep)
        spread = max(max(f_ms) - min(f_ms), max(t_ms) - min(t_ms))
        res["rows"].append({"arch": name, "batch": B, "n_params": ppo.n_params, "ms": {"step": med(f_ms), "torch_step": med(t_ms)},
                            "ms_min_max": {"step": [min(f_ms), max(f_ms)], "torch_step": [min(t_ms), max(t_ms)]},
                            "torch_over_step": med(t_ms) / med(f_ms), "step_equals_ppo_step_ref": same,
                            "step_ahead_by_more_than_the_spread": bool(med(t_ms) - med(f_ms) > spread)})
        ppo.close()
        pol.close()
write_json(res, args.out)
