"""What the data-parallel split of DeviceVecNormalize.step() costs per step on one GPU: local phase / exchange /
apply phase (mrp_norm_local_device, dist.GradExchange with float64 blocks, mrp_norm_apply_device) against the
unsharded step (mrp_norm_step_device_ex, which stays in the library), and what the collective itself adds.

One process, the nccl backend at world size 1.  v0 dims: 4096 lanes x 28 observations, training on, every
optional output given.  Three variants, one after the other in every repetition (interleaved):

    unsharded    DeviceVecNormalize(...)                               2 launches
    copy         shard=Shard(0, 1, 4096): the copy-only exchange       3 launches and one 512-byte device copy
    collective   the same with force_collective=True                   3 launches and RCCL all_gather_into_tensor

A repetition times --inner steps of one variant between two HIP events on the current stream and divides by
--inner, in two modes: "device", where a spinning kernel goes first so that the host enqueues all the steps while
the device still spins and the events see device time alone, and "loop", the plain enqueueing loop (whichever of
host and device is the bottleneck).  From launch count the expected ratio copy : unsharded is about 3 : 2.  No
multi-rank exchange over xGMI runs on one GPU.  Before anything is timed the tool asserts that both sharded
variants give the unsharded statistics and outputs bit for bit.

    python tools/normdistbench.py [--repeats 25] [--warmup 3] [--inner 200] [--out profiles/norm_dist_bench.json]

Needs a HIP device: without one nothing is timed and no file is written.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
from trainbench import bits, lib_sha256, summary, write_json  # noqa: E402

from gym_puzzles_amd import DeviceVecNormalize  # noqa: E402
from gym_puzzles_amd.dist import Shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--inner", type=int, default=200, help="steps between the two events of one repetition")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_dist_bench.json"))
args = ap.parse_args()
if args.repeats < 20:
    ap.error("--repeats: at least 20")
if not torch.cuda.is_available():
    sys.exit("normdistbench: no HIP device visible; nothing measured")

LANES, OBS = 4096, 28
CASES = ("unsharded", "copy", "collective")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29518")
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)


def make(case):
    if case == "unsharded":
        return DeviceVecNormalize(LANES, OBS, 0)
    return DeviceVecNormalize(LANES, OBS, 0, shard=Shard(0, 1, LANES), force_collective=case == "collective")


class Step:
    """One normaliser with its own outputs over the shared inputs."""

    def __init__(self, case, inputs):
        self.norm, self.inputs = make(case), inputs
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
        self.outs = (z(LANES, OBS), z(LANES), z(LANES, OBS), z(LANES, dt=torch.float64), z(LANES, dt=torch.int32))
        self.norm.reset(inputs[0], self.outs[0])

    def __call__(self):
        obs, rew, done, term, rew64 = self.inputs
        o, r, t, epr, epl = self.outs
        self.norm.step(obs, rew, done, o, r, term, t, epr, epl, rew64)

    def state(self):
        torch.cuda.synchronize(dev)
        st = self.norm.get_stats()
        return [bits(x, None) for x in self.outs] + [np.atleast_1d(np.asarray(st[k], np.float64)).view(np.uint64) for k in sorted(st)]


g = torch.Generator(device="cpu").manual_seed(11)
inputs = (torch.randn(LANES, OBS, generator=g).to(dev), torch.randn(LANES, generator=g).to(dev),
          (torch.rand(LANES, generator=g) < 0.05).to(torch.uint8).to(dev), torch.randn(LANES, OBS, generator=g).to(dev),
          torch.randn(LANES, generator=g, dtype=torch.float64).to(dev))
steps = {case: Step(case, inputs) for case in CASES}
for _ in range(5):
    for case in CASES:
        steps[case]()
states = {case: steps[case].state() for case in CASES}
same = all(np.array_equal(x, y) for case in CASES[1:] for x, y in zip(states[case], states["unsharded"]))
assert same, "a sharded step at world size 1 differs from the unsharded step"


def timed(fn, sleep_cycles=0):
    """Microseconds per step of args.inner enqueued steps between two HIP events, and the host's share.  With
    sleep_cycles a spinning kernel goes first, so the host enqueues ahead of the device and the events see device
    time alone; the third value says whether the host did finish enqueueing before the spin ended."""
    es, e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    es.record()
    if sleep_cycles:
        torch.cuda._sleep(sleep_cycles)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(args.inner):
        fn()
    e1.record()
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / args.inner, host_ms * 1e3 / args.inner, es.elapsed_time(e0) >= host_ms


# the spin that covers the slowest variant's enqueueing twice over, in cycles of the device's sleep clock
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
torch.cuda._sleep(10_000_000)
e1.record()
torch.cuda.synchronize(dev)
cycles_per_ms = 10_000_000 / e0.elapsed_time(e1)
for _ in range(args.warmup):
    host = [timed(steps[case])[1] for case in CASES]
spin = int(2.0 * max(host) * 1e-3 * args.inner * cycles_per_ms)
loop, device, host_us, ahead = ({case: [] for case in CASES} for _ in range(4))
for _ in range(args.repeats):
    for case in CASES:               # interleaved: one repetition of each variant in turn, in both modes
        t, h, _ = timed(steps[case])
        loop[case].append(t)
        host_us[case].append(h)
        t, _, ok = timed(steps[case], spin)
        device[case].append(t)
        ahead[case].append(bool(ok))

res = {"device": torch.cuda.get_device_name(dev), "lanes": LANES, "obs_dim": OBS, "repeats": args.repeats, "warmup": args.warmup,
       "steps_per_repeat": args.inner, "libmrp_sha256": lib_sha256(),
       "timer": "HIP events around steps_per_repeat enqueued steps: device = behind a spinning kernel, so the host enqueues "
                "ahead; loop = the plain enqueueing loop",
       "backend": "nccl (RCCL) at world size 1; the collective case forces all_gather_into_tensor on device tensors",
       "not_measured": "no multi-rank RCCL exchange over xGMI has run", "sharded_equals_unsharded_bitwise": same,
       "launches": {"unsharded": 2, "copy": "3 + one device copy", "collective": "3 + all_gather_into_tensor"}}
for case in CASES:
    res[case] = {"device_us_per_step": summary(device[case]), "loop_us_per_step": summary(loop[case]),
                 "host_enqueue_us_per_step": summary(host_us[case]), "host_ran_ahead_in": f"{sum(ahead[case])}/{args.repeats}"}
for key in ("device_us_per_step", "loop_us_per_step"):
    m = {case: res[case][key]["median"] for case in CASES}
    res[key.replace("us_per_step", "ratios")] = {"copy_to_unsharded": m["copy"] / m["unsharded"],
                                                 "collective_to_unsharded": m["collective"] / m["unsharded"],
                                                 "collective_cost_us": m["collective"] - m["copy"]}
for s in steps.values():
    s.norm.close()
dist.destroy_process_group()
write_json(res, args.out)
