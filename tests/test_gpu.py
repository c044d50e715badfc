"""GPU parity tests: the HIP step (libmrp.so, through the C ABI) against the CPU oracle.

The bar is bit-exactness: the engine runs float32 with the same operation order as the
oracle (both built without FMA contraction), so obs, reward, done and every body's state must
be identical, not merely close.  Sizes: small lane counts over hundreds of steps for the
step-by-step comparisons, and BASELINE.json's 4096 lanes for the device auto-reset path
(final state + reward sums vs the oracle's multi-threaded batch runner).
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from gym_puzzles_amd.spawn import draw_bounds, reference_draws

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENVS = range(7)
# MultiRobotPuzzle2 / MultiRobotPuzzleHeavy2(num_agents = 1, 3, 4, 5) (multi_robot_puzzle_02.py:139) and
# RobotPuzzleBase(num_agents = 1, 3, 4, 5[, heavy=True]) (core.py:88)
AGENT_VARIANTS = range(7, 23)


@pytest.fixture(scope="module")
def orc(oracle_lib):
    from oracle import oracle
    return oracle


def _eq(name, g, c):
    g, c = np.asarray(g), np.asarray(c)
    bad = ~((g == c) | (np.isnan(g) & np.isnan(c)))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} elements differ, first at {i}: gpu {g[i]!r} oracle {c[i]!r}")


@pytest.mark.parametrize("env_id", list(ENVS) + list(AGENT_VARIANTS))
def test_step_parity_host_inputs(gpu_lib, orc, env_id):
    """64 lanes x 200 steps with host spawns/actions; finished lanes reset through the mask."""
    _host_input_parity(orc, env_id, 64, 200)


@pytest.mark.parametrize("env_id", [0, 1])
def test_step_parity_block_angle_ranges(gpu_lib, orc, env_id):
    """v0 / Heavy-v0 blocks spawned at angles around and far beyond 120 rad (glibc's sinf / cosf switch
    to the Payne-Hanek reduction there), and at +-0 and tiny angles: the device's rot() evaluates the
    straight-line fast form (valid below 120 rad) on every lane and replaces its result through glibc's
    other branches on the lanes at 120 rad or more, so every lane stays bit-exact against the oracle."""
    angles = np.r_[np.linspace(118.5, 121.5, 24), np.linspace(-121.5, -118.5, 16),
                   [0.0, -0.0, 1e-5, -1e-5, 2.0 ** -12, 0.78539816, 125.0, -125.0, 250.0, -250.0, 1e3, -1e3,
                    1e4, 3e4, 7.5e4, -7.5e4, 1e5, 4.0e5, 8.0e5, 1.6e6, 1e6, -1e6, 3.3e6, 5.4e6]]

    def spawn_angle(draws):
        draws[:, 2] = angles[:len(draws)]   # v0 / Heavy-v0 draw order: block x, y, angle, then agents
        return draws
    _host_input_parity(orc, env_id, 64, 120, draws_fn=spawn_angle)


def _host_input_parity(orc, env_id, lanes, steps, draws_fn=None):
    from gym_puzzles_amd import Batch
    rs_d = [np.random.RandomState(17 + l) for l in range(lanes)]
    rs_a = np.random.RandomState(1017)
    b = Batch(env_id, lanes)
    envs = [orc.OracleEnv(env_id) for _ in range(lanes)]
    draws = np.stack([reference_draws(env_id, r) for r in rs_d])
    if draws_fn is not None:
        draws = draws_fn(draws)
    acts = rs_a.uniform(-1, 1, size=(lanes, b.act_dim)).astype(np.float32)
    _eq("reset obs", b.reset(draws, acts), np.stack([o.reset(draws[l], acts[l]) for l, o in enumerate(envs)]).astype(np.float32))
    for t in range(steps):
        a = rs_a.uniform(-1, 1, size=(lanes, b.act_dim)).astype(np.float32)
        obs, rew, done, trunc = b.step(a)
        res = [o.step(a[l]) for l, o in enumerate(envs)]
        # Known divergence (advisor r5): the oracle takes the reference's distance() with glibc pow for
        # `** 2` / `** 0.5` (CPython's float_pow), the device with a multiply and sqrt; the float64
        # distance differs by 1 ulp on rare inputs (pinned on CPU: tests/test_v2_env_layer.py::
        # test_distance_pow_semantics_known_case, where both round to the same float32).  The float32
        # obs entries derived from distances are compared bit for bit here; a mismatch would need that
        # 1-ulp difference to straddle a float32 rounding boundary.
        _eq(f"obs@{t}", obs, np.stack([r[0] for r in res]).astype(np.float32))
        _eq(f"reward@{t}", rew, np.array([r[1] for r in res]).astype(np.float32))
        # float64 reward (the reference's Python float): the device takes distances with sqrt where
        # CPython's `** 0.5` calls libm pow (1 ulp apart for ~0.1 % of inputs), so the float64 value
        # carries a 1e-12 tolerance; its float32 rounding is the bit-exact `reward` above
        r64 = np.array([r[1] for r in res], np.float64)
        np.testing.assert_allclose(b.reward64, r64, rtol=1e-12, atol=1e-9, err_msg=f"reward64@{t}")
        _eq(f"reward64->f32@{t}", b.reward64.astype(np.float32), rew)
        _eq(f"done@{t}", done, np.array([r[2] for r in res], np.uint8))
        _eq(f"status@{t}", b.status, np.array([r[3] for r in res], np.uint8))
        _eq(f"bodies@{t}", b.bodies(), np.stack([o.bodies() for o in envs]))
        fl = b.flags()
        _eq(f"flags@{t}", fl, np.stack([np.r_[o.flags()[0], o.flags()[1]] for o in envs]).astype(np.int32))
        fin = done.astype(bool) | trunc.astype(bool)
        if fin.any():
            d2 = np.stack([reference_draws(env_id, r) for r in rs_d])
            a2 = rs_a.uniform(-1, 1, size=(lanes, b.act_dim)).astype(np.float32)
            o2 = b.reset(d2, a2, mask=fin).copy()
            for l in np.nonzero(fin)[0]:
                _eq(f"reset obs@{t} lane {l}", o2[l], envs[l].reset(d2[l], a2[l]).astype(np.float32))
    toi = sum(o.counters()[0] for o in envs)
    pos = sum(o.counters()[1] for o in envs)
    assert b.counters() == (toi, pos)
    assert not b.faults().any(), "a loop guard tripped"
    # per-batch counters (mrp_counters_ex) against the oracle's
    ctr = b.counters_ex()
    oc = [o.counters_ex() for o in envs]
    assert ctr["toi_events"] == toi and ctr["position_iterations"] == pos
    assert ctr["touching_contacts"] == sum(c["touching_contacts"] for c in oc) > 0
    assert ctr["steps"] == lanes * steps
    assert ctr["nonfinite_steps"] == 0 and ctr["faulted_lanes"] == 0
    b.close()


@pytest.mark.parametrize("env_id", ENVS)
def test_golden_trajectory(gpu_lib, env_id):
    """The committed fixtures (tests/golden/traj_env*.npz) reproduce on the GPU."""
    from gym_puzzles_amd import Batch
    z = np.load(os.path.join(GOLDEN, f"traj_env{env_id}.npz"))
    lanes = z["draws0"].shape[0]
    b = Batch(env_id, lanes)
    _eq("obs0", b.reset(z["draws0"], z["act0"]), z["obs0"])
    for t in range(z["acts"].shape[0]):
        obs, rew, done, _ = b.step(z["acts"][t])
        _eq(f"obs@{t}", obs, z["obs"][t])
        _eq(f"reward@{t}", rew, z["reward"][t])
        _eq(f"done@{t}", done, z["done"][t])
        _eq(f"bodies@{t}", b.bodies(), z["bodies"][t])
        if done.any():
            m = done.astype(bool)
            o2 = b.reset(z["rdraws"][t], z["racts"][t], mask=m).copy()
            _eq(f"reset obs@{t}", o2[m], z["robs"][t][m])
    b.close()


def test_reference_test_flow_v0_seed17(gpu_lib):
    """gym_puzzles/tests/test_env.py flow (seed 17) on v0; expected values from the fixture."""
    from gym_puzzles_amd import Batch
    from gym_puzzles_amd.seeding import Box
    z = np.load(os.path.join(GOLDEN, "scenario_v0_seed17.npz"))
    b = Batch(0, 1)
    sp = Box(-1.0, 1.0, shape=(6,))
    np.random.seed(0)
    b.reset(reference_draws(0)[None], sp.sample()[None])
    _eq("obs0", b.reset(z["draws"][None], z["act0"][None]), z["obs0"][None])
    for t in range(z["acts"].shape[0]):
        obs, rew, _, _ = b.step(z["acts"][t][None])
        _eq(f"obs@{t}", obs[0], z["obs"][t])
        _eq(f"reward@{t}", rew[0], np.float32(z["reward"][t]))
    _eq("bodies", b.bodies()[0], z["bodies"])
    b.close()


@pytest.mark.parametrize("env_id", list(ENVS) + list(AGENT_VARIANTS))
def test_device_autoreset_full_size(gpu_lib, orc, env_id):
    """BASELINE.json-size batch (4096 lanes; 1024 for the num_agents variants) on the device-input
    path: counter-RNG spawns and actions, TimeLimit 64 so every lane auto-resets several times; final
    body state and per-lane reward sums must equal the oracle's batch runner bit for bit."""
    from gym_puzzles_amd import Batch
    lanes, steps, limit = (4096 if env_id in ENVS else 1024), 200, 64
    b = Batch(env_id, lanes, seed=17)
    b.set_auto_reset(True)
    b.set_time_limit(limit)
    b.reset()
    rsum = np.zeros(lanes, np.float64)
    n_fin = 0
    for _ in range(steps):
        _, rew, done, _ = b.step()
        rsum += rew.astype(np.float64)
        n_fin += int(done.sum())
    threads = min(16, os.cpu_count() or 1)
    n, _, bodies, orsum, eps = orc.batch_run(env_id, lanes, steps, 17, draw_bounds(env_id), threads=threads,
                                             outputs=True, max_steps=limit)
    assert n == lanes * steps
    assert n_fin == int((eps - 1).sum()) and n_fin >= 3 * lanes
    _eq("bodies", b.bodies(), bodies)
    _eq("reward sums", rsum, orsum)
    assert not b.faults().any(), "a loop guard tripped"
    b.close()


def test_lane_offset_invariance(gpu_lib):
    """A shard with lane_offset = k steps exactly like lanes k.. of the unsharded batch."""
    from gym_puzzles_amd import Batch
    full = Batch(2, 256, seed=5)
    half = Batch(2, 128, seed=5, lane_offset=128)
    for b in (full, half):
        b.set_auto_reset(True)
        b.set_time_limit(40)
        b.reset()
    for _ in range(100):
        of, rf, df, _ = full.step()
        oh, rh, dh, _ = half.step()
        _eq("obs", oh, of[128:])
        _eq("reward", rh, rf[128:])
        _eq("done", dh, df[128:])
    _eq("bodies", half.bodies(), full.bodies()[128:])


def test_autoreset_terminal_obs_matches_manual_reset(gpu_lib):
    """Auto-reset (SB3 semantics) == stepping without it and resetting the finished lanes by mask."""
    from gym_puzzles_amd import Batch
    lanes = 96
    a = Batch(0, lanes, seed=9)
    m = Batch(0, lanes, seed=9)
    for b in (a, m):
        b.set_time_limit(30)
        b.reset()
    a.set_auto_reset(True)
    rs = np.random.RandomState(4)
    for _ in range(75):
        act = rs.uniform(-1, 1, size=(lanes, 6)).astype(np.float32)
        oa, ra, da, ta = a.step(act, want_terminal_obs=True)
        om, rm, dm, tm = m.step(act)
        _eq("reward", ra, rm)
        _eq("done", da, dm)
        _eq("truncated", ta, tm)
        fin = dm.astype(bool)
        if fin.any():
            _eq("terminal obs", a.terminal_obs[fin], om[fin])
            om = m.reset(mask=fin).copy()                    # device-RNG reset of those lanes
        _eq("obs", oa, om)


def test_state_round_trip(gpu_lib):
    from gym_puzzles_amd import Batch
    b = Batch(4, 32, seed=3)
    b.set_auto_reset(True)
    b.reset()
    for _ in range(40):
        b.step()
    snap = b.get_state().copy()
    runs = []
    for _ in range(2):
        b.set_state(snap)
        for _ in range(30):
            obs, rew, _, _ = b.step()
        runs.append((obs.copy(), rew.copy(), b.bodies()))
    for x, y in zip(*runs):
        _eq("replay", x, y)


def test_step_before_reset_fails_loudly(gpu_lib):
    from gym_puzzles_amd import Batch, MrpError
    b = Batch(0, 4)
    with pytest.raises(MrpError, match="before reset"):
        b.step()


def test_device_sincos_matches_glibc(gpu_lib, orc):
    """b2Rot::Set as the step evaluates it (mrp::rot: the branch-free form below 120 rad, glibc's
    other branches above) equals the host glibc sinf/cosf (the oracle's) on every input: random
    angles at several scales, random bit patterns (NaN, inf, subnormals included) and the range
    thresholds (2^-12, pi/4, 120) and quadrant boundaries."""
    from gym_puzzles_amd._native import selftest_sincos
    rs = np.random.RandomState(0)
    edges = np.array([2.0 ** -12, np.pi / 4, 120.0], np.float32)
    near = (edges.view(np.int32)[:, None] + np.arange(-2000, 2001)[None, :]).astype(np.int32).view(np.float32).ravel()
    x = np.concatenate([
        rs.uniform(-10, 10, 200000), rs.uniform(-1e4, 1e4, 50000), rs.uniform(-1e30, 1e30, 2000),
        np.arange(-64, 65) * (np.pi / 4), np.array([0.0, -0.0, 1e-30, -1e-30, 1e-45, np.pi, 3e38, -3e38]),
    ]).astype(np.float32)
    x = np.concatenate([x, near, -near, rs.randint(0, 2 ** 32, 300000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    s, c = selftest_sincos(x)
    es, ec = np.zeros_like(x), np.zeros_like(x)
    orc.lib().or_sincos_batch(x.ctypes.data, es.ctypes.data, ec.ctypes.data, x.size)
    for name, got, exp in (("sinf", s, es), ("cosf", c, ec)):
        nan = np.isnan(exp)
        assert np.array_equal(np.isnan(got), nan), name
        _eq(name, got[~nan].view(np.uint32), exp[~nan].view(np.uint32))   # bit patterns: signed zeros count


def test_step_device_with_torch_stream(gpu_lib):
    """mrp_step_device on torch tensors, on a torch stream, equals the host-pointer path."""
    import torch

    from gym_puzzles_amd import Batch
    lanes = 128
    h = Batch(2, lanes, seed=11)
    d = Batch(2, lanes, seed=11)
    for b in (h, d):
        b.set_auto_reset(True)
        b.reset()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    d.set_stream(s.cuda_stream)
    obs = torch.zeros((lanes, d.obs_dim), device=dev)
    rew = torch.zeros(lanes, device=dev)
    done = torch.zeros(lanes, dtype=torch.uint8, device=dev)
    for _ in range(50):
        h.step()
        with torch.cuda.stream(s):
            d.step_device(0, obs.data_ptr(), rew.data_ptr(), done.data_ptr())
    s.synchronize()
    _eq("obs", obs.cpu().numpy(), h.obs)
    _eq("reward", rew.cpu().numpy(), h.reward)
    _eq("done", done.cpu().numpy(), h.done)


@pytest.mark.parametrize("env_id,lanes,explicit", [(0, 512, True), (1, 4096, False), (5, 8192, False)])
def test_costliest_first_schedule_changes_nothing(gpu_lib, env_id, lanes, explicit):
    """Lane scheduling (mrp_set_schedule) only permutes which workgroup steps which lane: every
    output and the full lane state must be bit-identical to lane-order dispatch.  Env 1 at 4096
    lanes and env 5 at 8192 (more than k_step keeps resident; v3 runs 4 waves per SIMD, so its 4096 lanes
    are all resident) run mrp_create's default, which is costliest-first
    there (mrp_kernels.hip mrp_create), so the default path's ordering kernel over all lanes is covered."""
    from gym_puzzles_amd import Batch
    steps = 60
    a, b = Batch(env_id, lanes, seed=5), Batch(env_id, lanes, seed=5)
    if explicit:
        a.set_schedule(True)
    else:
        assert a.get_schedule() == 1, "costliest-first is the default for this env above the resident lanes"
    b.set_schedule(False)
    assert b.get_schedule() == 0
    for x in (a, b):
        x.set_auto_reset(True)
        x.set_time_limit(25)
    _eq("reset", a.reset(), b.reset())
    for t in range(steps):
        oa, ra, da, _ = a.step()
        ob, rb, db, _ = b.step()
        _eq(f"obs@{t}", oa, ob)
        _eq(f"reward@{t}", ra, rb)
        _eq(f"done@{t}", da, db)
    _eq("state", a.get_state(), b.get_state())
    a.close()
    b.close()


def test_two_units_alive_at_once_keep_their_own_tables(gpu_lib):
    """mrp_create uploads a context's tables into its own env unit only.  Envs 15 and 19 (one agent, light /
    heavy block) share their Dims but not their tables: two contexts alive at once and stepped alternately
    give, bit for bit, what a context of the same id gives stepped alone in a fresh Batch.  A table that
    reached the wrong unit would otherwise show only as a physics mismatch far from its cause."""
    from gym_puzzles_amd import Batch
    lanes, steps, seed = 2, 8, 31

    def run(env_ids):
        bs = [Batch(e, lanes, seed=seed) for e in env_ids]
        rows = [[("reset", b.reset().copy())] for b in bs]
        for t in range(steps):
            for b, r in zip(bs, rows):   # alternately: one step of each context per round
                b.step()                 # device-RNG actions
                r += [(f"obs@{t}", b.obs.copy()), (f"reward64@{t}", b.reward64.copy()), (f"done@{t}", b.done.copy()),
                      (f"status@{t}", b.status.copy())]
        for b in bs:
            b.close()
        return rows

    together = run((15, 19))
    assert not np.array_equal(together[0][0][1], together[1][0][1]), "the two envs' tables give different worlds"
    for env_id, both in zip((15, 19), together):
        alone, = run((env_id,))
        for (name, g), (_, c) in zip(both, alone):
            _eq(f"env {env_id} {name}", g, c)


@pytest.mark.parametrize("env_id", list(ENVS) + list(AGENT_VARIANTS))
def test_whole_episode_soak(gpu_lib, orc, env_id):
    """One whole episode at the registered TimeLimit (2000 / 3000 / 1500 steps) plus 50 steps of
    the next, on the device-RNG + auto-reset path the bench runs: every lane reaches its TimeLimit
    reset (or an earlier done), no loop guard trips, every observation stays finite, and the final
    body state and per-lane reward sums equal the oracle's batch runner bit for bit."""
    from gym_puzzles_amd import Batch
    lanes = 4096 if env_id in (0, 5) else (1024 if env_id in ENVS else 256)
    b = Batch(env_id, lanes, seed=23)
    steps = b.max_episode_steps + 50
    b.set_auto_reset(True)
    b.reset()
    rsum = np.zeros(lanes, np.float64)
    ended = np.zeros(lanes, bool)
    for _ in range(steps):
        obs, rew, done, _ = b.step()
        assert np.isfinite(obs).all()
        rsum += rew.astype(np.float64)
        ended |= done.astype(bool)
    assert ended.all()
    assert not b.faults().any(), "a loop guard tripped"
    threads = min(16, os.cpu_count() or 1)
    n, _, bodies, orsum, _ = orc.batch_run(env_id, lanes, steps, 23, draw_bounds(env_id), threads=threads,
                                           outputs=True, max_steps=b.max_episode_steps)
    assert n == lanes * steps
    _eq("bodies", b.bodies(), bodies)
    _eq("reward sums", rsum, orsum)
    b.close()


def _twin(env_id, lanes, seed=21, warm=30):
    """Two identical batches advanced `warm` device-RNG steps (auto-reset on)."""
    from gym_puzzles_amd import Batch
    bs = [Batch(env_id, lanes, seed=seed) for _ in range(2)]
    for b in bs:
        b.set_auto_reset(True)
        b.reset()
        for _ in range(warm):
            b.step()
    return bs


@pytest.mark.parametrize("env_id", [0, 4])
def test_nonfinite_lane_is_flagged_not_fatal(gpu_lib, env_id):
    """A lane corrupted through mrp_set_state (a NaN body velocity) is reported by the status
    flag MRP_STATUS_NONFINITE and counted; the other lanes stay bit-identical to an uncorrupted
    twin batch and nothing raises (SURVEY.md 8b Errors: per-lane NaN -> info['nan'], never a crash)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from gym_puzzles_amd._native import STATUS_NONFINITE
    from lane_layout import offsets
    lanes, bad = 64, 5
    a, b = _twin(env_id, lanes)
    st = b.get_state().copy()
    off, _ = offsets(env_id)
    st[bad, off["vx"]] = np.float32(np.nan).view(np.uint32)
    b.set_state(st)
    flagged = 0
    keep = np.arange(lanes) != bad
    for t in range(3):
        oa, ra, da, _ = a.step()
        ob, rb, db, _ = b.step()
        if t == 0:   # the NaN velocity reaches the position and the observation in this step
            assert b.status[bad] & STATUS_NONFINITE
        flagged += int(bool(b.status[bad] & STATUS_NONFINITE))
        assert not (b.status[keep] & STATUS_NONFINITE).any()
        _eq("obs of healthy lanes", ob[keep], oa[keep])
        _eq("reward of healthy lanes", rb[keep], ra[keep])
    # NaN compares false, so the reference's in-place test `not abs(fx - x) > eps` holds and the
    # lane ends its episode (auto-reset) -- the flag counts the lane-steps that carried the NaN
    assert b.counters_ex()["nonfinite_steps"] == flagged >= 1 and a.counters_ex()["nonfinite_steps"] == 0


def test_loop_guard_fault_reaches_info(gpu_lib):
    """A lane whose loop-guard fault word is set (as a tripped guard leaves it; written through
    mrp_set_state) is reported in every later step: status bit MRP_STATUS_FAULT and the VecEnv's
    info['mrp_fault'] = the guard code; no other lane is flagged and every lane's physics is
    bit-identical to an uncorrupted twin (the fault word is a report, not a physics input)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from gym_puzzles_amd import MultiRobotPuzzleVecEnv
    from gym_puzzles_amd._native import STATUS_FAULT
    from lane_layout import offsets
    lanes, bad = 64, 9
    venvs = [MultiRobotPuzzleVecEnv(0, lanes, seed=3) for _ in range(2)]
    for v in venvs:
        v.reset()
    rs = np.random.RandomState(2)
    acts = rs.uniform(-1, 1, size=(30, lanes, 6)).astype(np.float32)
    for t in range(20):
        for v in venvs:
            v.step(acts[t])
    st = venvs[1].batch.get_state().copy()
    off, _ = offsets(0)
    st[bad, off["fault"]] = np.uint32(4)          # MRP_FAULT_CONTACT_LIST
    venvs[1].batch.set_state(st)
    for t in range(20, 24):
        oa, ra, da, ia = venvs[0].step(acts[t])
        ob, rb, db, ib = venvs[1].step(acts[t])
        assert venvs[1].batch.status[bad] & STATUS_FAULT
        assert ib[bad].get("mrp_fault") == 4
        assert all("mrp_fault" not in ib[i] for i in range(lanes) if i != bad)
        assert all("mrp_fault" not in x for x in ia)
        _eq("obs", ob, oa)
        _eq("reward", rb, ra)
    assert venvs[1].batch.counters_ex()["faulted_lanes"] == 1
    for v in venvs:
        v.close()


@pytest.mark.parametrize("env_id", [0, 2, 4])
def test_multi_step_launch_equals_single_steps(gpu_lib, env_id):
    """mrp_step_n_device (K env steps per launch, device-RNG actions, auto-reset) writes every
    step's obs / reward / done / truncated / status / terminal obs bit-identical to K single-step
    launches, and leaves the identical lane state."""
    import torch
    lanes, K, rounds = 256, 8, 5
    a, b = _twin(env_id, lanes, seed=31, warm=3)
    for x in (a, b):
        x.set_time_limit(13)
    dev = torch.device("cuda", 0)
    O = a.obs_dim
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    obs, rew, r64, done, tr, stt, term = (z(K, lanes, O), z(K, lanes), z(K, lanes, dt=torch.float64),
                                          z(K, lanes, dt=torch.uint8), z(K, lanes, dt=torch.uint8),
                                          z(K, lanes, dt=torch.uint8), z(K, lanes, O))
    a.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    for r in range(rounds):
        a.step_n_device(K, 0, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), tr.data_ptr(), stt.data_ptr(),
                        term.data_ptr(), r64.data_ptr())
        torch.cuda.synchronize()
        for k in range(K):
            ob, rb, db, tb = b.step(want_terminal_obs=True)
            _eq(f"obs@{r},{k}", obs[k].cpu().numpy(), ob)
            _eq(f"reward@{r},{k}", rew[k].cpu().numpy(), rb)
            _eq(f"reward64@{r},{k}", r64[k].cpu().numpy(), b.reward64)
            _eq(f"done@{r},{k}", done[k].cpu().numpy(), db)
            _eq(f"truncated@{r},{k}", tr[k].cpu().numpy(), tb)
            _eq(f"status@{r},{k}", stt[k].cpu().numpy(), b.status)
            m = db.astype(bool)
            _eq(f"terminal obs@{r},{k}", term[k].cpu().numpy()[m], b.terminal_obs[m])
    _eq("state", a.get_state(), b.get_state())
    assert a.counters_ex() == b.counters_ex()


@pytest.mark.parametrize("env_id,frameskip", [(2, 3), (0, 2)])
def test_frameskip_parity(gpu_lib, orc, env_id, frameskip):
    """MultiRobotPuzzle2(frameskip=k) (multi_robot_puzzle_02.py:139,476-478): k world.Step calls per
    env step, bit-identical to the oracle doing the same, including the reset's step."""
    from gym_puzzles_amd import Batch
    lanes, steps = 32, 80
    rs_d = [np.random.RandomState(300 + l) for l in range(lanes)]
    rs_a = np.random.RandomState(77)
    b = Batch(env_id, lanes)
    b.set_frameskip(frameskip)
    b.update_params(0, 1)
    envs = [orc.OracleEnv(env_id) for _ in range(lanes)]
    for o in envs:
        o.set_frameskip(frameskip)
        o.set_shaped(1000.0, 100.0, 10000.0)
    draws = np.stack([reference_draws(env_id, r) for r in rs_d])
    acts = rs_a.uniform(-1, 1, size=(lanes, b.act_dim)).astype(np.float32)
    _eq("reset obs", b.reset(draws, acts), np.stack([o.reset(draws[l], acts[l]) for l, o in enumerate(envs)]).astype(np.float32))
    for t in range(steps):
        a = rs_a.uniform(-1, 1, size=(lanes, b.act_dim)).astype(np.float32)
        obs, rew, done, _ = b.step(a)
        res = [o.step(a[l]) for l, o in enumerate(envs)]
        _eq(f"obs@{t}", obs, np.stack([r[0] for r in res]).astype(np.float32))
        _eq(f"reward@{t}", rew, np.array([r[1] for r in res]).astype(np.float32))
        _eq(f"bodies@{t}", b.bodies(), np.stack([o.bodies() for o in envs]))
        if done.any():
            m = done.astype(bool)
            d2 = np.stack([reference_draws(env_id, r) for r in rs_d])
            a2 = rs_a.uniform(-1, 1, size=(lanes, b.act_dim)).astype(np.float32)
            o2 = b.reset(d2, a2, mask=m).copy()
            for l in np.nonzero(m)[0]:
                _eq(f"reset obs@{t}", o2[l], envs[l].reset(d2[l], a2[l]).astype(np.float32))
    assert b.counters()[1] == sum(o.counters()[1] for o in envs)
    b.close()


@pytest.mark.parametrize("env_id", [0, 2])
def test_set_state_repairs_understated_contact_mark(gpu_lib, env_id):
    """k_step moves only the contact slots below LaneState::cHW; a state injected through
    mrp_set_state with that mark understated (here zeroed on every lane) must not lose its live
    contacts: mrp_set_state recomputes the mark from the slots, so the lanes step exactly as from
    the unmodified state.  Env 0 moves its live slots word by word, env 2 in 16-B granules; the
    oracle's device-RNG rollout of seed 41 holds contacts (5 / 17 slots) in both at step 40, with
    no lane reset before it.  tests/test_lane_repair.py checks the repair's arithmetic on the host."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from lane_layout import offsets
    a, b = _twin(env_id, 64, seed=41, warm=40)
    snap = a.get_state().copy()
    off, _ = offsets(env_id)
    assert (snap[:, off["cHW"]] > 0).any(), "no lane holds a contact slot: the test needs a live contact"
    bad = snap.copy()
    bad[:, off["cHW"]] = 0
    a.set_state(snap)
    b.set_state(bad)
    assert (b.get_state()[:, off["cHW"]].astype(np.int32) >= 1)[snap[:, off["cHW"]] > 0].all()
    for t in range(30):
        oa, ra, da, _ = a.step()
        ob, rb, db, _ = b.step()
        _eq(f"obs@{t}", ob, oa)
        _eq(f"reward@{t}", rb, ra)
    _eq("bodies", b.bodies(), a.bodies())


@pytest.mark.parametrize("env_id", [2, 4])
def test_eight_shard_composition_equals_one_batch(gpu_lib, env_id):
    """BASELINE.json configs[3]/[4]: 8192 global lanes as 8 shards of 1024 (rank r owns lane_offset
    r * 1024, gym_puzzles_amd/dist.py), each stepped by its own libmrp ctx on the device path and packed
    into the per-step message with StepGather.pack; the 8 packed blocks, in rank order, equal one
    8192-lane batch's packed outputs bit for bit at every step (obs, reward, done), across auto-resets."""
    import torch

    from gym_puzzles_amd import Batch
    from gym_puzzles_amd.dist import Shard, StepGather
    L, R, steps = 1024, 8, 60
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    full = Batch(env_id, L * R, seed=13)
    shards = [Batch(env_id, L, seed=13, lane_offset=r * L) for r in range(R)]
    for b in [full] + shards:
        b.set_stream(stream)          # the packing runs on torch's stream: same stream, ordered
        b.set_auto_reset(True)
        b.set_time_limit(25)
        b.reset()
    O = full.obs_dim

    def outs(n):
        return (torch.zeros((n, O), dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev),
                torch.zeros(n, dtype=torch.uint8, device=dev))
    fo = outs(L * R)
    so = [outs(L) for _ in range(R)]
    gfull = StepGather(Shard(0, 1, L * R), O, dev)
    gsh = [StepGather(Shard(r, R, L), O, dev) for r in range(R)]
    n_done = 0
    for t in range(steps):
        full.step_device(0, fo[0].data_ptr(), fo[1].data_ptr(), fo[2].data_ptr())
        for b, o in zip(shards, so):
            b.step_device(0, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
        want = gfull.pack(*fo)
        got = torch.cat([g.pack(*o) for g, o in zip(gsh, so)])
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"packed step {t} differs"
        n_done += int(fo[2].sum().item())
    assert n_done >= L * R, "every lane should have auto-reset at least once (TimeLimit 25)"
    _eq("bodies", np.concatenate([b.bodies() for b in shards]), full.bodies())
    for b in [full] + shards:
        assert not b.faults().any()
        b.close()
