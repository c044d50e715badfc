"""CPU tests of the parity oracle (oracle/, test infrastructure) against everything that pins it:

* known-answer masses/inertias recomputed here from the reference geometry
  (multi_robot_puzzle_00.py:62-67,303-332; multi_robot_puzzle_02.py:63-66,162-165,331-384)
  with the polygon mass formulas, independently of the C code;
* closed-form free-flight kinematics of a v0 agent (velocity set, damping, integration;
  multi_robot_puzzle_00.py:415-424 + Box2D b2Island::Solve), float32 bit for bit;
* a numpy restatement of the v0 observation/reward (multi_robot_puzzle_00.py:130-132,
  277-291,430-521) and of the v3 observation/reward (core.py:65-67,289-350,369-414)
  recomputed from the oracle's body state;
* the committed golden fixtures (tests/golden/, see make_golden.py).
Parity of the oracle against pybox2d itself is unpinned (no box2d-py here).
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import pytest

from gym_puzzles_amd.spawn import ENV_CFG, draw_bounds, reference_draws

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def orc(oracle_lib):
    from oracle import oracle
    return oracle


# ----------------------------------------------------------------------------- mass KATs
def _poly_mass(verts, density):
    """Area, centroid and inertia about the origin of a convex CCW polygon (float64)."""
    v = np.asarray(verts, np.float64)
    area = 0.0
    c = np.zeros(2)
    inertia = 0.0
    for i in range(len(v)):
        e1, e2 = v[i], v[(i + 1) % len(v)]
        d = e1[0] * e2[1] - e1[1] * e2[0]
        a = 0.5 * d
        area += a
        c += a * (e1 + e2) / 3.0
        inertia += (0.25 / 3.0) * d * (e1 @ e1 + e1 @ e2 + e2 @ e2)
    return density * area, c / area, density * inertia


def _box(hx, hy, cx=0.0, cy=0.0):
    return [(cx - hx, cy - hy), (cx + hx, cy - hy), (cx + hx, cy + hy), (cx - hx, cy + hy)]


def _compound(parts):
    m = sum(p[0] for p in parts)
    c = sum(p[0] * p[1] for p in parts) / m
    return m, c, sum(p[2] for p in parts)


AGENT_V0 = [(-0.25, -0.75), (0.25, -0.75), (0.75, -0.25), (0.75, 0.25), (0.25, 0.75), (-0.25, 0.75),
            (-0.75, 0.25), (-0.75, -0.25)]
AGENT_V2 = [(-0.039, -0.095), (0.039, -0.095), (0.095, -0.039), (0.095, 0.039), (0.039, 0.095), (-0.039, 0.095),
            (-0.095, 0.039), (-0.095, -0.039)]


def _expected_masses(env_id):
    if ENV_CFG[env_id][0] == 3:   # Block("T") blocks.py:80-90 at scale 0.5 / 1, density 5 / 10; Robot robot.py:34-40
        s, dens = (1.0, 10.0) if ENV_CFG[env_id][3] else (0.5, 5.0)
        blk = _compound([_poly_mass(_box(1 * s, 1 * s, 0, -1 * s), dens), _poly_mass(_box(3 * s, 1 * s, 0, 1 * s), dens)])
        agent = _poly_mass([(x * 8.0, y * 8.0) for x, y in AGENT_V2], 5.0)
        return [blk] + [agent] * ENV_CFG[env_id][1]
    if env_id in (0, 1):
        s = 2.0 if env_id == 1 else 1.0
        blk = _compound([_poly_mass(_box(0.5 * s, 0.5 * s, 0, -0.5 * s), 5.0 * (2 if env_id == 1 else 1)),
                         _poly_mass(_box(1.5 * s, 0.5 * s, 0, 0.5 * s), 5.0 * (2 if env_id == 1 else 1))])
        agent = (1.0, np.zeros(2), 0.0)    # zero density -> mass 1, I 0 (Box2D ResetMassData)
        return [blk] + [agent] * (2 if env_id == 0 else 5)
    _, na, nb, heavy = ENV_CFG[env_id]
    dens = 20.0 if heavy else 1.56
    t = _compound([_poly_mass(_box(0.1, 0.1, 0, -0.1), dens), _poly_mass(_box(0.3, 0.1, 0, 0.1), dens)])
    agent = _poly_mass(AGENT_V2, 17.3)
    if nb == 1:   # MultiRobotPuzzle2(num_agents=na): the T block, then na agents (_02.py:313-378)
        return [t] + [agent] * na
    l_blk = _compound([_poly_mass(_box(0.1, 0.1, 0.1, 0.05), dens), _poly_mass(_box(0.1, 0.2, -0.1, -0.05), dens)])
    i_blk = _poly_mass(_box(0.1, 0.2), dens)
    return [t, l_blk, i_blk, agent, agent]


@pytest.mark.parametrize("env_id", range(23))
def test_mass_known_answers(orc, env_id):
    e = orc.OracleEnv(env_id)
    e.reset(reference_draws(env_id, np.random.RandomState(17)), np.zeros(e.act_dim, np.float32))
    exp = _expected_masses(env_id)
    for i, (m, c, inertia) in enumerate(exp):
        got = e.body_mass(i)
        assert got[0] == pytest.approx(m, rel=2e-6)
        assert got[1] == pytest.approx(inertia, rel=2e-5, abs=1e-9)
        assert got[2] == pytest.approx(c[0], abs=1e-6) and got[3] == pytest.approx(c[1], abs=1e-6)


def test_mass_survey_values(orc):
    """SURVEY.md Appendix A figures (I about the centre of mass = I_origin - m|c|^2)."""
    for env_id, m, icm in ((0, 20.0, 17.0833), (1, 160.0, 546.667), (2, 0.2496, 0.008528), (3, 3.2, 0.109333)):
        e = orc.OracleEnv(env_id)
        e.reset(reference_draws(env_id, np.random.RandomState(1)), np.zeros(e.act_dim, np.float32))
        mass, i_o, cx, cy = e.body_mass(0)
        assert mass == pytest.approx(m, rel=1e-5)
        assert i_o - mass * (cx * cx + cy * cy) == pytest.approx(icm, rel=1e-4)
    e = orc.OracleEnv(2)
    e.reset(reference_draws(2, np.random.RandomState(1)), np.zeros(4, np.float32))
    assert e.body_mass(1)[0] == pytest.approx(0.516024, rel=1e-6)


# ----------------------------------------------------------------------------- kinematics KAT
def test_v0_free_agent_kinematics_bitwise(orc):
    """Agents far from everything: v = f32(a * SPEED) (numpy float64 product), then per step
    v *= 1/(1 + h*5), c += h*v in float32 (Box2D integrate; agents have invI = 0)."""
    e = orc.OracleEnv(0)
    draws = np.array([15.0, 12.0, 0.0, 5.0, 5.0, 5.0, 10.0])    # block x,y,angle; agents (x,y)
    rs = np.random.RandomState(3)
    a0 = (rs.uniform(-1, 1, 6) * 0.2).astype(np.float32)
    e.reset(draws, a0)
    f32 = np.float32
    h = f32(1.0) / f32(50.0)
    damp = f32(1.0) / (f32(1.0) + h * f32(5.0))
    speed = 10 / 30.0 * 4
    pos = [np.array([5.0, 5.0], np.float32), np.array([5.0, 10.0], np.float32)]
    ang = [f32(0.0), f32(0.0)]
    acts = [a0] + [(rs.uniform(-1, 1, 6) * 0.2).astype(np.float32) for _ in range(5)]
    for k, a in enumerate(acts):
        if k > 0:
            e.step(a)
        b = e.bodies().reshape(3, 6)
        for i in range(2):
            v = np.array([f32(float(a[3 * i]) * speed), f32(float(a[3 * i + 1]) * speed)], np.float32) * damp
            w = f32(float(a[3 * i + 2])) * damp
            pos[i] = (pos[i] + h * v).astype(np.float32)
            ang[i] = f32(ang[i] + h * w)
            assert np.array_equal(b[1 + i, :2], pos[i]), (k, i, b[1 + i, :2], pos[i])
            assert b[1 + i, 2] == ang[i]
            assert np.array_equal(b[1 + i, 3:5], v) and b[1 + i, 5] == w


# ----------------------------------------------------------------------------- env-layer restatement
def _t_vertices_v0():
    wide = [(-1.5, 0.0), (1.5, 0.0), (1.5, 1.0), (-1.5, 1.0)]     # fixture list is head-inserted:
    stem = [(-0.5, -1.0), (0.5, -1.0), (0.5, 0.0), (-0.5, 0.0)]   # the wide bar comes first
    return np.array(wide + stem, np.float64)


def test_v0_obs_and_reward_restatement(orc):
    """Recompute the v0 observation and reward in numpy from the oracle's bodies."""
    SCALE = 30.0
    fx, fy, fa = 320.0, 240.0 + 0.75 * SCALE, 0.0
    e = orc.OracleEnv(0)
    rs = np.random.RandomState(5)
    draws = reference_draws(0, rs)
    obs = e.reset(draws, rs.uniform(-1, 1, 6).astype(np.float32))
    verts = _t_vertices_v0()

    def dists(b):
        blk = b[0, :2].astype(np.float64) * SCALE
        ag = [b[1 + i, :2].astype(np.float64) * SCALE for i in range(2)]
        return math.hypot(blk[0] - fx, blk[1] - fy), [math.hypot(*(a - blk)) for a in ag]

    prev_bd, prev_ad = dists(e.bodies().reshape(3, 6))
    for t in range(40):
        a = rs.uniform(-1, 1, 6).astype(np.float32)
        obs, rew, done, _ = e.step(a)
        b = e.bodies().reshape(3, 6)
        gc, _ = e.flags()
        bd, ad = dists(b)
        # world centre of the block: body origin + R * localCenter (0, 0.25)
        ca, sa = math.cos(b[0, 2]), math.sin(b[0, 2])
        ox, oy = b[0, 0] - (ca * 0.0 - sa * 0.25), b[0, 1] - (sa * 0.0 + ca * 0.25)
        exp = []
        for i in range(2):
            exp += [(b[1 + i, 0] - b[0, 0]) * SCALE, (b[1 + i, 1] - b[0, 1]) * SCALE, ad[i], float(gc[i])]
        ang = b[0, 2] % (2 * np.pi)
        exp += [b[0, 0] * SCALE - fx, b[0, 1] * SCALE - fy, fa % (2 * np.pi) - ang, bd]
        for vx, vy in verts:
            exp += [(ox + ca * vx - sa * vy) * SCALE, (oy + sa * vx + ca * vy) * SCALE]
        np.testing.assert_allclose(obs, exp, rtol=1e-5, atol=2e-3)
        r = (prev_bd - bd) * 50 / 4 - 0.025 * bd / 4
        for i in range(2):
            r += (prev_ad[i] - ad[i]) * 10 / 4 - 0.1 * ad[i] / 4 + (0.25 if gc[i] else 0.0)
        assert rew == pytest.approx(r, rel=1e-5, abs=2e-3)
        assert not done
        prev_bd, prev_ad = bd, ad


def _t_vertices_v3(s):
    wide = [(-3 * s, 0.0), (3 * s, 0.0), (3 * s, 2 * s), (-3 * s, 2 * s)]   # box(3s, s) at (0, s), newest first
    stem = [(-s, -2 * s), (s, -2 * s), (s, 0.0), (-s, 0.0)]
    return np.array(wide + stem, np.float64)


@pytest.mark.parametrize("env_id", [5, 6, 15, 18, 19, 22])
def test_v3_obs_and_reward_restatement(orc, env_id):
    """Recompute the v3 observation and reward in numpy from the oracle's bodies: normalised
    poses (x - ws) / ws, (y - hs) / ws, angle % 2 pi; the goal (5/6 * 640 - 4/3, 240) px; eight
    normalised T vertices; reward weights 50 / 0.025 / 10 / 0.1 with the agent terms over 4; any num_agents (core.py:88)."""
    ws, hs = 640 / 30 / 2, 480 / 30 / 2
    gx, gy = (5 / 6 * 640 - 4 / 3 - 320) / 320, (240 - 240) / 320
    s = 1.0 if ENV_CFG[env_id][3] else 0.5
    na = ENV_CFG[env_id][1]
    e = orc.OracleEnv(env_id)
    rs = np.random.RandomState(8)
    obs = e.reset(reference_draws(env_id, rs), rs.uniform(-1, 1, 3 * na).astype(np.float32))
    verts = _t_vertices_v3(s)
    lcy = e.body_mass(0)[3]

    def poses(b):
        n = lambda x, y: ((x - ws) / ws, (y - hs) / ws)
        return n(*b[0, :2].astype(np.float64)), [n(*b[1 + i, :2].astype(np.float64)) for i in range(na)]

    def dists(b):
        (bx, by), ag = poses(b)
        return math.hypot(bx - gx, by - gy), [math.hypot(ax - bx, ay - by) for ax, ay in ag]

    prev_bd, prev_ad = dists(e.bodies().reshape(1 + na, 6))
    for t in range(60):
        a = rs.uniform(-1, 1, 3 * na).astype(np.float32)
        obs, rew, done, _ = e.step(a)
        b = e.bodies().reshape(1 + na, 6)
        (bx, by), ag = poses(b)
        bd, ad = dists(b)
        brot = float(b[0, 2]) % (2 * np.pi)
        exp = []
        for i in range(na):
            exp += [bx - ag[i][0], by - ag[i][1], float(b[1 + i, 2]) % (2 * np.pi), 0.0]
        exp += [gx - bx, gy - by, 0.0 - brot]
        ca, sa = math.cos(b[0, 2]), math.sin(b[0, 2])
        ox, oy = b[0, 0] - (-sa * lcy), b[0, 1] - (ca * lcy)      # body origin from worldCenter
        for vx, vy in verts:
            exp += [(ox + ca * vx - sa * vy - ws) / ws, (oy + sa * vx + ca * vy - hs) / ws]
        np.testing.assert_allclose(obs, exp, rtol=1e-5, atol=2e-5)
        r = (prev_bd - bd) * 50 - 0.025 * bd
        for i in range(na):
            r += (prev_ad[i] - ad[i]) * 10 / 4. - 0.1 * ad[i] / 4.
        if bd <= 25 / 640 * 2:
            r += 100
        assert rew == pytest.approx(r, rel=1e-5, abs=1e-5)
        assert bool(done) == (bd <= 25 / 640 * 2)
        assert e.flags()[0].tolist() == [0] * na   # the v3 contact detector never fires
        prev_bd, prev_ad = bd, ad


def test_v3_draw_bounds_match_reference_ranges():
    """core.py:212-215 (block x, y, angle) and :231-232 (agent x, y), BORDER = 1, SCALE = 30."""
    for env_id in (5, 6):
        b = draw_bounds(env_id)
        assert b[0] == pytest.approx((640 / 30 / 3 + 2, 640 / 30 * 2 / 3 - 2)) and b[1] == (3, 480 / 30 - 3)
        assert b[2] == (0, 2 * np.pi) and b[3] == pytest.approx((1, 640 / 30 / 3 - 2)) and b[4] == (1, 480 / 30 - 1)
        assert len(b) == 7


# ----------------------------------------------------------------------------- golden fixtures
def test_spawn_draw_golden():
    with open(os.path.join(GOLDEN, "spawn_draws.json")) as f:
        g = json.load(f)
    for env_id in range(7):
        for seed in (0, 17, 2021):
            np.random.seed(seed)
            assert np.array_equal(reference_draws(env_id), np.array(g[f"draws/{env_id}/{seed}"]))
    # np.random.seed(17) -> v0 block at x = 6.6969, y = 8.4282
    assert g["draws/0/17"][0] == pytest.approx(6.69685672, abs=1e-8)
    assert g["draws/0/17"][1] == pytest.approx(8.42821458, abs=1e-8)


def test_draw_bounds_match_reference_ranges():
    b0 = draw_bounds(0)
    assert b0[0] == (1, 640 / 30.0 - 1) and b0[1] == (1, 480 / 30.0 - 1) and b0[2] == (0, 2 * np.pi)
    b2 = draw_bounds(2)
    assert b2[0] == (0, 2 * np.pi)
    assert b2[1] == pytest.approx((0.3, 1440 / 560.0 / 3 - 0.3)) and b2[2] == pytest.approx((0.3, 810 / 560.0 - 0.3))
    assert b2[-2] == pytest.approx((1440 / 560.0 * 2 / 3 + 0.4, 1440 / 560.0 - 0.4))
    assert len(draw_bounds(1)) == 3 + 2 * 5 and len(draw_bounds(4)) == 3 + 2 * 2 + 2


def _replay_golden(orc, env_id):
    z = np.load(os.path.join(GOLDEN, f"traj_env{env_id}.npz"))
    lanes = z["draws0"].shape[0]
    envs = [orc.OracleEnv(env_id) for _ in range(lanes)]
    obs0 = np.stack([o.reset(z["draws0"][l], z["act0"][l]) for l, o in enumerate(envs)]).astype(np.float32)
    assert np.array_equal(obs0, z["obs0"])
    for t in range(z["acts"].shape[0]):
        for l, o in enumerate(envs):
            ob, r, d, _ = o.step(z["acts"][t, l])
            assert np.array_equal(ob.astype(np.float32), z["obs"][t, l]), (env_id, t, l)
            assert np.float32(r) == z["reward"][t, l] and int(d) == z["done"][t, l]
            assert np.array_equal(o.bodies(), z["bodies"][t, l])
            if d:
                assert np.array_equal(o.reset(z["rdraws"][t, l], z["racts"][t, l]).astype(np.float32), z["robs"][t, l])


@pytest.mark.parametrize("env_id", range(7))
def test_oracle_matches_golden_trajectory(orc, env_id):
    _replay_golden(orc, env_id)


def test_reference_test_flow_v0_seed17(orc):
    """gym_puzzles/tests/test_env.py flow (seed 17) on MultiRobotPuzzle-v0 via gym 0.21 seeding."""
    from gym_puzzles_amd.seeding import Box
    z = np.load(os.path.join(GOLDEN, "scenario_v0_seed17.npz"))
    o = orc.OracleEnv(0)
    sp = Box(-1.0, 1.0, shape=(6,))
    np.random.seed(0)
    o.reset(reference_draws(0), sp.sample())
    np.random.seed(17)
    sp.seed(17)
    d = reference_draws(0)
    a0 = sp.sample()
    assert np.array_equal(d, z["draws"]) and np.array_equal(a0, z["act0"])
    assert np.array_equal(o.reset(d, a0).astype(np.float32), z["obs0"])
    for t in range(z["acts"].shape[0]):
        a = sp.sample()
        assert np.array_equal(a, z["acts"][t])
        ob, r, _, _ = o.step(a)
        assert np.array_equal(ob.astype(np.float32), z["obs"][t]) and r == z["reward"][t]
    assert np.array_equal(o.bodies(), z["bodies"])


# ----------------------------------------------------------------------------- misc oracle facts
def test_fresh_world_proxy_ids(orc):
    """Fresh b2World: leaf/parent allocation gives proxy ids 0, 1, 3, 5, ...."""
    e = orc.OracleEnv(0)
    e.reset(reference_draws(0, np.random.RandomState(2)), np.zeros(6, np.float32))
    ids = e.proxy_ids()
    assert list(ids[:4]) == [0, 1, 3, 5]


def test_rng_u01_range_and_determinism(orc):
    v = [orc.rng_u01(17, l, 3, c) for l in range(8) for c in range(64)]
    assert all(0.0 <= x < 1.0 for x in v)
    assert orc.rng_u01(17, 5, 3, 9) == orc.rng_u01(17, 5, 3, 9)
    assert abs(np.mean(v) - 0.5) < 0.05


def test_batch_run_lane_offset_invariance(orc):
    """Per-lane trajectories depend only on the global lane id (multi-GPU sharding rule)."""
    b = draw_bounds(0)
    _, _, full, rs_full, ep_full = orc.batch_run(0, 8, 120, 17, b, threads=2, outputs=True)
    _, _, half, rs_half, ep_half = orc.batch_run(0, 4, 120, 17, b, threads=1, lane_offset=4, outputs=True)
    assert np.array_equal(full[4:], half) and np.array_equal(rs_full[4:], rs_half)
    assert np.array_equal(ep_full[4:], ep_half)


# The device keeps every per-lane structure in a fixed pool (gym_puzzles_amd/csrc/mrp_config.h,
# mrp_world.h LaneState / Shared): contact slots CMAX, tree nodes tree_n (the moved-proxy set is a
# 32-bit mask), move buffer MOVE_N, island arrays NBODY = ND + 4 bodies and CMAX contacts (the
# register / lane solvers need <= 64).  Box2D grows these dynamically; the oracle does too and
# records its high-water marks, so a long synthetic rollout shows the fixed pools are never
# exceeded (an overrun on the device would corrupt the lane's LDS instead of failing).
def _pools():
    from lane_layout import DIMS, move_n, tree_n
    return {e: {"contacts": c, "tree_node_id": tree_n(nf) - 1, "move_buffer": move_n(nf),
                "island_bodies": na + nb + 4, "island_contacts": min(c, 64), "toi_island_bodies": na + nb + 4,
                "toi_island_contacts": min(c, 32)}
            for e, (na, nb, nf, c) in DIMS.items()}


POOLS = _pools()


@pytest.mark.parametrize("env_id", range(23))
def test_device_pools_hold_the_oracle_high_water_marks(oracle_lib, env_id):
    from gym_puzzles_amd.spawn import draw_bounds
    from oracle.oracle import batch_capacity
    lanes = 1024 if env_id < 7 else 256   # the num_agents variants: fewer lanes, same 300-step rollout
    caps = batch_capacity(env_id, lanes, 300, 41, draw_bounds(env_id), threads=min(8, os.cpu_count() or 1), max_steps=60)
    for k, lim in POOLS[env_id].items():
        assert caps[k] <= lim, (k, caps[k], lim)
    assert caps["move_buffer"] >= 1 and caps["contacts"] >= 1


@pytest.mark.parametrize("env_id", range(23))
def test_oracle_under_asan_ubsan(env_id):
    """The oracle's sources built with AddressSanitizer + UBSan (make -C oracle asan, every finding
    fatal) run the synthetic workload of every env id cleanly: 64 lanes x 500 steps, TimeLimit 60
    (8 resets per lane)."""
    import subprocess
    from gym_puzzles_amd.spawn import draw_bounds
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    subprocess.run(["make", "-s", "-C", here, "asan"], check=True)
    args = [repr(float(x)) for lo, hi in draw_bounds(env_id) for x in (lo, hi)]
    r = subprocess.run([os.path.join(here, "build", "oracle_check_asan"), str(env_id), "64", "500", "60"] + args,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    caps = json.loads(r.stdout)
    assert caps["env_steps"] == 64 * 500
    for k, lim in POOLS[env_id].items():
        assert caps[k] <= lim, (k, caps[k], lim)


def test_work_model_is_consistent(oracle_lib):
    """The oracle's work model (OrWork; tools/chain_model.py, tools/roofline_model.py): sweeps run
    never exceed 180 per island (the device's exact early exit only shortens), dependency levels and
    the unrolled critical path never exceed the contact-by-contact count, and the committed
    VALU/latency table holds the bench's default and driver-window keys."""
    from gym_puzzles_amd.spawn import draw_bounds
    from oracle.oracle import WORK_NAMES, batch_work
    W = {n: i for i, n in enumerate(WORK_NAMES)}
    w = batch_work(0, 256, 40, 17, draw_bounds(0), threads=min(8, os.cpu_count() or 1))
    t = w.sum(axis=(0, 1))
    assert 0 < t[W["vel_sweeps"]] <= 180 * t[W["islands"]]
    upd = t[W["vel_upd1"]] + t[W["vel_upd2"]]
    assert t[W["vel_levels"]] <= upd and t[W["vel_pipe"]] <= upd + t[W["toi_vel_upd"]]
    assert t[W["pos_level_points"]] <= t[W["pos_points"]] and t[W["pos_passes"]] <= 60 * t[W["islands"]]
    assert (w >= 0).all()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                           "r3_valu_latency.json")) as f:
        table = json.load(f)
    for key in ("0:4096:6:25:17", "0:4096:21:220:17"):
        assert table[key]["flops_per_launch"] > 0 and table[key]["latency_floor_ms"] > 0


def test_work_model_matches_pinned_counts(oracle_lib):
    """The checker's work model (oracle/b2_work.c) gives exactly the counts pinned in
    tests/golden/work_model.npz (make_golden.py work_model_record, replayed here): the OrWork array of
    env ids 0, 1, 2, 4, 5, the two-wave and paired-update cycle sums, the sweep total under
    b2o_model_period(8), and on one thread the block-solver case counts and the period and topology
    histograms of env 0 and 4.  With every switch back off the first array comes out again."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rec = gen.work_model_record(threads=min(8, os.cpu_count() or 1))
    for e in gen.WORK_ENVS:
        assert np.array_equal(rec.pop(f"again_{e}"), rec[f"work_{e}"]), f"env {e}: a model switch stayed on"
    with np.load(os.path.join(GOLDEN, "work_model.npz")) as pin:
        assert sorted(pin.files) == sorted(rec)
        for k in pin.files:
            assert np.array_equal(rec[k], pin[k]), k


@pytest.mark.parametrize("env_id", [0, 1, 2, 4, 5])
def test_baseline_builds_bit_identical(orc, env_id):
    """bench.py's CPU baseline times two builds of the oracle without the work model (oracle/Makefile:
    `port`, all 180 velocity sweeps; `early`, the device's exact period-1/2 early exit).  Both must
    produce the checker's bits: final body state, per-lane reward sums and episode counts over a
    window that starts after untimed steps (or_batch_run_window) and crosses auto-resets."""
    lanes, skip, steps = 48, 5, 40
    ref = orc.batch_run(env_id, lanes, steps, 17, draw_bounds(env_id), threads=4, outputs=True, skip=skip, max_steps=25)
    for variant in ("port", "early"):
        got = orc.batch_run(env_id, lanes, steps, 17, draw_bounds(env_id), threads=4, outputs=True, skip=skip, max_steps=25,
                            variant=variant)
        assert got[0] == ref[0] == lanes * steps   # only the timed steps are counted
        for name, x, y in zip(("bodies", "reward sums", "episodes"), got[2:], ref[2:]):
            assert np.array_equal(x, y), f"{variant}: {name} differ from the checker build"
    assert "port" in orc.build_kind("port") and "early-exit" in orc.build_kind("early")


def test_batch_run_window_equals_unsplit_run(orc):
    """Untimed steps followed by timed steps (or_batch_run_window) advance every lane exactly like one
    run over both: the split only moves the clock."""
    a = orc.batch_run(2, 32, 30, 9, draw_bounds(2), threads=4, outputs=True, skip=10)
    b = orc.batch_run(2, 32, 40, 9, draw_bounds(2), threads=4, outputs=True)
    assert a[0] == 32 * 30 and b[0] == 32 * 40
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(x, y)
