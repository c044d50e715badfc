"""Host-side spawn draws in the reference's order (the reference draws from numpy's
*global* ``np.random``, not ``self.np_random``).

``reference_draws(env_id, rs)`` returns exactly the float64 values the reference's
``np.random.uniform(low, high)`` calls produce, in call order:

* v0 / Heavy-v0 (``multi_robot_puzzle_00.py:311-315,366-367``): block x, y, angle, then
  x, y per agent.
* v2 / Heavy-v2 (``multi_robot_puzzle_02.py:324,358-359,307-308``): block angle, then x, y
  per agent, then goal x, y (``_set_random_goal``; SIMPLE=True places the block at the
  screen centre and fixes agent heading at 3/2*pi).
* 3-block (build-defined): one angle per block (T, L, I), agents, goal.
* v3 / v3 heavy (``core.py:212-215,231-232``): block x, y, angle, then x, y per agent.
"""
from __future__ import annotations

import numpy as np

# v0 constants (multi_robot_puzzle_00.py:38-43)
_V0_SCALE, _V0_W, _V0_H, _V0_BORDER = 30.0, 640, 480, 1
# v2 constants (multi_robot_puzzle_02.py:39-44, 305)
_V2_SCALE, _V2_W, _V2_H, _V2_BORDER, _V2_GOAL_BORDER = 140.0 * 4, 1440, 810, 0.3, 0.4

# v3 constants (core.py:16-19, 97-98)
_V3_SCALE, _V3_W, _V3_H, _V3_BORDER = 30.0, 640, 480, 1

# The env registry, row e = env id e: (name, version, agents, blocks, heavy).  It restates the rows of
# csrc/mrp_config.h's MRP_ENV_LIST with their names (tests/test_abi.py compares the two); every table
# below derives from it.
_ENVS = (
    ("MultiRobotPuzzle-v0", 0, 2, 1, 0),
    ("MultiRobotPuzzleHeavy-v0", 0, 5, 1, 1),
    ("MultiRobotPuzzle-v2", 2, 2, 1, 0),
    ("MultiRobotPuzzleHeavy-v2", 2, 2, 1, 1),
    ("MultiRobotPuzzleHeavy-v2-3block", 2, 2, 3, 1),
    ("MultiRobotPuzzle-v3", 3, 2, 1, 0),
    ("MultiRobotPuzzle-v3-heavy", 3, 2, 1, 1),      # RobotPuzzleBase(heavy=True) (tests/test_env.py:12)
    # MultiRobotPuzzle2 / MultiRobotPuzzleHeavy2(num_agents=N) (multi_robot_puzzle_02.py:139)
    ("MultiRobotPuzzle-v2-agents1", 2, 1, 1, 0),
    ("MultiRobotPuzzle-v2-agents3", 2, 3, 1, 0),
    ("MultiRobotPuzzle-v2-agents4", 2, 4, 1, 0),
    ("MultiRobotPuzzle-v2-agents5", 2, 5, 1, 0),
    ("MultiRobotPuzzleHeavy-v2-agents1", 2, 1, 1, 1),
    ("MultiRobotPuzzleHeavy-v2-agents3", 2, 3, 1, 1),
    ("MultiRobotPuzzleHeavy-v2-agents4", 2, 4, 1, 1),
    ("MultiRobotPuzzleHeavy-v2-agents5", 2, 5, 1, 1),
    # RobotPuzzleBase(num_agents=N[, heavy=True]) (core.py:86-106)
    ("MultiRobotPuzzle-v3-agents1", 3, 1, 1, 0),
    ("MultiRobotPuzzle-v3-agents3", 3, 3, 1, 0),
    ("MultiRobotPuzzle-v3-agents4", 3, 4, 1, 0),
    ("MultiRobotPuzzle-v3-agents5", 3, 5, 1, 0),
    ("MultiRobotPuzzle-v3-heavy-agents1", 3, 1, 1, 1),
    ("MultiRobotPuzzle-v3-heavy-agents3", 3, 3, 1, 1),
    ("MultiRobotPuzzle-v3-heavy-agents4", 3, 4, 1, 1),
    ("MultiRobotPuzzle-v3-heavy-agents5", 3, 5, 1, 1),
)
ENV_IDS = {row[0]: e for e, row in enumerate(_ENVS)}       # name -> env id
ENV_CFG = {e: row[1:] for e, row in enumerate(_ENVS)}      # env id -> (version, agents, blocks, heavy)
ENV_VERSION = {e: c[0] for e, c in ENV_CFG.items()}
N_AGENTS = {e: c[1] for e, c in ENV_CFG.items()}
N_BLOCKS = {e: c[2] for e, c in ENV_CFG.items()}
# MultiRobotPuzzle2(num_agents=N) / MultiRobotPuzzleHeavy2(num_agents=N) -> env id
V2_AGENT_IDS = {(c[3], c[1]): e for e, c in ENV_CFG.items() if c[0] == 2 and c[2] == 1}
# RobotPuzzleBase(num_agents=N, heavy=h) -> env id
V3_AGENT_IDS = {(c[3], c[1]): e for e, c in ENV_CFG.items() if c[0] == 3}


def draw_bounds(env_id: int):
    """(low, high) of every uniform draw of one reset, in call order."""
    b = []
    if ENV_VERSION[env_id] == 0:
        xr = (_V0_BORDER, _V0_W / _V0_SCALE - _V0_BORDER)
        yr = (_V0_BORDER, _V0_H / _V0_SCALE - _V0_BORDER)
        b += [xr, yr, (0, 2 * np.pi)]
        b += [xr, yr] * N_AGENTS[env_id]
    elif ENV_VERSION[env_id] == 3:
        b += [(_V3_W / _V3_SCALE / 3 + 2 * _V3_BORDER, _V3_W / _V3_SCALE * 2 / 3 - 2 * _V3_BORDER),
              (3 * _V3_BORDER, _V3_H / _V3_SCALE - 3 * _V3_BORDER), (0, 2 * np.pi)]
        b += [(_V3_BORDER, _V3_W / _V3_SCALE / 3 - 2 * _V3_BORDER), (_V3_BORDER, _V3_H / _V3_SCALE - _V3_BORDER)] * N_AGENTS[env_id]
    else:
        b += [(0, 2 * np.pi)] * N_BLOCKS[env_id]
        xr = (_V2_BORDER, _V2_W / _V2_SCALE / 3 - _V2_BORDER)
        yr = (_V2_BORDER, _V2_H / _V2_SCALE - _V2_BORDER)
        b += [xr, yr] * N_AGENTS[env_id]
        b += [(_V2_W / _V2_SCALE * 2 / 3 + _V2_GOAL_BORDER, _V2_W / _V2_SCALE - _V2_GOAL_BORDER),
              (_V2_GOAL_BORDER, _V2_H / _V2_SCALE - _V2_GOAL_BORDER)]
    return b


def reference_draws(env_id: int, rs=None) -> np.ndarray:
    """Draw one reset's spawn values from ``rs`` (a RandomState; default: global np.random)."""
    rs = np.random if rs is None else rs
    return np.array([rs.uniform(lo, hi) for lo, hi in draw_bounds(env_id)], dtype=np.float64)


def sample_action(act_dim: int, rs) -> np.ndarray:
    """gym 0.21 ``Box.sample()`` for a bounded [-1, 1] box: uniform(low, high).astype(float32)."""
    return rs.uniform(low=-np.ones(act_dim), high=np.ones(act_dim), size=(act_dim,)).astype(np.float32)
