// mrp_config.h -- per-environment static tables (geometry, mass, spawn bounds) and the
// registry of the MultiRobotPuzzle ids with their compile-time dimensions.
//
// Env ids follow include/mrp.h: 0 MultiRobotPuzzle-v0, 1 MultiRobotPuzzleHeavy-v0,
// 2 MultiRobotPuzzle-v2, 3 MultiRobotPuzzleHeavy-v2, 4 Heavy-v2 with the build-defined
// 3-block square, 5 MultiRobotPuzzle-v3 (RobotPuzzleBase,
// core.py), 6 v3 constructed with heavy=True (tests/test_env.py:12), 7-10 MultiRobotPuzzle2
// constructed with num_agents = 1, 3, 4, 5 and 11-14 MultiRobotPuzzleHeavy2 with the same
// agent counts (multi_robot_puzzle_02.py:139,151,354), 15-18 / 19-22 RobotPuzzleBase(num_agents =
// 1, 3, 4, 5) with heavy False / True (core.py:86-106).
#pragma once
#include "mrp_math.h"

namespace mrp {

// status byte flags next to the terminal kind (include/mrp.h MRP_STATUS_NONFINITE / MRP_STATUS_FAULT)
constexpr int MRP_STATUS_NONFINITE_BIT = 0x40, MRP_STATUS_FAULT_BIT = 0x80;

constexpr int BLOCK = 64;     // threads of a lane kernel's workgroup: one wave, so lanes of a block never wait on each other
constexpr int MAX_POLY = 8;
constexpr int MAXBODY = 10;   // bodies: blocks + agents + 4 walls (max over configs: 1 + 5 + 4)
constexpr int MAXF = 24;      // fixtures (max over configs: v2 with 5 agents, 2 + 5 * 3 + 4 = 21)
constexpr int MAXV = 16;
constexpr int MAXDRAW = 16;

// The registry: one row per env id, X(id, version (0 v0, 2 v2, 3 v3), agents, blocks, heavy block,
// registered TimeLimit), in id order.  N_ENVS, ENV_CFG, Dims<ENV> and the launch table of mrp_ops.h
// expand from it; build.py compiles one env unit per row, and gym_puzzles_amd/spawn.py restates the
// rows with their names (tests/test_abi.py compares the two).
// clang-format off
#define MRP_ENV_LIST(X) \
    X(0, 0, 2, 1, 0, 2000) \
    X(1, 0, 5, 1, 1, 3000) \
    X(2, 2, 2, 1, 0, 2000) \
    X(3, 2, 2, 1, 1, 2000) \
    X(4, 2, 2, 3, 1, 2000) \
    X(5, 3, 2, 1, 0, 1500) \
    X(6, 3, 2, 1, 1, 1500) \
    X(7, 2, 1, 1, 0, 2000) \
    X(8, 2, 3, 1, 0, 2000) \
    X(9, 2, 4, 1, 0, 2000) \
    X(10, 2, 5, 1, 0, 2000) \
    X(11, 2, 1, 1, 1, 2000) \
    X(12, 2, 3, 1, 1, 2000) \
    X(13, 2, 4, 1, 1, 2000) \
    X(14, 2, 5, 1, 1, 2000) \
    X(15, 3, 1, 1, 0, 1500) \
    X(16, 3, 3, 1, 0, 1500) \
    X(17, 3, 4, 1, 0, 1500) \
    X(18, 3, 5, 1, 0, 1500) \
    X(19, 3, 1, 1, 1, 1500) \
    X(20, 3, 3, 1, 1, 1500) \
    X(21, 3, 4, 1, 1, 1500) \
    X(22, 3, 5, 1, 1, 1500)
// clang-format on

struct EnvCfg { int id, version, n_agents, n_blocks, heavy, max_steps; };
#define MRP_ENV_CFG_ROW(id, version, n_agents, n_blocks, heavy, max_steps) {id, version, n_agents, n_blocks, heavy, max_steps},
constexpr EnvCfg ENV_CFG[] = {MRP_ENV_LIST(MRP_ENV_CFG_ROW)};
#undef MRP_ENV_CFG_ROW
constexpr int N_ENVS = sizeof(ENV_CFG) / sizeof(ENV_CFG[0]);
constexpr bool env_rows_in_id_order() {
    for (int i = 0; i < N_ENVS; ++i)
        if (ENV_CFG[i].id != i) return false;
    return true;
}
static_assert(env_rows_in_id_order(), "row i of MRP_ENV_LIST is env id i");

// Compile-time dimensions per env id: one family per version, selected by the registry row.
// CMAX = fixture pairs on different bodies with at least one dynamic body, not both static (upper
// bound on live contacts).
// MultiRobotPuzzle2(num_agents = N) (multi_robot_puzzle_02.py:139): one T block (2 fixtures),
// N agents (body + 2 wheels), 4 walls
template <int N> struct DimsV2 {
    static constexpr int DF = 2 + 3 * N;   // dynamic fixtures
    static constexpr int V = 2, NA = N, NB = 1, NF = DF + 4, CMAX = DF * (DF - 1) / 2 - 1 - 3 * N + 4 * DF,
                         OBS = 9 * N + 4 + 16 + 1, ACT = 2 * N, NDRAW = 1 + 2 * N + 2;
};
// RobotPuzzleBase(num_agents = N) (core.py:88,106,230): one T block (2 fixtures), N Robots (1 fixture), 4 walls
template <int N> struct DimsV3 {
    static constexpr int DF = 2 + N;
    static constexpr int V = 3, NA = N, NB = 1, NF = DF + 4, CMAX = DF * (DF - 1) / 2 - 1 + 4 * DF,
                         OBS = 4 * N + 3 + 16, ACT = 3 * N, NDRAW = 3 + 2 * N;
};
// v0 has v3's bodies, actions and draws; its observation carries one more word
template <int N> struct DimsV0 : DimsV3<N> {
    static constexpr int V = 0, OBS = 4 * N + 20;
};
template <int VERSION, int NA, int NB> struct DimsOf;   // a row no family covers does not compile
template <int N> struct DimsOf<0, N, 1> : DimsV0<N> {};
template <int N> struct DimsOf<2, N, 1> : DimsV2<N> {};
template <int N> struct DimsOf<3, N, 1> : DimsV3<N> {};
// Heavy-v2 with the build-defined 3-block square: its block fixtures are not a formula
template <> struct DimsOf<2, 2, 3> { static constexpr int V = 2, NA = 2, NB = 3, NF = 15, CMAX = 91, OBS = 69, ACT = 4, NDRAW = 9; };
template <int ENV> struct Dims : DimsOf<ENV_CFG[ENV].version, ENV_CFG[ENV].n_agents, ENV_CFG[ENV].n_blocks> {};

// Node pool of a lane's dynamic tree.  b2DynamicTree starts at 16 nodes and doubles only when
// all are live; a world holds at most 2 * proxies - 1 live nodes, so an env with <= 8 proxies
// never grows past 16 and its node ids (free-list order) never exceed 15.  A pool allocated at
// its final size with the free list in index order hands out the same ids as Box2D's doubling
// pool (the doubled part is appended to the free list in index order once the old part is full).
template <int ENV> constexpr int tree_n() {
    return 2 * Dims<ENV>::NF - 1 <= 16 ? 16 : (2 * Dims<ENV>::NF - 1 <= 32 ? 32 : 64);
}
// Move buffer: at most NF proxies are buffered between two UpdatePairs (every proxy after a
// reset's CreateProxy calls; a moved proxy at most once per Solve / TOI sub-step)
template <int ENV> constexpr int move_n() { return Dims<ENV>::NF < 16 ? 16 : 32; }

struct ShapeDef {
    int count;
    float radius;
    V2 v[MAX_POLY];
    V2 n[MAX_POLY];
};

// Body order everywhere: creation order of the reference = blocks, agents, walls.
struct EnvTables {
    int env_id, version, n_agents, n_blocks, n_dyn, n_bodies, n_fix, obs_dim, act_dim, n_draws, max_steps, pad;
    float mass[MAXBODY], invMass[MAXBODY], I[MAXBODY], invI[MAXBODY], lcx[MAXBODY], lcy[MAXBODY];
    float linDamp[MAXBODY], angDamp[MAXBODY];
    int body_fix0[MAXBODY], body_nfix[MAXBODY];
    int body_reset_mass[MAXBODY];      // 1 if any fixture had density > 0 (ResetMassData ran)
    float wall_px[4], wall_py[4];
    int fix_body[MAXF];
    float fix_friction[MAXF], fix_restitution[MAXF];
    ShapeDef shape[MAXF];
    int nverts[3];
    V2 verts[3][MAXV];
    double draw_lo[MAXDRAW], draw_hi[MAXDRAW];
    double block_px[3], block_py[3];   // v2: fixed spawn position per block
    float agent_angle;
    float pad2;
    double goal_x, goal_y, goal_a;     // v0 block_final_pos['t_block']
    double goal_off[3][3];             // 3-block: goal offsets (world m) + angle per block
};

// Reward / shaping parameters (set_reward_params, update_params, update_goal).
struct EnvParams {
    double w_dAgent, w_agentDist, w_dBlock, w_blkDist;
    double shaped_bounds, shaped_blk_bounds, shaped_puzzle;
    double scaled_epsilon;
    double puzzle_complete;            // v3 puzzle_complete_reward (core.py:155), added as is on completion
    int frameskip;                     // world.Step calls per env step (multi_robot_puzzle_02.py:139,476-478)
    int pad;
};

}  // namespace mrp
