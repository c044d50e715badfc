/*
 * mrp.h -- C ABI of the MI355X-native MultiRobotPuzzle step library (libmrp.so).
 *
 * Drop-in boundary for the gym_puzzles hot path.  In the reference the per-step work is
 * Python driving pybox2d object-by-object (~20 SWIG crossings per agent per step plus
 * C++->Python contact callbacks); here one call advances N independent worlds ("lanes")
 * on one GPU.  Each entry point names the reference interface it replaces.
 *
 * Conventions
 *   - Plain C types only; all arrays are row-major [n_lanes][dim].
 *   - Functions return 0 on success, a negative MRP_E* code on failure; mrp_last_error()
 *     gives the message (per context, or the last create failure when ctx == NULL).
 *   - "_device" variants take device pointers (hipMalloc / torch.cuda tensors) and are
 *     asynchronous on the context's stream; the plain variants take host pointers and
 *     synchronize.
 *   - Not re-entrant per context; one context per (device, stream, thread).
 *
 * env_id:  0 MultiRobotPuzzle-v0       (gym_puzzles/__init__.py:3-8,  multi_robot_puzzle_00.py:142)
 *          1 MultiRobotPuzzleHeavy-v0  (gym_puzzles/__init__.py:10-15, multi_robot_puzzle_00.py:606)
 *          2 MultiRobotPuzzle-v2       (gym_puzzles/__init__.py:17-22, multi_robot_puzzle_02.py:126)
 *          3 MultiRobotPuzzleHeavy-v2  (gym_puzzles/__init__.py:24-29, multi_robot_puzzle_02.py:711)
 *          4 MultiRobotPuzzleHeavy-v2 with the build-defined 3-block square
 *          5 MultiRobotPuzzle-v3       (gym_puzzles/__init__.py:31-35, core.py:77 RobotPuzzleBase)
 *          6 MultiRobotPuzzle-v3 constructed with heavy=True (gym_puzzles/tests/test_env.py:12)
 *          7-10  MultiRobotPuzzle2(num_agents=1, 3, 4, 5)      (multi_robot_puzzle_02.py:139,151,354)
 *          11-14 MultiRobotPuzzleHeavy2(num_agents=1, 3, 4, 5) (multi_robot_puzzle_02.py:711)
 *          15-18 RobotPuzzleBase(num_agents=1, 3, 4, 5)        (core.py:86-106,230)
 *          19-22 RobotPuzzleBase(num_agents=1, 3, 4, 5, heavy=True)
 */
#ifndef MRP_H
#define MRP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRP_OK 0
#define MRP_E_ARG (-1)     /* bad argument (env id, lane count, null pointer) */
#define MRP_E_HIP (-2)     /* HIP runtime error (no device, launch failure, OOM) */
#define MRP_E_STATE (-3)   /* call order violation (e.g. step before reset) */

/* lane status codes written by mrp_step (the reference's done_status strings) */
#define MRP_STATUS_RUNNING 0
#define MRP_STATUS_PUZZLE_COMPLETE 1   /* multi_robot_puzzle_00.py:515-519, _02.py:575-582 */
#define MRP_STATUS_AGENT_OOB 2         /* multi_robot_puzzle_02.py:552-556 */
#define MRP_STATUS_BLOCK_OOB 3         /* multi_robot_puzzle_02.py:558-562 */
/* flag bits OR-ed into the status byte (SURVEY.md 8b "Errors": per-lane NaN is reported, never a
 * crash; the reference would carry the NaN on silently, multi_robot_puzzle_00.py:521 returns {}) */
#define MRP_STATUS_KIND_MASK 0x3f
#define MRP_STATUS_NONFINITE 0x40      /* this step's observation or a dynamic body's state holds NaN/inf */
#define MRP_STATUS_FAULT 0x80          /* a loop guard has tripped in this lane (sticky; code: mrp_get_faults) */

typedef struct mrp_ctx mrp_ctx;

/* Static dimensions of an env id: observation_space / action_space shapes
 * (multi_robot_puzzle_00.py:186-207, _02.py:174-195), number of spawn draws per reset,
 * agents, blocks and the TimeLimit max_episode_steps (gym_puzzles/__init__.py:6-27).
 * MRP_E_STATE if the library's compiled layout of the env disagrees with its tables (a build defect). */
int mrp_env_dims(int env_id, int* obs_dim, int* act_dim, int* n_draws, int* n_agents, int* n_blocks,
                 int* max_episode_steps);

/* Create n_lanes worlds on HIP device `device`.  Replaces gym.make(id) ->
 * MultiRobotPuzzle.__init__ (multi_robot_puzzle_00.py:152-209): one Box2D.b2World per lane
 * (gravity 0, no sleep).  `seed` keys the on-device counter RNG (device resets, synthetic
 * actions); `lane_offset` is the global index of lane 0 (multi-GPU sharding keeps per-lane
 * streams identical for any GPU count).  Worlds are empty until mrp_reset. */
int mrp_create(int env_id, int n_lanes, int device, uint64_t seed, uint64_t lane_offset, mrp_ctx** out);
void mrp_destroy(mrp_ctx* ctx);
const char* mrp_last_error(const mrp_ctx* ctx);
int mrp_n_lanes(const mrp_ctx* ctx);
int mrp_env_id(const mrp_ctx* ctx);

/* Use this hipStream_t for all subsequent work; NULL selects the HIP null stream (torch's default
 * stream, cuda_stream == 0).  A new context runs on its own non-blocking stream until this is called. */
int mrp_set_stream(mrp_ctx* ctx, void* hip_stream);
int mrp_synchronize(mrp_ctx* ctx);

/* set_reward_params (multi_robot_puzzle_00.py:231-239, _02.py:216-225; v3 core.py:149-155, where
 * puzzle_comp is the completion bonus step() adds unshaped and the two penalties are unused). */
int mrp_set_reward_params(mrp_ctx* ctx, double agent_delta, double agent_distance, double block_delta,
                          double block_distance, double puzzle_comp, double out_of_bounds, double blk_out_of_bounds);
/* update_params(timestep, decay) (multi_robot_puzzle_00.py:241-243, _02.py:227-230; v3 stores a value
 * its step() never reads, core.py:158-159, so it changes nothing there). */
int mrp_update_params(mrp_ctx* ctx, double timestep, double decay);
/* update_goal(epoch, nb_epochs) (multi_robot_puzzle_00.py:245-246, _02.py:232-233). */
int mrp_update_goal(mrp_ctx* ctx, double epoch, double nb_epochs);

/* reset() (multi_robot_puzzle_00.py:392-411, _02.py:421-442) for the lanes whose
 * lane_mask byte is nonzero (NULL = all): destroy + rebuild the bodies in the reference's
 * order, then the reference's extra physics step with a random action.
 *   draws   [n_lanes][n_draws] float64: the np.random.uniform(...) values the reference
 *           draws (gym_puzzles_amd/spawn.py); NULL = device counter RNG.
 *   actions [n_lanes][act_dim] float32: the reset step's action_space.sample(); NULL = RNG.
 *   obs     [n_lanes][obs_dim] float32 out (rows of unmasked lanes are left untouched). */
int mrp_reset(mrp_ctx* ctx, const uint8_t* lane_mask, const double* draws, const float* actions, float* obs);
int mrp_reset_device(mrp_ctx* ctx, const uint8_t* d_lane_mask, const double* d_draws, const float* d_actions,
                     float* d_obs);

/* step(action) (multi_robot_puzzle_00.py:413-521, _02.py:444-584) under gym's TimeLimit
 * wrapper, for all lanes:
 *   actions  [n_lanes][act_dim] float32 (NULL = device RNG uniform[-1,1), keyed by lane/step)
 *   obs      [n_lanes][obs_dim] float32 out (the reference returns float64; values are
 *            float32(reference value))
 *   reward   [n_lanes] float32 out, done/truncated [n_lanes] uint8 out
 *            (truncated = TimeLimit.truncated), status [n_lanes] uint8 out (MRP_STATUS_*),
 *   terminal_obs [n_lanes][obs_dim] float32 out or NULL: when auto-reset is on, done lanes
 *            are reset on device (RNG spawns) and obs holds the new episode's first
 *            observation while terminal_obs holds the last one (SB3 VecEnv semantics).
 * Any output pointer except obs may be NULL. */
int mrp_step(mrp_ctx* ctx, const float* actions, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
             uint8_t* status, float* terminal_obs);
int mrp_step_device(mrp_ctx* ctx, const float* d_actions, float* d_obs, float* d_reward, uint8_t* d_done,
                    uint8_t* d_truncated, uint8_t* d_status, float* d_terminal_obs);
/* As mrp_step / mrp_step_device, plus `reward64` [n_lanes] float64 out (may be NULL): the reward
 * exactly as the reference returns it (a Python float, multi_robot_puzzle_00.py:521,
 * _02.py:584), before the float32 rounding of `reward`.  Monitor's episode return sums these. */
int mrp_step_ex(mrp_ctx* ctx, const float* actions, float* obs, float* reward, double* reward64, uint8_t* done,
                uint8_t* truncated, uint8_t* status, float* terminal_obs);
int mrp_step_device_ex(mrp_ctx* ctx, const float* d_actions, float* d_obs, float* d_reward, double* d_reward64,
                       uint8_t* d_done, uint8_t* d_truncated, uint8_t* d_status, float* d_terminal_obs);
/* n_steps consecutive step() calls of every lane in ONE launch (synthetic rollouts, evaluation
 * with device-RNG or pre-computed actions): the lane state stays on chip between the steps, and
 * each step writes its outputs exactly as one mrp_step_device_ex would (step s of lane l at row
 * s * n_lanes + l of every array: d_actions [n_steps][n_lanes][act_dim] or NULL = device RNG,
 * d_obs / d_terminal_obs [n_steps][n_lanes][obs_dim], the others [n_steps][n_lanes]).  The result
 * is bit-identical to n_steps single steps; lanes advance independently inside the launch. */
int mrp_step_n_device(mrp_ctx* ctx, int n_steps, const float* d_actions, float* d_obs, float* d_reward, double* d_reward64,
                      uint8_t* d_done, uint8_t* d_truncated, uint8_t* d_status, float* d_terminal_obs);
int mrp_set_auto_reset(mrp_ctx* ctx, int enabled);
/* frameskip: world.Step(1/50, 180, 60) calls per env step, 1-64 (default 1).  Replaces the
 * MultiRobotPuzzle2(frameskip=k) constructor argument (multi_robot_puzzle_02.py:139,146,476-478:
 * `for _ in range(self.frameskip): self.world.Step(...)`; the reset's extra step takes it too). */
int mrp_set_frameskip(mrp_ctx* ctx, int frameskip);
/* Re-key the device counter RNG (spawns of later resets, synthetic actions) without touching the
 * lanes, parameters, stream or time limit: SB3 VecEnv.seed(seed) (train/train.py:63-75 seeds
 * every env before the first reset).  Per-lane streams stay keyed by the global lane index. */
int mrp_set_seed(mrp_ctx* ctx, uint64_t seed);
/* Lane scheduling: with costliest_first = 1 each step dispatches the lanes in descending order of
 * their previous step's cost, so the long serial solver chains start first (one small sort kernel
 * per step); 0 keeps lane order.  Results never depend on it.  The default is per env id, set by
 * mrp_create: on for Heavy-v0 (env 1) and v3 (env 5) when n_lanes exceeds the lanes k_step keeps
 * resident at once (CUs x 4 SIMDs x its waves per SIMD), off otherwise (round-4 A/B, DESIGN.md:
 * Heavy-v0 +4 %, v3 +1-2 %; v0 -0.9 % at 4096 lanes and -3..-5 % at 1024). */
int mrp_set_schedule(mrp_ctx* ctx, int costliest_first);
/* the context's current lane scheduling mode (the per-env default until mrp_set_schedule) */
int mrp_get_schedule(const mrp_ctx* ctx);
/* TimeLimit max_episode_steps applied inside mrp_step (default: the registered value of
 * gym_puzzles/__init__.py:6-27); 0 disables it (when an outer gym.wrappers.TimeLimit is used). */
int mrp_set_time_limit(mrp_ctx* ctx, int max_episode_steps);

/* Introspection (tests, checkpointing).  Dynamic bodies in creation order (blocks, agents),
 * 6 floats each: worldCenter.x, worldCenter.y, angle, linearVelocity.x, .y, angularVelocity. */
int mrp_get_bodies(mrp_ctx* ctx, float* out /* [n_lanes][6*(n_blocks+n_agents)] */);
/* per lane: goal_contact flags [n_agents] then blks_in_place -> int32 [n_lanes][n_agents+1] */
int mrp_get_flags(mrp_ctx* ctx, int32_t* out);
/* per lane: 0, or the code of the loop guard that ended a runaway loop in that lane (a bound no
 * valid world reaches: tree walks, contact-list walks, islands, TOI passes; see mrp_world.h
 * MRP_FAULT_*: 1-8 loop guards -- tree walks, contact-list walks, islands, TOI passes, pair decoding,
 * island DFS; 9-12 pool guards -- tree nodes, contact slots, move buffer, island arrays).  Sticky.
 * int32 [n_lanes] */
int mrp_get_faults(mrp_ctx* ctx, int32_t* out);
/* summed over lanes: TOI events and position-solver iterations (diagnostics) */
int mrp_counters(mrp_ctx* ctx, int64_t* toi_events, int64_t* pos_iters);
/* per-batch counters (SURVEY.md 5 "Metrics"), summed over lanes since mrp_create, reduced on the
 * device: out[8] = steps, resets, TOI events, position iterations, touching contacts (after each
 * world.Step's Collide), lane-steps with a non-finite output, lanes with a tripped loop guard, 0 */
int mrp_counters_ex(mrp_ctx* ctx, int64_t* out8);
/* Raw per-lane state (checkpoint / resume): mrp_state_words() 32-bit words per lane. */
int mrp_state_words(int env_id);
int mrp_get_state(mrp_ctx* ctx, uint32_t* out /* [n_lanes][state_words] */);
int mrp_set_state(mrp_ctx* ctx, const uint32_t* in);

/* rgb_array rendering, replacing render(mode='rgb_array') of
 * gym_puzzles/envs/multi_robot_puzzle_00.py:528-592 and multi_robot_puzzle_02.py:590-661
 * (_render_human_vision).  Renders the n selected lanes into uint8 RGB images
 * [n][height][width][3], row 0 at the top (the reference's `arr[::-1]`, :598); the full-size
 * viewport is 640x480 (v0) / 1440x810 (v2), other sizes resample the same scene.  The
 * rasteriser is defined in gym_puzzles_amd/csrc/mrp_render.h.  _device: device pointers,
 * asynchronous on the ctx stream; plain: host pointers, synchronous. */
int mrp_render_device(mrp_ctx* ctx, const int32_t* d_lanes, int n, int width, int height, uint8_t* d_rgb);
int mrp_render(mrp_ctx* ctx, const int32_t* lanes, int n, int width, int height, uint8_t* rgb);
/* Pixel observations ('image' obs_type, multi_robot_puzzle_00.py:148-162,197-200): the next frame
 * stack of every lane.  next/prev: uint8 [n_lanes][depth][height][width][channels].
 * Per lane, slot depth-1 (the newest) is the frame of the lane's current state, drawn by the
 * rasteriser of mrp_render at width x height: channels 3 stores R, G, B, channels 1 the integer luma
 * (77 R + 150 G + 29 B + 128) >> 8.  Slot k < depth-1 is slot k+1 of `prev`; with prev NULL, or for a
 * lane whose `done` byte is nonzero (NULL: none), those slots are zero, as the reference starts an
 * episode's image state from zeros.  The slots are stacked vertically, oldest first: a lane's block
 * read as [depth*height][width][channels] is the observation.  One launch covers all lanes.
 * MRP_E_ARG: channels not 1 or 3, depth outside 1..16, a size mrp_render refuses, a null ctx or
 * next, prev == next with depth > 1 (the shift is not done in place); MRP_E_STATE before the first
 * reset.  _device: device pointers, asynchronous on the ctx stream; plain: host pointers, synchronous. */
int mrp_pixels_device(mrp_ctx* ctx, int width, int height, int channels, int depth,
                      const uint8_t* d_done, const uint8_t* d_prev, uint8_t* d_next);
int mrp_pixels(mrp_ctx* ctx, int width, int height, int channels, int depth,
               const uint8_t* done, const uint8_t* prev, uint8_t* next);
/* per lane block_final_pos (x, y, angle) per block, in the units of the reference's
 * block_final_pos (v0 px, v2 scaled units): double [n_lanes][n_blocks][3] */
int mrp_get_goals(mrp_ctx* ctx, double* out);
/* host-only: the env's fixture geometry (creation order; local vertices, 16 fixtures x 8
 * vertices x (x, y); unused entries 0 / fix_body -1) */
int mrp_shapes(int env_id, int32_t* n_fix, int32_t* fix_body, int32_t* counts, float* verts);

/* Device self-test of the glibc-faithful sinf/cosf of every b2Rot::Set on the GPU: evaluates
 * b2Rot::Set (sin, cos) as the step does on device `device` for n host inputs (host output arrays). */
int mrp_selftest_sincos(int device, const float* x, float* sin_out, float* cos_out, int n);
/* Diagnostic builds (-DMRP_STAMPS) only: per-phase cycle totals of thread 0 since the last call
 * (returns MRP_E_STATE in the shipped build). */
int mrp_debug_stamps(int device, uint64_t* out16);
/* Diagnostic builds only: per-phase maxima over lane-steps, the slowest lane's total per step
 * (256 slots, indexed by step counter mod 256) and the (s_memtime, s_memrealtime) sums of lane
 * totals since the last call. */
int mrp_debug_stamps_ext(int device, uint64_t* pmax16, uint64_t* stepmax256, uint64_t* rt2);
/* Diagnostic builds only: the last step's per-lane trace, n_lanes x MRP_TRACE_WORDS words (phase
 * cycles 0-10, total, island contacts, TOI events, position iterations, velocity-solver contact
 * units, velocity-sweep / position-pass / island set-up cycles, the TOI split (20-21), the collide
 * split (22-23), the lane timeline words (24-31), then the solve's thread-0 bookkeeping (32 island
 * building, 33 island write-back + integration, 34 fixture synchronisation) and the TOI scan alone (35)).  `out` must hold n_lanes * mrp_debug_trace_words()
 * words; it is left untouched (MRP_E_STATE) when the library has no diagnostic unit. */
#define MRP_TRACE_WORDS 40
int mrp_debug_trace_words(void);
int mrp_debug_trace(int device, uint32_t* out, int n_lanes);
/* Diagnostic builds (-DMRP_PROGRESS) only: allocate n_lanes host-mapped words that every lane's
 * thread 0 overwrites with the last progress point it reached; readable while a launch runs
 * (hang localisation).  Returns MRP_E_STATE in the shipped build. */
int mrp_debug_progress(int device, uint32_t** host_words, int n_lanes);
/* Diagnostic micro-benchmark: `blocks` workgroups each sweep a synthetic v0 island (nc agent-block
 * contacts of pcount points) `iters` times with the early exit off; cycles[block] = s_memtime
 * cycles of the sweeps (per-contact-update cost = cycles / (iters * nc)). */
int mrp_debug_velbench(int device, int nc, int pcount, int iters, int blocks, uint64_t* cycles);
/* Diagnostic micro-benchmark: `blocks` workgroups each run the position passes (up to `iters`) of a
 * synthetic island of nc static-wall contacts of pcount points squeezing one block (the passes never
 * reach the exit test); out[2 * block] = s_memtime cycles, out[2 * block + 1] = passes run. */
int mrp_debug_posbench(int device, int nc, int pcount, int iters, int blocks, uint64_t* out);

/* ------------------------------------------------------------------------------------------
 * On-device VecNormalize + Monitor statistics.  Replaces the host-side
 * stable-baselines3 wrappers the reference trains with: Monitor(env) per env
 * (train/train.py:68) and VecNormalize(DummyVecEnv(...)) with default arguments
 * (train/train.py:80-82; loaded back by train/test.py:66).  The statistics live on the device;
 * inputs and outputs are device arrays of a step's outputs ([n_lanes][obs_dim] float32 obs,
 * [n_lanes] float32 reward, uint8 done).  Asynchronous on the context's stream.
 * ------------------------------------------------------------------------------------------ */
typedef struct mrp_norm mrp_norm;

/* VecNormalize(clip_obs, clip_reward, gamma, epsilon); RunningMeanStd(epsilon=1e-4) for obs and returns */
int mrp_norm_create(int n_lanes, int obs_dim, int device, double clip_obs, double clip_reward, double gamma, double epsilon,
                    mrp_norm** out);
void mrp_norm_destroy(mrp_norm* n);
const char* mrp_norm_last_error(const mrp_norm* n);
int mrp_norm_set_stream(mrp_norm* n, void* hip_stream);   /* as mrp_set_stream: NULL = the HIP null stream */
/* VecNormalize.training: statistics update on (1) or frozen (0, evaluation) */
int mrp_norm_set_training(mrp_norm* n, int training);
/* VecNormalize.norm_obs: with 0 the observation statistics are not updated (SB3 updates obs_rms
 * only when training and norm_obs); the normalised outputs are still written */
int mrp_norm_set_norm_obs(mrp_norm* n, int norm_obs);
/* VecNormalize.reset: update obs statistics, normalise obs, zero the discounted returns and
 * the Monitor accumulators */
int mrp_norm_reset_device(mrp_norm* n, const float* d_obs, float* d_obs_out);
/* VecNormalize.step_wait + Monitor.step: normalised obs / reward (and terminal obs of done
 * lanes, optional), returns[done] = 0; for done lanes the finished episode's return (float64
 * sum of raw rewards) and length (Monitor's info["episode"] r / l; optional outputs) */
int mrp_norm_step_device(mrp_norm* n, const float* d_obs, const float* d_reward, const uint8_t* d_done, const float* d_term_obs,
                         float* d_obs_out, float* d_reward_out, float* d_term_out, double* d_ep_return, int32_t* d_ep_len);
/* As mrp_norm_step_device; with d_reward64 (mrp_step_device_ex's float64 rewards, may be NULL) the
 * Monitor episode return sums the env's float64 rewards, as SB3's Monitor does (train/train.py:68). */
int mrp_norm_step_device_ex(mrp_norm* n, const float* d_obs, const float* d_reward, const double* d_reward64,
                            const uint8_t* d_done, const float* d_term_obs, float* d_obs_out, float* d_reward_out,
                            float* d_term_out, double* d_ep_return, int32_t* d_ep_len);
/* ---- Data-parallel VecNormalize: one set of running statistics over the lanes of all R ranks, each rank with
 * n_lanes lanes (vec_env.py moments_local_ref / moments_combine_ref; every operation float64 and rounded on
 * its own).  A reset or step is the local phase, the caller's all-gather of the ranks' parts in rank order,
 * and the apply phase; every rank then holds the same bits.  Discounted returns and Monitor stay per lane.
 *   part     float64 [mrp_norm_part_len(obs_dim)] = 2 * (obs_dim + 1): for statistic column c (the obs
 *            columns, then the discounted returns) part[2c] = the mean over this rank's lanes and
 *            part[2c + 1] = M2 = sum((x - mean)^2), not divided by n.
 * mrp_norm_local_device: one launch.  With step != 0 it first advances returns = returns * gamma + reward
 * (d_reward required) while training.  Only the columns that move are written: the obs columns when training
 * and norm_obs, the returns column on a step while training; when nothing moves nothing is launched.
 * mrp_norm_apply_device: d_parts is float64 [R][part_stride], row r from rank r.  One thread per moving
 * column folds the rows in ascending rank order (na = n_lanes; per row d = mb - ma, nt = na + n_lanes,
 * Ma = Ma + Mb + d*d*na*n_lanes/nt, ma = ma + d*n_lanes/nt, na = nt) and merges (ma, Ma / na, na) into the
 * running statistics; then the normalisation of mrp_norm_step_device_ex (step != 0) or mrp_norm_reset_device
 * (step == 0: only d_obs and d_obs_out are read), with the obs count advanced by R * n_lanes.  With R = 1
 * the two phases give mrp_norm_step_device_ex's bits.
 * MRP_E_ARG, before the first HIP call: a null required pointer, R < 1, part_stride < the part length,
 * d_part overlapping an input, d_parts overlapping an output.  Asynchronous on the context's stream. */
int mrp_norm_part_len(int obs_dim);   /* MRP_E_ARG for obs_dim < 1 */
int mrp_norm_local_device(mrp_norm* n, const float* d_obs, const float* d_reward, int step, double* d_part);
int mrp_norm_apply_device(mrp_norm* n, int R, const double* d_parts, long long part_stride, int step, const float* d_obs,
                          const float* d_reward, const double* d_reward64, const uint8_t* d_done, const float* d_term_obs,
                          float* d_obs_out, float* d_reward_out, float* d_term_out, double* d_ep_return, int32_t* d_ep_len);
/* statistics as float64[2*obs_dim + 4]: obs mean[obs_dim], obs var[obs_dim], obs count,
 * return mean, return var, return count (VecNormalize save/load) */
int mrp_norm_get_stats(mrp_norm* n, double* out);
int mrp_norm_set_stats(mrp_norm* n, const double* in);

/* SB3 RolloutBuffer.compute_returns_and_advantage (+ collect_rollouts' TimeLimit bootstrap) for
 * n_lanes lanes x n_steps rows in one launch on `hip_stream` (NULL = the null stream) of `device`.
 * All arrays are device pointers, row-major [n_steps][n_lanes] except d_last_values / d_last_dones
 * [n_lanes].  d_truncated and d_terminal_values are both NULL (no bootstrap) or both given.
 * An output may overlap no input and not the other output (byte extents, so a view into an input's
 * allocation that starts where the input ends is fine).  Asynchronous.
 * The rule, which the kernel matches bit for bit, is gym_puzzles_amd.rollout.gae_ref: truncated
 * elements first get reward += float32(gamma) * terminal_value (float32); then, from the last row
 * down, with nnt = 1 - (d_last_dones on the last row, the next row's episode_starts otherwise) and
 * nv = d_last_values / the next row's values, a float64 accumulator L per lane:
 *   last row : L = ((double)r + (double)(g32 * nv) * nnt) - (double)v
 *   other    : L = (double)((r + (g32 * nv) * nnt) - v) + (double)(c32 * nnt) * L
 * with g32 = (float)gamma, c32 = (float)(gamma * gae_lambda), every operation rounded separately;
 * advantages = (float)L, returns = advantages + values (float32).
 * MRP_E_ARG: n_steps < 1, n_lanes < 1, a null required pointer, one bootstrap array without the
 * other, an output that overlaps an input or the other output, a device index out of range.
 * MRP_E_HIP: no device, launch failure.  The message is read with mrp_norm_last_error(NULL). */
int mrp_gae_device(int device, void* hip_stream, int n_steps, int n_lanes,
                   const float* d_rewards, const float* d_values, const uint8_t* d_episode_starts,
                   const uint8_t* d_truncated, const float* d_terminal_values,
                   const float* d_last_values, const uint8_t* d_last_dones,
                   double gamma, double gae_lambda, float* d_advantages, float* d_returns);

/* ------------------------------------------------------------------------------------------
 * Device policy: SB3's ActorCriticPolicy with MlpExtractor (forward pass, diagonal-Gaussian
 * sampling, log-prob, value, action clipping) for a batch of lanes in one launch.  The rule,
 * which the kernel matches bit for bit, is gym_puzzles_amd.policy.policy_ref (DESIGN.md "Device
 * policy"): n_shared trunk layers, then n_pi policy-tower and n_vf value-tower layers, each
 * Linear + activation, a linear action head (act_dim outputs), a linear value head and a
 * state-independent log_std[act_dim]; every Linear is a float32 fmaf chain in ascending k from
 * the bias.  Limits: obs_dim and every width 1..256, act_dim 1..16, n_shared + max(n_pi, n_vf)
 * <= 4 (all three may be 0).
 * ------------------------------------------------------------------------------------------ */
typedef struct mrp_policy mrp_policy;
#define MRP_POLICY_TANH 0
#define MRP_POLICY_RELU 1

/* widths: n_shared + n_pi + n_vf layer widths (trunk, policy tower, value tower).  MRP_E_ARG for
 * dims or counts outside the limits (message: mrp_policy_last_error(NULL)). */
int mrp_policy_create(int device, int obs_dim, int act_dim, int n_shared, int n_pi, int n_vf, const int* widths,
                      int activation, mrp_policy** out);
void mrp_policy_destroy(mrp_policy* p);
const char* mrp_policy_last_error(const mrp_policy* p);
/* The length of the flat parameter vector: SB3's parameters() order, log_std, then trunk, policy
 * tower, value tower, action head, value head, each weight row-major [out][in], then bias. */
int mrp_policy_n_params(const mrp_policy* p);
/* Host pointers: flat[mrp_policy_n_params] in that order and std[act_dim], std[i] being
 * float32(exp(float64(log_std[i]))), computed by the caller.  Packs the weights for the kernel and
 * copies them; synchronises the device. */
int mrp_policy_set_params(mrp_policy* p, const float* flat, const float* std);
/* One launch on `hip_stream` (NULL = the null stream): d_obs [n_lanes][obs_dim]; noise d_eps_in
 * [n_lanes][act_dim], or NULL for the device counter RNG keyed by (seed, lane_offset + lane,
 * counter * act_dim + i) (Box-Muller in float64 rounded to float32); deterministic: action = mean.
 * Outputs: d_actions [n_lanes][act_dim] (unclipped, what SB3 stores), optional d_clipped (what
 * steps the env), d_values [n_lanes], d_log_probs [n_lanes] and d_eps_out (the noise used).
 * MRP_E_ARG: n_lanes < 1, a null d_obs / d_actions, an output that overlaps an input or another
 * output; MRP_E_STATE before mrp_policy_set_params.  Asynchronous. */
int mrp_policy_act_device(mrp_policy* p, void* hip_stream, int n_lanes, const float* d_obs, const float* d_eps_in,
                          uint64_t seed, uint64_t lane_offset, uint64_t counter, int deterministic, float* d_actions,
                          float* d_clipped, float* d_values, float* d_log_probs, float* d_eps_out);
/* Trunk + value tower + value head only (V(terminal_obs), last_values): the same bits as
 * mrp_policy_act_device's d_values. */
int mrp_policy_values_device(mrp_policy* p, void* hip_stream, int n_lanes, const float* d_obs, float* d_values);
/* Device self-test of the policy's tanh rule (mrp_math.h tanh_f32) on n host inputs (host output). */
int mrp_selftest_tanh(int device, const float* x, float* out, int n);
/* The device's parameters as mrp_policy_set_params takes them: its inverse, e.g. after
 * mrp_ppo_step_device.  Synchronises the device.  MRP_E_ARG: a null pointer; MRP_E_STATE before
 * mrp_policy_set_params. */
int mrp_policy_get_params(mrp_policy* p, float* flat, float* std);

/* ---------------------------------------------------------------------------------------------
 * Device PPO update: one optimiser step of SB3's PPO.train() on a minibatch (evaluate_actions, the
 * clipped surrogate / value / entropy losses, the backward pass, global grad-norm clipping, Adam),
 * written into the policy's device parameters in place, with no host synchronisation and no
 * atomics.  The rule, which the kernels match bit for bit, is gym_puzzles_amd.ppo.ppo_grad_ref /
 * adam_ref (DESIGN.md "Device PPO update").  The flat parameter order is mrp_policy_n_params's.
 * --------------------------------------------------------------------------------------------- */
typedef struct mrp_ppo mrp_ppo;
/* The optimiser of one policy (which must outlive it: every call reads it; one mrp_ppo per policy): master parameters,
 * gradient, Adam moments (zero) and a workspace for minibatches of up to max_batch samples.
 * MRP_E_ARG: a null pointer, max_batch outside 1..1048576 (message: mrp_ppo_last_error(NULL)).  A
 * later mrp_policy_set_params is picked up by the next call; the moments stay. */
int mrp_ppo_create(mrp_policy* policy, int max_batch, mrp_ppo** out);
void mrp_ppo_destroy(mrp_ppo* o);
const char* mrp_ppo_last_error(const mrp_ppo* o);
/* The length of the flat parameter vector: its policy's mrp_policy_n_params. */
int mrp_ppo_n_params(const mrp_ppo* o);
/* Gradients and statistics only: d_grad [n_params] takes the flat gradient before clipping, d_stats
 * [5] the policy loss, value loss, entropy loss, approx_kl and clip fraction.  Inputs: float32 device
 * arrays d_obs [B][obs_dim], d_actions [B][act_dim] (the stored, unclipped actions), d_old_log_probs,
 * d_advantages, d_returns [B].  Parameters and moments are not written.  MRP_E_ARG: B < 1, B >
 * max_batch, a null pointer, an output that overlaps an input or the other output; MRP_E_STATE before
 * mrp_policy_set_params.  Asynchronous. */
int mrp_ppo_grad_device(mrp_ppo* o, void* hip_stream, int B, const float* d_obs, const float* d_actions,
                        const float* d_old_log_probs, const float* d_advantages, const float* d_returns, float clip_range,
                        float ent_coef, double vf_coef, float* d_grad, float* d_stats);
/* Gradients, clip and Adam; the policy's parameters (std = exp_f32(log_std) included) are updated
 * in place for the next mrp_policy_act_device on the same stream.  The Adam scalars of step t are
 * computed by the caller in float64 and passed as float32: beta1, 1 - beta1, beta2, 1 - beta2,
 * sqrt(1 - beta2^t), lr / (1 - beta1^t), eps.  Errors as mrp_ppo_grad_device.  Asynchronous. */
int mrp_ppo_step_device(mrp_ppo* o, void* hip_stream, int B, const float* d_obs, const float* d_actions,
                        const float* d_old_log_probs, const float* d_advantages, const float* d_returns, float clip_range,
                        float ent_coef, double vf_coef, double max_grad_norm, float beta1, float one_minus_beta1, float beta2,
                        float one_minus_beta2, float sqrt_bc2, float step_size, float eps, float* d_stats);
/* Host copies of Adam's moments, n_params floats each.  Synchronises the device. */
int mrp_ppo_get_state(mrp_ppo* o, float* m, float* v);
/* ---- SB3's train() loop with target_kl, clip_range_vf and the minibatch gather on the device.  The
 * object keeps three device words: `stopped` (a minibatch's approx_kl exceeded 1.5 * target_kl: that
 * minibatch was not applied and nothing after it runs), `applied` (optimiser steps applied) and a sticky
 * `bad_index`.  mrp_ppo_begin_device clears them (asynchronous); a train() call is one begin and one
 * mrp_ppo_minibatch_device per minibatch, with no host synchronisation in between. */
int mrp_ppo_begin_device(mrp_ppo* o, void* hip_stream);
/* One minibatch of B samples under the predicate: every kernel first loads `stopped` and returns when it
 * is set, so a skipped minibatch writes nothing, its d_stats row included.
 *   fields   d_obs [rows][obs_dim], d_actions [rows][act_dim], d_old_values, d_old_log_probs, d_advantages,
 *            d_returns [rows] (float32).  d_index (int64 [B]) names the minibatch's rows among rows = n_rows
 *            (a rollout buffer's flat [T * N] view): they are gathered into the object's staging buffers.  An
 *            index outside [0, n_rows) reads row 0 and sets bad_index (mrp_ppo_progress reports it).
 *            d_index NULL: the fields are the B rows themselves (n_rows is ignored).
 *   options  normalize_advantage != 0: the (staged) advantages are normalised by ppo.normalize_adv_ref
 *            (skipped for B = 1); clip_range_vf < 0: none (d_old_values may be NULL and is not read), else
 *            SB3's value clipping; target_kl < 0: none, else ppo.kl_stop_ref decides on the device.
 *   d_grad   non-NULL: the gradient before clipping and the statistics only, as mrp_ppo_grad_device: no
 *            clip, no Adam, no stop.  NULL: the step, with the Adam scalars of mrp_ppo_step_device.
 * MRP_E_ARG as mrp_ppo_grad_device (the alias rule covers d_index and every field over all its rows), and:
 * clip_range_vf >= 0 with d_old_values NULL, n_rows < 1.  No allocation, no synchronisation. */
int mrp_ppo_minibatch_device(mrp_ppo* o, void* hip_stream, int B, const long long* d_index, long long n_rows,
                             const float* d_obs, const float* d_actions, const float* d_old_values,
                             const float* d_old_log_probs, const float* d_advantages, const float* d_returns,
                             int normalize_advantage, float clip_range, float clip_range_vf, double target_kl, float ent_coef,
                             double vf_coef, double max_grad_norm, float beta1, float one_minus_beta1, float beta2,
                             float one_minus_beta2, float sqrt_bc2, float step_size, float eps, float* d_grad, float* d_stats);
/* Synchronises the stream and returns the words.  MRP_E_ARG (with both words still returned) when
 * bad_index is set. */
int mrp_ppo_progress(mrp_ppo* o, void* hip_stream, int* stopped, int* applied);
/* Host copies of the first B rows of the staging buffers as the last indexed or normalising
 * mrp_ppo_minibatch_device left them (NULL outputs are skipped; old_values are staged only under
 * clip_range_vf).  Synchronises the device.  For tests. */
int mrp_ppo_get_staged(mrp_ppo* o, int B, float* obs, float* actions, float* old_values, float* old_log_probs,
                       float* advantages, float* returns);
/* ---- Data-parallel PPO: the apply phase.  Every rank computes its minibatch's gradient before clipping and
 * its statistics (mrp_ppo_minibatch_device with d_grad), the ranks exchange them, and every rank applies the
 * same combined step, so the replicas stay bit-identical (ppo.combine_ref, ppo.ppo_train_dist_ref).
 *   d_parts  float32 [R][part_stride]: row r holds rank r's flat gradient in its first n_params floats and
 *            its five statistics at [n_params, n_params + 5); the rest of a row is padding and is not read.
 * Three launches under the predicate of mrp_ppo_minibatch_device (every kernel first loads `stopped`; a
 * skipped call writes nothing, d_stats included): the rows are added in ascending rank order with plain
 * float32 adds and multiplied by float32(1 / R) into the object's gradient vector and into d_stats [5]; then
 * the grad-norm clip, the target_kl decision (< 0: none) on the combined approx_kl, and Adam with the scalars
 * of mrp_ppo_step_device, which advances `applied`.  MRP_E_ARG: R outside 1..64, part_stride < n_params + 5,
 * a null pointer, d_stats overlapping any of the R * part_stride floats of d_parts; MRP_E_STATE before
 * mrp_policy_set_params.  No allocation, no synchronisation. */
int mrp_ppo_apply_device(mrp_ppo* o, void* hip_stream, int R, const float* d_parts, long long part_stride,
                         double target_kl, double max_grad_norm, float beta1, float one_minus_beta1, float beta2,
                         float one_minus_beta2, float sqrt_bc2, float step_size, float eps, float* d_stats);
/* Adam's moments from host arrays of n_params floats each: the inverse of mrp_ppo_get_state (a replica
 * that starts from another rank's optimiser state, a resumed checkpoint).  Synchronises the device. */
int mrp_ppo_set_state(mrp_ppo* o, const float* m, const float* v);
/* Device self-test of the exp rule (mrp_math.h exp_f32) on n host inputs (host output). */
int mrp_selftest_exp(int device, const float* x, float* out, int n);

#ifdef __cplusplus
}
#endif
#endif
