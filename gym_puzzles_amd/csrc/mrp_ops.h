// mrp_ops.h -- the per-env launch table between the C ABI (mrp_kernels.hip) and the per-env
// kernel translation units (mrp_unit.hip, compiled once per env id with -DMRP_ENV=<id>).
//
// Every env id is its own template instantiation of the whole lane step (k_step<ENV> and
// friends), and each instantiation is compiled in its own translation unit so the N_ENVS
// builds run in parallel (build.py).  A translation unit exports one EnvOps: plain host
// functions that launch its kernels on a given stream.  The C ABI never names a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "mrp_config.h"

namespace mrpr {
struct RenderArgs {
    float sx, sy;              // world units per pixel
    float lw_unit;             // world units per viewport pixel (line widths)
    float ring_r;              // v2: scaled_epsilon / RATIO
    double goal_scale;         // lane goal units -> world metres
};
constexpr int RBLOCK = 256;
constexpr int RPPT = 8;        // pixels per thread: one display-list build serves RBLOCK*RPPT pixels
constexpr int PIX_BLOCK = 256, PIX_CHUNK = 16384;   // k_pixels: threads per workgroup, pixels per workgroup (mrp_pixels.h)
}  // namespace mrpr

namespace mrp {

// k_step's arguments (mrp_step_device_ex)
struct StepArgs {
    uint32_t* state;
    int nl;
    const float* actions;      // NULL: device RNG
    float* obs;
    float* reward;
    double* reward64;
    uint8_t* done;
    uint8_t* trunc;
    uint8_t* status;
    float* term_obs;
    EnvParams P;
    uint64_t seed, lane_offset;
    int auto_reset, max_steps;
    const int* order;          // NULL: workgroup b steps lane b
    uint32_t* cost;            // NULL: no per-lane cycle record
    const uint32_t* costmax;   // NULL: no cost-derived priority
    int nsteps;                // env steps per launch (mrp_step_n_device); step s of lane l writes row s * nl + l
};

// per-lane counters summed over the lanes (mrp_counters_ex), in this order
enum : int { CTR_STEPS = 0, CTR_RESETS, CTR_TOI, CTR_POS_ITERS, CTR_TOUCHING, CTR_NONFINITE, CTR_FAULT_LANES, CTR_N = 8 };

// diagnostic symbols of a -DMRP_STAMPS / -DMRP_PROGRESS build (debug_read's `what`)
enum : int { DBG_STAMPS = 0, DBG_PMAX = 1, DBG_STEPMAX = 2, DBG_RT = 3, DBG_TRACE = 4 };

struct EnvOps {
    int words;                 // lane_words<ENV>()
    int dims[6];               // Dims<ENV>: OBS, ACT, NDRAW, NA, NB, NF (mrp_create checks them against the tables)
    int step_waves_per_eu;     // k_step's launch bound: resident waves per SIMD (mrp_create: resident lanes)
    // host arithmetic on n_lanes lane states (mrp_set_state): raise every lane's contact high-water
    // mark cHW to cover its non-initial slots (mrp_lane.h StateIO::repair_marks)
    void (*repair_marks)(uint32_t* state, size_t n_lanes);
    hipError_t (*upload_tables)(const EnvTables& t);   // this env's tables -> its unit's __constant__ copy
    void (*init)(hipStream_t, uint32_t* state, int nl);
    void (*reset)(hipStream_t, uint32_t* state, int nl, const uint8_t* mask, const double* draws, const float* actions,
                  float* obs, const EnvParams& P, uint64_t seed, uint64_t lane_offset);
    void (*step)(hipStream_t, const StepArgs& a);
    void (*bodies)(hipStream_t, const uint32_t* state, int nl, float* out, int32_t* flags);
    void (*faults)(hipStream_t, const uint32_t* state, int nl, int32_t* out);
    void (*counters)(hipStream_t, const uint32_t* state, int nl, int64_t* out /* [CTR_N] */);
    void (*render)(hipStream_t, dim3 grid, const uint32_t* state, const int32_t* lanes, int nl, int W, int H,
                   const mrpr::RenderArgs& A, uint8_t* rgb);
    // the next frame stack of every lane (mrp_pixels_device; grid: lanes x chunks of the frame)
    void (*pixels)(hipStream_t, dim3 grid, const uint32_t* state, int nl, int W, int H, int C, int depth,
                   const mrpr::RenderArgs& A, const uint8_t* done, const uint8_t* prev, uint8_t* next);
    void (*goals)(hipStream_t, const uint32_t* state, int nl, double* out);
    // diagnostic builds only (MRP_E_STATE-like hipErrorNotSupported otherwise): copy `bytes` of
    // symbol `what` into `out` and zero it; point the progress word array at `dev_words`
    hipError_t (*debug_read)(int what, void* out, size_t bytes);
    hipError_t (*debug_progress)(uint32_t* dev_words);
};

// one EnvOps per row of the registry (mrp_config.h), defined by the unit compiled with MRP_ENV = id
#define MRP_ENV_OPS_NAME(id) g_env_ops_##id
#define MRP_ENV_OPS_DECL(id, ...) extern const EnvOps MRP_ENV_OPS_NAME(id);
MRP_ENV_LIST(MRP_ENV_OPS_DECL)
#undef MRP_ENV_OPS_DECL
// defined in env 0's unit: the lane-distributed velocity-sweep micro-benchmark (mrp_debug_velbench)
// and the position-pass micro-benchmark (mrp_debug_posbench), on v0's tables
hipError_t velbench_launch(const EnvTables& v0, int nc, int pcount, int iters, int blocks, unsigned long long* d_out);
hipError_t posbench_launch(const EnvTables& v0, int nc, int pcount, int iters, int blocks, unsigned long long* d_out);

inline const EnvOps* env_ops(int env_id) {
#define MRP_ENV_OPS_ENTRY(id, ...) &MRP_ENV_OPS_NAME(id),
    static const EnvOps* const t[N_ENVS] = {MRP_ENV_LIST(MRP_ENV_OPS_ENTRY)};
#undef MRP_ENV_OPS_ENTRY
    return env_id >= 0 && env_id < N_ENVS ? t[env_id] : nullptr;
}

}  // namespace mrp
