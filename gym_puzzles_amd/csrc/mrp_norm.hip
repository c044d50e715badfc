// mrp_norm.hip -- on-device VecNormalize + Monitor statistics for a batch of lanes (SURVEY.md
// 8f-2).  The reference trains with stable-baselines3's Monitor(env) per env and
// VecNormalize(DummyVecEnv(...)) with default arguments (train/train.py:68,80-82; reloaded by
// train/test.py:66); this is the same arithmetic on the step outputs while they are still in
// HBM, so a policy on the GPU never sees host copies.
//
// Semantics (stable-baselines3 1.x VecNormalize / RunningMeanStd / Monitor, restated):
//   reset : obs_rms.update(obs) (training), obs' = clip((obs - mean) / sqrt(var + eps), +-clip_obs)
//   step  : obs_rms.update(obs); obs' as above; returns = returns * gamma + reward;
//           ret_rms.update(returns); reward' = clip(reward / sqrt(ret_var + eps), +-clip_reward);
//           terminal_obs' normalised with the updated obs_rms; returns[done] = 0.
//   RunningMeanStd.update(x[L][D]) (Chan et al. parallel moments): batch mean/var over the L
//   lanes, delta = bm - mean, tot = count + L, mean += delta * L / tot,
//   var = (var * count + bv * L + delta^2 * count * L / tot) / tot, count = tot.
//   Monitor: per lane ep_return += reward (float64, in step order), ep_len += 1; on done both
//   are reported and restarted.
// The batch moments are float64 (two passes over the lanes); numpy's float32 np.mean/np.var
// of a float32 batch round differently, so the statistics are held to a bound derived from the
// inputs around the exact moments and the outputs to half a float32 ulp plus what that bound
// propagates (tests/vecnorm_exact.py, tests/test_norm_gpu.py), not bitwise.  Counts and Monitor
// sums are bit-exact; a NaN input gives NaN where numpy's rule does.
//
// Kernels: k_moments (one block per statistic column: the D obs columns, plus one block that
// advances the per-lane discounted returns and takes their moments) and k_apply (one thread per
// obs element for the normalised obs / terminal obs; per lane: reward, returns reset, Monitor).
// Both are tiny next to k_step; the statistics stay on the device between steps.
// Data-parallel (one set of statistics over the lanes of all ranks, DESIGN.md "Data-parallel
// VecNormalize"): k_moments<true> writes the rank's column moments into its part, the caller
// all-gathers the parts in rank order, and k_norm_merge folds them in that order before k_apply.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>

#include "../../include/mrp.h"
#include "mrp_host.h"

using namespace mrp_host;

namespace {

constexpr int NT = 256;

__device__ __forceinline__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}

// np.clip(x, -c, c): +-inf saturate and NaN stays NaN (fmin / fmax would return the bound for a NaN)
__device__ __forceinline__ double clip_np(double x, double c) { return x < -c ? -c : (x > c ? c : x); }

// Chan et al. merge of the batch moments (mean, var over n) into the running (mean, var, count)
__device__ __forceinline__ void rms_merge(double* mean, double* var, double* count, double bm, double bv, double n) {
    double delta = bm - *mean;
    double tot = *count + n;
    double new_mean = *mean + delta * n / tot;
    double m_a = *var * *count;
    double m_b = bv * n;
    double m2 = m_a + m_b + delta * delta * *count * n / tot;
    *mean = new_mean;
    *var = m2 / tot;
    *count = tot;
}

// blocks 0..D-1: obs column moments (if update_obs); block D: returns update + moments (if step).
// LOCAL (data-parallel, vec_env.py moments_local_ref): thread 0 writes this rank's part of the column,
// part[2c] = bm and part[2c + 1] = M2 = sum((x - bm)^2), and merges nothing; k_norm_merge folds the
// ranks' parts.  Otherwise thread 0 merges bv = M2 / n into the running statistics.  The sums are the
// same instructions in both, so the unsharded statistics keep their bits.
template <bool LOCAL>
__global__ __launch_bounds__(NT) void k_moments(const float* __restrict__ obs, int L, int D, const float* __restrict__ reward,
                                                double* __restrict__ returns, double gamma, double* obs_mean, double* obs_var,
                                                double* obs_count, double* ret_stats, int update_obs, int step,
                                                double* __restrict__ part) {
    __shared__ double red[NT];
    const int col = blockIdx.x, t = threadIdx.x;
    const double n = (double)L;
    if (col < D) {
        if (!update_obs) return;
        double s = 0.0;
        for (int l = t; l < L; l += NT) s += (double)obs[(size_t)l * D + col];
        const double bm = block_sum(s, red) / n;
        double q = 0.0;
        for (int l = t; l < L; l += NT) { double d = (double)obs[(size_t)l * D + col] - bm; q += d * d; }
        const double m2 = block_sum(q, red);
        if (t != 0) return;
        if (LOCAL) {
            part[2 * col] = bm; part[2 * col + 1] = m2;
        } else {
            double c = *obs_count;   // every column block reads the pre-update count
            double m = obs_mean[col], v = obs_var[col];
            rms_merge(&m, &v, &c, bm, m2 / n, n);
            obs_mean[col] = m; obs_var[col] = v;
        }
    } else {
        if (!step) return;
        double s = 0.0;
        for (int l = t; l < L; l += NT) {
            double r = returns[l] * gamma + (double)reward[l];
            returns[l] = r;
            s += r;
        }
        const double bm = block_sum(s, red) / n;
        double q = 0.0;
        for (int l = t; l < L; l += NT) { double d = returns[l] - bm; q += d * d; }
        const double m2 = block_sum(q, red);
        if (t != 0) return;
        if (LOCAL) {
            part[2 * D] = bm; part[2 * D + 1] = m2;
        } else {
            rms_merge(&ret_stats[0], &ret_stats[1], &ret_stats[2], bm, m2 / n, n);
        }
    }
}

// Data-parallel statistics (vec_env.py moments_combine_ref): one thread per statistic column folds the
// R rows of the gathered parts [R][stride] in ascending rank order, every rank with L lanes, and merges
// the result into the running statistics.  Every rank runs this on the same rows and the same
// statistics, so the replicas' statistics stay bit-identical.  Plain loads and stores, no atomics; the
// obs columns all read the pre-update count, which k_apply advances by R * L.
__global__ __launch_bounds__(NT) void k_norm_merge(const double* __restrict__ parts, int R, size_t stride, int L, int D,
                                                   double* __restrict__ obs_mean, double* __restrict__ obs_var,
                                                   const double* __restrict__ obs_count, double* __restrict__ ret_stats,
                                                   int update_obs, int step) {
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c > D || !(c < D ? update_obs : step)) return;
    const double nb = (double)L;
    double ma = parts[2 * c], Ma = parts[2 * c + 1], na = nb;
    for (int r = 1; r < R; ++r) {
        const double mb = parts[(size_t)r * stride + 2 * c], Mb = parts[(size_t)r * stride + 2 * c + 1];
        const double nt = na + nb, d = mb - ma;
        Ma = Ma + Mb + d * d * na * nb / nt;
        ma = ma + d * nb / nt;
        na = nt;
    }
    const double bv = Ma / na;
    if (c < D) {
        double cnt = *obs_count, m = obs_mean[c], v = obs_var[c];
        rms_merge(&m, &v, &cnt, ma, bv, na);
        obs_mean[c] = m; obs_var[c] = v;
    } else {
        rms_merge(&ret_stats[0], &ret_stats[1], &ret_stats[2], ma, bv, na);
    }
}

// one thread per obs element (coalesced rows) for obs / terminal obs; threads e < L also do lane
// e's reward, discounted-return reset and Monitor accumulators; thread 0 advances the obs count by
// count_add, the lanes of all ranks (k_moments / k_norm_merge read the pre-update count)
__global__ __launch_bounds__(NT) void k_apply(const float* __restrict__ obs, const float* __restrict__ term, int L, int D,
                                              const double* __restrict__ obs_mean, const double* __restrict__ obs_var,
                                              double* __restrict__ obs_count, int count_obs, double count_add,
                                              const double* __restrict__ ret_stats, double clip_obs, double clip_rew, double eps,
                                              const float* __restrict__ reward, const double* __restrict__ reward64,
                                              const uint8_t* __restrict__ done, double* __restrict__ returns, float* __restrict__ obs_out, float* __restrict__ term_out,
                                              float* __restrict__ reward_out, double* __restrict__ ep_ret, int* __restrict__ ep_len,
                                              double* __restrict__ ep_ret_out, int* __restrict__ ep_len_out, int step) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e == 0 && count_obs) *obs_count += count_add;
    if (e < L * D) {
        const int l = e / D, j = e - l * D;
        const double sd = sqrt(obs_var[j] + eps);
        double x = ((double)obs[e] - obs_mean[j]) / sd;
        obs_out[e] = (float)clip_np(x, clip_obs);
        if (step && done && done[l] && term && term_out) {
            double y = ((double)term[e] - obs_mean[j]) / sd;
            term_out[e] = (float)clip_np(y, clip_obs);
        }
    }
    if (e >= L) return;
    const int l = e;
    if (!step) { returns[l] = 0.0; ep_ret[l] = 0.0; ep_len[l] = 0; return; }
    const bool fin = done && done[l];
    const double r = (double)reward[l];
    if (reward_out) {
        double x = r / sqrt(ret_stats[1] + eps);
        reward_out[l] = (float)clip_np(x, clip_rew);
    }
    // Monitor sums the env's own (float64) rewards when the step exported them
    double er = ep_ret[l] + (reward64 ? reward64[l] : r);
    int el = ep_len[l] + 1;
    if (fin) {
        returns[l] = 0.0;
        if (ep_ret_out) ep_ret_out[l] = er;
        if (ep_len_out) ep_len_out[l] = el;
        er = 0.0; el = 0;
    }
    ep_ret[l] = er; ep_len[l] = el;
}

// ---- k_gae: SB3 RolloutBuffer.compute_returns_and_advantage + the TimeLimit bootstrap --------------
// The rule is gym_puzzles_amd/rollout.py's gae_ref (DESIGN.md "Rollout buffer"), numpy's dtype
// promotion included: the recurrence's accumulator L is float64, each row's delta is float32 except
// on the last row, and every product and sum rounds on its own (-ffp-contract=off).
//
// One thread per lane walks the rows from T-1 down to 0; a wave reads 64 consecutive elements of a
// row.  The recurrence cannot be re-associated (the result is pinned bit for bit), but only L is
// carried: the loads depend on nothing, so the rows are taken GAE_ROWS at a time and the loads of
// the block below are issued before the chain of the block in hand runs.  Row s needs v[s+1] and
// episode_starts[s+1], which the row above it already loaded, so each element is read once.
constexpr int GAE_NT = 64;    // one wave per workgroup: 4096 lanes spread over 64 CUs
constexpr int GAE_ROWS = 8;

struct GaeRow { float r, v, tv; uint8_t es, tr; };

template <bool BOOT>
__device__ __forceinline__ GaeRow gae_load(size_t i, const float* __restrict__ rew, const float* __restrict__ val,
                                           const uint8_t* __restrict__ es, const uint8_t* __restrict__ trunc,
                                           const float* __restrict__ tval) {
    GaeRow x;
    x.r = rew[i]; x.v = val[i]; x.es = es[i];
    x.tr = BOOT ? trunc[i] : (uint8_t)0;
    x.tv = BOOT ? tval[i] : 0.0f;
    return x;
}

// collect_rollouts: rewards[idx] += gamma * terminal_value, float32 throughout
template <bool BOOT>
__device__ __forceinline__ float gae_reward(const GaeRow& x, float g32) {
    if (BOOT && x.tr) return x.r + g32 * x.tv;
    return x.r;
}

// a row below the last: float32 delta, float64 accumulator; then this row becomes the "next" one
template <bool BOOT>
__device__ __forceinline__ void gae_row(const GaeRow& x, size_t i, float g32, float c32, double& L, float& nv, float& nnt,
                                        float* __restrict__ adv, float* __restrict__ ret) {
    const float delta = (gae_reward<BOOT>(x, g32) + (g32 * nv) * nnt) - x.v;
    L = (double)delta + (double)(c32 * nnt) * L;
    const float a = (float)L;
    adv[i] = a;
    ret[i] = a + x.v;
    nv = x.v;
    nnt = 1.0f - (x.es ? 1.0f : 0.0f);
}

template <bool BOOT>
__global__ __launch_bounds__(GAE_NT) void k_gae(int T, int N, const float* __restrict__ rew, const float* __restrict__ val,
                                                const uint8_t* __restrict__ es, const uint8_t* __restrict__ trunc,
                                                const float* __restrict__ tval, const float* __restrict__ last_val,
                                                const uint8_t* __restrict__ last_done, float g32, float c32,
                                                float* __restrict__ adv, float* __restrict__ ret) {
    const int lane = blockIdx.x * GAE_NT + threadIdx.x;
    if (lane >= N) return;
    const size_t n = (size_t)N;
    const size_t top = (size_t)(T - 1) * n + (size_t)lane;
    // last row: 1.0 - dones is float64 in numpy, so gamma * last_values rounds to float32 and the
    // rest of this delta is float64; `+ 0.0` is the recurrence's term of the zero initial L
    float nv, nnt;
    double L;
    {
        const GaeRow x = gae_load<BOOT>(top, rew, val, es, trunc, tval);
        const double nnt64 = 1.0 - (last_done[lane] ? 1.0 : 0.0);
        const float gnv = g32 * last_val[lane];
        L = (((double)gae_reward<BOOT>(x, g32) + (double)gnv * nnt64) - (double)x.v) + 0.0;
        const float a = (float)L;
        adv[top] = a;
        ret[top] = a + x.v;
        nv = x.v;
        nnt = 1.0f - (x.es ? 1.0f : 0.0f);
    }
    // rows s, s-1, ..., s-GAE_ROWS+1 per block: element j of a block is row s-j
    int s = T - 2;
    size_t i = top - n;   // index of row s (unused when s < 0)
    if (s >= GAE_ROWS - 1) {
        GaeRow cur[GAE_ROWS], nxt[GAE_ROWS];
#pragma unroll
        for (int j = 0; j < GAE_ROWS; ++j) cur[j] = gae_load<BOOT>(i - (size_t)j * n, rew, val, es, trunc, tval);
        while (s - GAE_ROWS >= GAE_ROWS - 1) {
            const size_t i2 = i - (size_t)GAE_ROWS * n;
#pragma unroll
            for (int j = 0; j < GAE_ROWS; ++j) nxt[j] = gae_load<BOOT>(i2 - (size_t)j * n, rew, val, es, trunc, tval);
#pragma unroll
            for (int j = 0; j < GAE_ROWS; ++j) gae_row<BOOT>(cur[j], i - (size_t)j * n, g32, c32, L, nv, nnt, adv, ret);
#pragma unroll
            for (int j = 0; j < GAE_ROWS; ++j) cur[j] = nxt[j];
            s -= GAE_ROWS;
            i = i2;
        }
#pragma unroll
        for (int j = 0; j < GAE_ROWS; ++j) gae_row<BOOT>(cur[j], i - (size_t)j * n, g32, c32, L, nv, nnt, adv, ret);
        s -= GAE_ROWS;
        i -= (size_t)GAE_ROWS * n;   // wraps when s is now -1; not used then
    }
    for (; s >= 0; --s, i -= n) gae_row<BOOT>(gae_load<BOOT>(i, rew, val, es, trunc, tval), i, g32, c32, L, nv, nnt, adv, ret);
}

thread_local std::string g_norm_create_error;

}  // namespace

struct mrp_norm {
    int n_lanes = 0, obs_dim = 0, device = 0, training = 1, norm_obs = 1;
    double clip_obs = 10.0, clip_rew = 10.0, gamma = 0.99, eps = 1e-8;
    hipStream_t stream = nullptr, own_stream = nullptr;
    double* d_stats = nullptr;   // [obs_mean D][obs_var D][obs_count][ret mean, var, count]
    double* d_returns = nullptr;
    double* d_ep_ret = nullptr;
    int* d_ep_len = nullptr;
    std::string err;
    double* obs_mean() { return d_stats; }
    double* obs_var() { return d_stats + obs_dim; }
    double* obs_count() { return d_stats + 2 * obs_dim; }
    double* ret_stats() { return d_stats + 2 * obs_dim + 1; }
    int n_stats() const { return 2 * obs_dim + 4; }
};

// MRP_E_ARG with a message that names the function; without an object it goes where
// mrp_norm_last_error(NULL) reads it
static int norm_bad(mrp_norm* n, const char* what) {
    (n ? n->err : g_norm_create_error) = what;
    return MRP_E_ARG;
}

extern "C" {

const char* mrp_norm_last_error(const mrp_norm* n) { return n ? n->err.c_str() : g_norm_create_error.c_str(); }

void mrp_norm_destroy(mrp_norm* n) {
    if (!n) return;
    (void)hipSetDevice(n->device);
    if (n->stream) (void)hipStreamSynchronize(n->stream);
    void* bufs[] = {n->d_stats, n->d_returns, n->d_ep_ret, n->d_ep_len};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    if (n->own_stream) (void)hipStreamDestroy(n->own_stream);
    delete n;
}

int mrp_norm_create(int n_lanes, int obs_dim, int device, double clip_obs, double clip_reward, double gamma, double epsilon,
                    mrp_norm** out) {
    g_norm_create_error.clear();
    if (!out || n_lanes <= 0 || obs_dim <= 0) return norm_bad(nullptr, "mrp_norm_create: null out, n_lanes < 1 or obs_dim < 1");
    *out = nullptr;
    if (const int rc = select_device(device, g_norm_create_error)) return rc;
    mrp_norm* n = new (std::nothrow) mrp_norm();
    if (!n) return norm_bad(nullptr, "mrp_norm_create: out of host memory");
    n->n_lanes = n_lanes; n->obs_dim = obs_dim; n->device = device;
    n->clip_obs = clip_obs; n->clip_rew = clip_reward; n->gamma = gamma; n->eps = epsilon;
    auto fail = [&](const char* what, hipError_t e) {
        g_norm_create_error = std::string(what) + ": " + hipGetErrorString(e);
        mrp_norm_destroy(n);
        return MRP_E_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&n->own_stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    n->stream = n->own_stream;
    size_t L = (size_t)n_lanes;
    if ((e = hipMalloc(&n->d_stats, n->n_stats() * sizeof(double))) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc(&n->d_returns, L * sizeof(double))) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc(&n->d_ep_ret, L * sizeof(double))) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc(&n->d_ep_len, L * sizeof(int))) != hipSuccess) return fail("hipMalloc", e);
    // RunningMeanStd(epsilon=1e-4): mean 0, var 1, count 1e-4 (obs and returns)
    double* h = new double[n->n_stats()];
    for (int j = 0; j < obs_dim; ++j) { h[j] = 0.0; h[obs_dim + j] = 1.0; }
    h[2 * obs_dim] = 1e-4;
    h[2 * obs_dim + 1] = 0.0; h[2 * obs_dim + 2] = 1.0; h[2 * obs_dim + 3] = 1e-4;
    e = hipMemcpy(n->d_stats, h, n->n_stats() * sizeof(double), hipMemcpyHostToDevice);
    delete[] h;
    if (e != hipSuccess) return fail("hipMemcpy", e);
    if ((e = hipMemset(n->d_returns, 0, L * sizeof(double))) != hipSuccess) return fail("hipMemset", e);
    if ((e = hipMemset(n->d_ep_ret, 0, L * sizeof(double))) != hipSuccess) return fail("hipMemset", e);
    if ((e = hipMemset(n->d_ep_len, 0, L * sizeof(int))) != hipSuccess) return fail("hipMemset", e);
    *out = n;
    return MRP_OK;
}

int mrp_norm_set_stream(mrp_norm* n, void* hip_stream) {
    if (!n) return norm_bad(n, "mrp_norm_set_stream: null handle");
    n->stream = (hipStream_t)hip_stream;   // NULL: the HIP null stream (torch's default stream)
    return MRP_OK;
}

int mrp_norm_set_training(mrp_norm* n, int training) {
    if (!n) return norm_bad(n, "mrp_norm_set_training: null handle");
    n->training = training ? 1 : 0;
    return MRP_OK;
}

int mrp_norm_set_norm_obs(mrp_norm* n, int norm_obs) {
    if (!n) return norm_bad(n, "mrp_norm_set_norm_obs: null handle");
    n->norm_obs = norm_obs ? 1 : 0;
    return MRP_OK;
}

// SB3 VecNormalize: obs statistics move when training and norm_obs, the returns' when training (and not in a reset)
struct Moves { int obs, ret; };
static Moves norm_moves(const mrp_norm* n, int step) { return Moves{n->training && n->norm_obs, step && n->training}; }

// k_apply over this rank's lanes; `lanes_all` is what the obs count advances by (the lanes of all ranks)
static int norm_apply_launch(mrp_norm* n, const float* obs, const float* reward, const double* reward64, const uint8_t* done,
                             const float* term, float* obs_out, float* reward_out, float* term_out, double* ep_ret_out,
                             int* ep_len_out, int step, int upd_obs, double lanes_all) {
    const int L = n->n_lanes, D = n->obs_dim;
    const int nthreads = L * D > L ? L * D : L;
    hipLaunchKernelGGL(k_apply, dim3((nthreads + NT - 1) / NT), dim3(NT), 0, n->stream, obs, term, L, D, n->obs_mean(),
                       n->obs_var(), n->obs_count(), upd_obs, lanes_all, n->ret_stats(), n->clip_obs, n->clip_rew, n->eps, reward,
                       reward64, done, n->d_returns, obs_out, term_out, reward_out, n->d_ep_ret, n->d_ep_len, ep_ret_out, ep_len_out,
                       step);
    MRP_HIPCHK(n, hipGetLastError());
    return MRP_OK;
}

static int norm_launch(mrp_norm* n, const float* obs, const float* reward, const double* reward64, const uint8_t* done,
                       const float* term, float* obs_out, float* reward_out, float* term_out, double* ep_ret_out, int* ep_len_out, int step) {
    MRP_HIPCHK(n, hipSetDevice(n->device));
    const int L = n->n_lanes, D = n->obs_dim;
    const Moves upd = norm_moves(n, step);
    if (upd.obs || upd.ret) {
        hipLaunchKernelGGL(k_moments<false>, dim3(D + 1), dim3(NT), 0, n->stream, obs, L, D, reward, n->d_returns, n->gamma,
                           n->obs_mean(), n->obs_var(), n->obs_count(), n->ret_stats(), upd.obs, upd.ret, nullptr);
        MRP_HIPCHK(n, hipGetLastError());
    }
    return norm_apply_launch(n, obs, reward, reward64, done, term, obs_out, reward_out, term_out, ep_ret_out, ep_len_out, step,
                             upd.obs, (double)L);
}

int mrp_norm_reset_device(mrp_norm* n, const float* d_obs, float* d_obs_out) {
    if (!n || !d_obs || !d_obs_out) return norm_bad(n, "mrp_norm_reset_device: null pointer");
    return norm_launch(n, d_obs, nullptr, nullptr, nullptr, nullptr, d_obs_out, nullptr, nullptr, nullptr, nullptr, 0);
}

int mrp_norm_step_device_ex(mrp_norm* n, const float* d_obs, const float* d_reward, const double* d_reward64, const uint8_t* d_done,
                            const float* d_term_obs, float* d_obs_out, float* d_reward_out, float* d_term_out, double* d_ep_return,
                            int32_t* d_ep_len) {
    if (!n || !d_obs || !d_reward || !d_done || !d_obs_out || !d_reward_out) return norm_bad(n, "mrp_norm_step_device: null pointer");
    return norm_launch(n, d_obs, d_reward, d_reward64, d_done, d_term_obs, d_obs_out, d_reward_out, d_term_out, d_ep_return,
                       d_ep_len, 1);
}

int mrp_norm_step_device(mrp_norm* n, const float* d_obs, const float* d_reward, const uint8_t* d_done, const float* d_term_obs,
                         float* d_obs_out, float* d_reward_out, float* d_term_out, double* d_ep_return, int32_t* d_ep_len) {
    return mrp_norm_step_device_ex(n, d_obs, d_reward, nullptr, d_done, d_term_obs, d_obs_out, d_reward_out, d_term_out,
                                   d_ep_return, d_ep_len);
}

// ---- data-parallel statistics: local phase, (the caller's all-gather), apply phase --------------------
int mrp_norm_part_len(int obs_dim) { return obs_dim < 1 ? MRP_E_ARG : 2 * (obs_dim + 1); }

int mrp_norm_local_device(mrp_norm* n, const float* d_obs, const float* d_reward, int step, double* d_part) {
    if (!n) return norm_bad(n, "mrp_norm_local_device: null handle");
    if (!d_obs || !d_part || (step && !d_reward)) return norm_bad(n, "mrp_norm_local_device: null pointer");
    const int L = n->n_lanes, D = n->obs_dim;
    const size_t f = sizeof(float);
    if (check_outputs({{d_obs, (size_t)L * D * f}, {step ? d_reward : nullptr, L * f}}, {{d_part, 2 * ((size_t)D + 1) * sizeof(double)}}))
        return norm_bad(n, "mrp_norm_local_device: d_part overlaps an input");
    const Moves upd = norm_moves(n, step);
    if (!upd.obs && !upd.ret) return MRP_OK;   // nothing moves: nothing to exchange
    MRP_HIPCHK(n, hipSetDevice(n->device));
    hipLaunchKernelGGL(k_moments<true>, dim3(D + 1), dim3(NT), 0, n->stream, d_obs, L, D, d_reward, n->d_returns, n->gamma,
                       n->obs_mean(), n->obs_var(), n->obs_count(), n->ret_stats(), upd.obs, upd.ret, d_part);
    MRP_HIPCHK(n, hipGetLastError());
    return MRP_OK;
}

int mrp_norm_apply_device(mrp_norm* n, int R, const double* d_parts, long long part_stride, int step, const float* d_obs,
                          const float* d_reward, const double* d_reward64, const uint8_t* d_done, const float* d_term_obs,
                          float* d_obs_out, float* d_reward_out, float* d_term_out, double* d_ep_return, int32_t* d_ep_len) {
    if (!n) return norm_bad(n, "mrp_norm_apply_device: null handle");
    if (R < 1) return norm_bad(n, "mrp_norm_apply_device: R < 1");
    if (!d_parts || !d_obs || !d_obs_out || (step && (!d_reward || !d_done || !d_reward_out)))
        return norm_bad(n, "mrp_norm_apply_device: null pointer");
    const int L = n->n_lanes, D = n->obs_dim;
    if (part_stride < 2 * ((long long)D + 1)) return norm_bad(n, "mrp_norm_apply_device: part_stride < mrp_norm_part_len(obs_dim)");
    const size_t f = sizeof(float), l = (size_t)L, ld = l * (size_t)D;
    const Span parts{d_parts, (size_t)R * (size_t)part_stride * sizeof(double)};
    for (const Span& out : {Span{d_obs_out, ld * f}, Span{d_reward_out, l * f}, Span{d_term_out, ld * f},
                            Span{d_ep_return, l * sizeof(double)}, Span{d_ep_len, l * sizeof(int32_t)}})
        if (check_outputs({parts}, {out})) return norm_bad(n, "mrp_norm_apply_device: d_parts overlaps an output");
    MRP_HIPCHK(n, hipSetDevice(n->device));
    const Moves upd = norm_moves(n, step);
    if (upd.obs || upd.ret) {
        hipLaunchKernelGGL(k_norm_merge, dim3((D + 1 + NT - 1) / NT), dim3(NT), 0, n->stream, d_parts, R, (size_t)part_stride, L, D,
                           n->obs_mean(), n->obs_var(), n->obs_count(), n->ret_stats(), upd.obs, upd.ret);
        MRP_HIPCHK(n, hipGetLastError());
    }
    // in a reset (step == 0) k_apply reads only the obs pointers
    return norm_apply_launch(n, d_obs, d_reward, d_reward64, d_done, d_term_obs, d_obs_out, d_reward_out, d_term_out, d_ep_return,
                             d_ep_len, step != 0, upd.obs, (double)R * (double)L);
}

int mrp_norm_get_stats(mrp_norm* n, double* out) {
    if (!n || !out) return norm_bad(n, "mrp_norm_get_stats: null pointer");
    MRP_HIPCHK(n, hipSetDevice(n->device));
    MRP_HIPCHK(n, hipMemcpyAsync(out, n->d_stats, n->n_stats() * sizeof(double), hipMemcpyDeviceToHost, n->stream));
    MRP_HIPCHK(n, hipStreamSynchronize(n->stream));
    return MRP_OK;
}

int mrp_norm_set_stats(mrp_norm* n, const double* in) {
    if (!n || !in) return norm_bad(n, "mrp_norm_set_stats: null pointer");
    MRP_HIPCHK(n, hipSetDevice(n->device));
    MRP_HIPCHK(n, hipMemcpyAsync(n->d_stats, in, n->n_stats() * sizeof(double), hipMemcpyHostToDevice, n->stream));
    MRP_HIPCHK(n, hipStreamSynchronize(n->stream));
    return MRP_OK;
}

int mrp_gae_device(int device, void* hip_stream, int n_steps, int n_lanes, const float* d_rewards, const float* d_values,
                   const uint8_t* d_episode_starts, const uint8_t* d_truncated, const float* d_terminal_values,
                   const float* d_last_values, const uint8_t* d_last_dones, double gamma, double gae_lambda,
                   float* d_advantages, float* d_returns) {
    std::string& err = g_norm_create_error;
    err.clear();
    auto bad = [&](const char* what) { err = std::string("mrp_gae_device: ") + what; return MRP_E_ARG; };
    // every check that needs no device comes before the first HIP call
    if (n_steps < 1) return bad("n_steps < 1");
    if (n_lanes < 1) return bad("n_lanes < 1");
    if (!d_rewards || !d_values || !d_episode_starts || !d_last_values || !d_last_dones || !d_advantages || !d_returns)
        return bad("null pointer");
    if ((d_truncated == nullptr) != (d_terminal_values == nullptr))
        return bad("d_truncated and d_terminal_values are given together or not at all");
    // extents in bytes: the flag arrays hold one byte per element
    const size_t n = (size_t)n_lanes, tn = (size_t)n_steps * n, f = sizeof(float);
    if (const char* what = check_outputs({{d_rewards, tn * f}, {d_values, tn * f}, {d_episode_starts, tn}, {d_truncated, tn},
                                          {d_terminal_values, tn * f}, {d_last_values, n * f}, {d_last_dones, n}},
                                         {{d_advantages, tn * f}, {d_returns, tn * f}}))
        return bad(what);
    if (const int rc = select_device(device, err)) {
        if (rc == MRP_E_ARG) err.insert(0, "mrp_gae_device: ");
        return rc;
    }
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) { err = std::string("hipSetDevice: ") + hipGetErrorString(e); return MRP_E_HIP; }
    const float g32 = (float)gamma, c32 = (float)(gamma * gae_lambda);
    const dim3 grid((unsigned)(((long long)n_lanes + GAE_NT - 1) / GAE_NT)), block(GAE_NT);
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_truncated)
        hipLaunchKernelGGL(k_gae<true>, grid, block, 0, st, n_steps, n_lanes, d_rewards, d_values, d_episode_starts, d_truncated,
                           d_terminal_values, d_last_values, d_last_dones, g32, c32, d_advantages, d_returns);
    else
        hipLaunchKernelGGL(k_gae<false>, grid, block, 0, st, n_steps, n_lanes, d_rewards, d_values, d_episode_starts, d_truncated,
                           d_terminal_values, d_last_values, d_last_dones, g32, c32, d_advantages, d_returns);
    if ((e = hipGetLastError()) != hipSuccess) { err = std::string("k_gae launch: ") + hipGetErrorString(e); return MRP_E_HIP; }
    return MRP_OK;
}

}  // extern "C"
