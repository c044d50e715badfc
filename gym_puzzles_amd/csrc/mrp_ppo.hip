// mrp_ppo.hip -- one optimiser step of SB3's PPO.train() on a minibatch, on the device: evaluate_actions,
// the clipped surrogate / value / entropy losses, the backward pass through the actor-critic network,
// global grad-norm clipping and Adam, written into the device policy's parameters in place (DESIGN.md
// "Device PPO update").  The rule, which the kernels match bit for bit, is gym_puzzles_amd/ppo.py's
// ppo_grad_ref / adam_ref.  Six launches on the caller's stream, no host synchronisation, no atomics:
// every reduction has a fixed order.
//
//   k_ppo_fb      a workgroup of 4 waves takes a tile of 32 samples forward (k_policy's hidden_layer
//                 and head, each layer's activation saved to the workspace), evaluates the loss terms
//                 and the upstream gradients, and goes backward: s = delta . W is the same MFMA loop
//                 with delta as the A operand in LDS and torch's row-major [out][in] image of the
//                 weights as B (a k-step's two B rows are contiguous), from +0; delta = s * act' is
//                 saved to the workspace.
//   k_ppo_wgrad   one wave per (32x32 tile of a weight matrix, chunk of 256 samples): A[i = j][k = n] is
//                 delta transposed, B[k = n][col = k] the saved input activation, the MFMA's k runs over
//                 the chunk's samples (an odd last sample is an explicit fmaf); writes chunk partials.
//   k_ppo_bsum    the bias and log_std chunk partials (plain adds in sample order) and the chunks'
//                 float64 sums of the five statistics' terms.
//   k_ppo_reduce  adds the chunk partials in ascending order into the flat gradient.
//   k_ppo_norm    one workgroup: the float64 sum of squares in 256 interleaved partials, the clip
//                 factor, and the five statistics.
//   k_ppo_adam    flat elementwise clip + Adam on the master vectors; writes both device images of the
//                 parameters (k_policy's [K][Npad] one and the row-major one) and std = exp_f32(log_std).
//
// mrp_ppo_minibatch_device puts up to three launches in front of these (ppo.py normalize_adv_ref):
//
//   k_ppo_gather   copies the minibatch's indexed rows of the rollout fields into the optimiser's staging
//                  buffers (a workgroup per 32 rows of a chunk, row reads coalesced); an index outside
//                  [0, n_rows) reads row 0 and sets the sticky bad_index word; with normalize_advantage the
//                  first workgroup of a chunk also writes the chunk's sequential float64 advantage sum.
//   k_ppo_advnorm  two launches of a workgroup per chunk: <0> the chunk's float64 sum of squared deviations
//                  from the mean, <1> the staged advantages normalised in place.  The chunk partials are
//                  added in ascending order by one thread of every workgroup.
//
// and runs the step under a predicate: the object's device words {stopped, applied, bad_index}.  Every
// kernel of such a call first loads `stopped` (wave-uniform, before any barrier) and returns when it is
// set; k_ppo_norm sets it when kl_stop_ref holds, k_ppo_adam advances `applied`.  mrp_ppo_grad_device and
// mrp_ppo_step_device pass a null predicate.
//
// mrp_ppo_apply_device is the data-parallel apply phase (ppo.py combine_ref): it starts from R ranks'
// gradients and statistics instead of a minibatch, under the same predicate, in three launches:
//
//   k_ppo_combine  elementwise over the n_params + 5 floats of a rank's part: the R rows added in ascending
//                  rank order (plain float32 adds), one multiply by float32(1 / R); writes the master
//                  gradient, the caller's statistics row and the word k_ppo_norm<true> reads approx_kl from.
//   k_ppo_norm<true>, k_ppo_adam   as above, on the combined values.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "../../include/mrp.h"
#include "mrp_host.h"
#include "mrp_math.h"
#include "mrp_policy_layout.h"
#include "mrp_policy_net.h"

using namespace mrp_pol;
using namespace mrp_host;

namespace {

constexpr int CHUNK = 256;                 // ppo.py CHUNK: samples per partial sum
constexpr int NL = 3 * P_MAXL;             // hidden layers at most (trunk, policy tower, value tower)
constexpr int L_ACT = NL, L_VAL = NL + 1;  // the heads' slots in the delta table
constexpr int HW = 32;                     // row stride of the heads' delta / log_std-term arrays
constexpr int NSTAT = 5, SW = 8;           // statistics, and the row stride of their per-sample terms
constexpr int S_KL = 3;                    // approx_kl's place among the statistics
constexpr int W_STOPPED = 0, W_APPLIED = 1, W_BAD_INDEX = 2, NWORDS = 4;   // the object's device progress words
constexpr int G_ROWS = 32;                 // rows of a chunk whose observation and action rows one workgroup gathers

struct PpoNet {
    Net net;
    Layer bwd[NL];         // per hidden layer: w = row-major [N][pad32(K)] image, K = outputs, N = inputs
    float* act[NL];        // saved activations [max_batch][Npad]
    float* delta[NL + 2];  // saved deltas [max_batch][Npad]; the heads' are [max_batch][HW]
    float* lsterm;         // [max_batch][HW]: the samples' log_std gradient terms
    float* sterm;          // [max_batch][SW]: the samples' statistics terms
};

struct WTile { const float* delta; const float* x; int dstride, xstride, j0, k0, N, K, off; };  // x == nullptr: the observations
struct BElem { const float* src; int stride, off; };

__device__ __forceinline__ float* buf(float* lds, int i) { return lds + i * (P_TILE * P_LDA); }

// forward through n layers from buffer `in` (as k_policy's tower), saving each activation
__device__ __forceinline__ int fwd_tower(const PpoNet& pn, const Layer* L, int li, int n, float* lds, int in, int a, int b,
                                         int base, int B) {
    for (int i = 0; i < n; ++i) {
        const int out = (i & 1) ? b : a;
        hidden_layer(L[i], buf(lds, in), buf(lds, out), pn.net.relu);
        __syncthreads();
        const int N = L[i].N, Npad = L[i].Npad;
        float* g = pn.act[li + i];
        for (int e = threadIdx.x; e < P_TILE * N; e += P_NT) {
            const int row = e / N, col = e - row * N;
            if (base + row < B) g[(size_t)(base + row) * Npad + col] = buf(lds, out)[row * P_LDA + col];
        }
        in = out;
    }
    return in;
}

// backward through n layers: buffer `cur` holds s at the tower's output; returns the buffer of s at its
// input (nothing is computed into the observations: `to_obs` marks a tower whose first layer reads them)
__device__ __forceinline__ int bwd_tower(const PpoNet& pn, const Layer* L, int li, int n, float* lds, int cur, int other,
                                         int to_obs, int base, int B) {
    const int relu = pn.net.relu;
    for (int i = n - 1; i >= 0; --i) {
        const int N = L[i].N, Npad = L[i].Npad;
        const float* t = pn.act[li + i];
        float* d = pn.delta[li + i];
        float* s = buf(lds, cur);
        for (int e = threadIdx.x; e < P_TILE * N; e += P_NT) {
            const int row = e / N, col = e - row * N;
            const bool live = base + row < B;
            const size_t g = (size_t)(base + row) * Npad + col;
            const float tv = live ? t[g] : 0.0f;
            const float dp = relu ? (tv > 0.0f ? 1.0f : 0.0f) : __builtin_fmaf(-tv, tv, 1.0f);
            const float dl = s[row * P_LDA + col] * dp;
            s[row * P_LDA + col] = dl;
            if (live) d[g] = dl;
        }
        __syncthreads();
        if (i == 0 && to_obs) break;
        hidden_layer<true>(pn.bwd[li + i], s, buf(lds, other), relu);
        __syncthreads();
        const int tmp = cur; cur = other; other = tmp;
    }
    return cur;
}

__global__ __launch_bounds__(P_NT) void k_ppo_fb(const PpoNet pn, int B, const float* __restrict__ obs,
                                                 const float* __restrict__ actions, const float* __restrict__ old_lp,
                                                 const float* __restrict__ adv_in, const float* __restrict__ ret_in, float clip,
                                                 float vf2, float invB, const float* __restrict__ old_v, float cv,
                                                 const int* pred) {
    if (pred && *pred) return;
    __shared__ float lds[3 * P_TILE * P_LDA];
    __shared__ float hs[P_TILE * P_HS];     // the heads' outputs, then the log-prob terms, then the heads' deltas
    __shared__ float gs[P_TILE];
    const Net& net = pn.net;
    const int tid = threadIdx.x, base = blockIdx.x * P_TILE;
    const int D = net.obs_dim, A = net.act_dim, relu = net.relu;
    const int S = net.n_shared, NP = net.n_pi, NV = net.n_vf;
    for (int e = tid; e < P_TILE * D; e += P_NT) {
        const int row = e / D, k = e - row * D;
        lds[row * P_LDA + k] = base + row < B ? obs[(size_t)(base + row) * D + k] : 0.0f;
    }
    __syncthreads();
    // ---- forward, as k_policy
    const int T = fwd_tower(pn, net.shared, 0, S, lds, 0, 1, 0, base, B);
    const int po = fwd_tower(pn, net.pi, S, NP, lds, T, 1 - T, 2, base, B);
    head(net.act, A, buf(lds, po), hs, 0);
    __syncthreads();
    const int vo = fwd_tower(pn, net.vf, S + NP, NV, lds, T, 1 - T, 2, base, B);
    head(net.val, 1, buf(lds, vo), hs, P_MAXA);
    __syncthreads();
    // ---- evaluate: d, the log-prob terms
    const int row = tid & 31, n = base + row;
    const bool live = n < B;
    constexpr int NS = (P_MAXA + 7) / 8;
    float term[NS], dd[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int i = (tid >> 5) + 8 * s;
        term[s] = 0.0f; dd[s] = 0.0f;
        if (i < A && live) {
            const float m = hs[row * P_HS + i], sd = net.std[i];
            const float d = actions[(size_t)n * A + i] - m;
            dd[s] = d;
            const float q = (-(d * d)) / (2.0f * (sd * sd));
            term[s] = (q - net.log_std[i]) - 0x1.d67f1cp-1f;   // float32(log(sqrt(2 pi)))
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int i = (tid >> 5) + 8 * s;
        if (i < A) hs[row * P_HS + i] = term[s];
    }
    __syncthreads();
    // ---- the loss terms and the upstream gradients of a sample
    if (tid < P_TILE) {
        float g = 0.0f, dv = 0.0f;
        if (live) {
            float lp = 0.0f;
            for (int i = 0; i < A; ++i) lp = lp + hs[row * P_HS + i];
            float ent = 0.0f;
            for (int i = 0; i < A; ++i) ent = ent + ((0.5f + 0x1.d67f1cp-1f) + net.log_std[i]);
            const float v = hs[row * P_HS + P_MAXA], adv = adv_in[n], ret = ret_in[n];
            const float diff = lp - old_lp[n];
            const float ratio = mrp::exp_f32(diff);
            const float lo = 1.0f - clip, hi = 1.0f + clip;
            const float pl1 = adv * ratio, pl2 = adv * mrp::fmin_(mrp::fmax_(ratio, lo), hi);
            const bool first = pl1 <= pl2;
            g = first ? (-(adv * ratio)) * invB : 0.0f;
            // clip_range_vf (old_v non-null): the value prediction is clamped to old_v +- cv, and the gradient
            // passes where the clamp does (torch's clamp backward: inclusive at both ends)
            float vp = v;
            bool pass = true;
            if (old_v) {
                const float ov = old_v[n], dvo = v - ov;
                vp = ov + mrp::fmin_(mrp::fmax_(dvo, -cv), cv);
                pass = dvo >= -cv && dvo <= cv;
            }
            dv = pass ? ((vp - ret) * vf2) * invB : 0.0f;
            const float r1 = ratio - 1.0f;
            float* st = pn.sterm + (size_t)n * SW;
            st[0] = -(first ? pl1 : pl2);
            st[1] = (ret - vp) * (ret - vp);
            st[2] = -ent;
            st[3] = r1 - diff;
            st[4] = __builtin_fabsf(r1) > clip ? 1.0f : 0.0f;
            pn.delta[L_VAL][(size_t)n * HW] = dv;
        }
        gs[row] = g;
        hs[row * P_HS + P_MAXA] = dv;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int i = (tid >> 5) + 8 * s;
        if (i < A) {
            const float sd = net.std[i], var = sd * sd, g = gs[row], d = dd[s];
            const float dm = g * (d / var);
            hs[row * P_HS + i] = dm;
            if (live) {
                pn.delta[L_ACT][(size_t)n * HW + i] = dm;
                pn.lsterm[(size_t)n * HW + i] = g * ((d * d) / var - 1.0f);
            }
        }
    }
    __syncthreads();
    // ---- backward.  Every activation is in the workspace, so the three LDS buffers are free.
    // policy tower: s at the action head's input, a chain over the head's outputs from +0
    {
        const int K = net.act.K;
        float* s = buf(lds, 0);
        for (int e = tid; e < P_TILE * K; e += P_NT) {
            const int k = e >> 5;
            float acc = 0.0f;
            for (int i = 0; i < A; ++i) acc = __builtin_fmaf(hs[row * P_HS + i], net.act.w[(size_t)i * net.act.Kpad + k], acc);
            s[row * P_LDA + k] = acc;
        }
    }
    __syncthreads();
    const int rp = bwd_tower(pn, net.pi, S, NP, lds, 0, 1, S == 0, base, B);
    // value tower in the two buffers that do not hold the policy tower's s
    const int x = rp == 0 ? 1 : 0, y = 3 - rp - x;
    {
        const int K = net.val.K;
        float* s = buf(lds, x);
        const float dv = hs[row * P_HS + P_MAXA];
        for (int e = tid; e < P_TILE * K; e += P_NT) {
            const int k = e >> 5;
            s[row * P_LDA + k] = dv * net.val.w[k];
        }
    }
    __syncthreads();
    const int rv = bwd_tower(pn, net.vf, S + NP, NV, lds, x, y, S == 0, base, B);
    if (S > 0) {
        const int K = net.shared[S - 1].N;
        float* sv = buf(lds, rv);
        const float* sp = buf(lds, rp);
        for (int e = tid; e < P_TILE * K; e += P_NT) {
            const int k = e >> 5;
            sv[row * P_LDA + k] = sp[row * P_LDA + k] + sv[row * P_LDA + k];
        }
        __syncthreads();
        (void)bwd_tower(pn, net.shared, 0, S, lds, rv, rp, 1, base, B);
    }
}

// one wave per (tile, chunk): partial[chunk][off + j * K + k] = fmaf chain over the chunk's samples n of
// fma(delta[n][j], x[n][k], acc) from +0
__global__ __launch_bounds__(P_NT) void k_ppo_wgrad(const WTile* __restrict__ tiles, int n_tiles, int B,
                                                    const float* __restrict__ obs, int obs_dim, float* __restrict__ partial,
                                                    int n_params, const int* pred) {
    if (pred && *pred) return;
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 31, h = l >> 5;
    const int n_chunks = (B + CHUNK - 1) / CHUNK;
    const int gid = blockIdx.x * (P_NT / 64) + wave;
    if (gid >= n_tiles * n_chunks) return;
    const int chunk = gid / n_tiles;
    const WTile t = tiles[gid - chunk * n_tiles];
    const float* xs = t.x ? t.x : obs;
    const int xstride = t.x ? t.xstride : obs_dim;
    const int n0 = chunk * CHUNK, cnt = (B - n0 < CHUNK ? B - n0 : CHUNK), cnt2 = cnt & ~1;
    const int j = t.j0 + c, k = t.k0 + c;
    const bool jok = j < t.N, kok = k < t.K;
    // A[i = l & 31][k = l >> 5] = delta[n + h][j0 + c];  B[k = l >> 5][col = l & 31] = x[n + h][k0 + c]
    const float* ap = t.delta + (size_t)(n0 + h) * t.dstride + (jok ? j : 0);
    const float* bp = xs + (size_t)(n0 + h) * xstride + (kok ? k : 0);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    int s = 0;
    for (; s + 2 * P_U <= cnt2; s += 2 * P_U) {
        float a[P_U], b[P_U];
#pragma unroll
        for (int u = 0; u < P_U; ++u) {
            a[u] = ap[(size_t)(s + 2 * u) * t.dstride];
            b[u] = bp[(size_t)(s + 2 * u) * xstride];
        }
#pragma unroll
        for (int u = 0; u < P_U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(jok ? a[u] : 0.0f, kok ? b[u] : 0.0f, acc, 0, 0, 0);
    }
    for (; s < cnt2; s += 2) {
        const float a = ap[(size_t)s * t.dstride], b = bp[(size_t)s * xstride];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(jok ? a : 0.0f, kok ? b : 0.0f, acc, 0, 0, 0);
    }
    // C/D: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    if (cnt & 1) {   // an odd last sample: a zero pad k-step would turn an accumulator of -0 into +0
        const int nl = n0 + cnt2;
        const float xv = kok ? xs[(size_t)nl * xstride + k] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jr = t.j0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float dv = jr < t.N ? t.delta[(size_t)nl * t.dstride + jr] : 0.0f;
            acc[r] = __builtin_fmaf(dv, xv, acc[r]);
        }
    }
    if (kok) {
        float* out = partial + (size_t)chunk * n_params + t.off;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jr = t.j0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (jr < t.N) out[(size_t)jr * t.K + k] = acc[r];
        }
    }
}

// grid (chunks, blocks over the bias elements + 1): plain adds in sample order from +0; the last block row
// sums the chunk's statistics terms in float64
__global__ __launch_bounds__(P_NT) void k_ppo_bsum(const BElem* __restrict__ elems, int n_elems, int B,
                                                   const float* __restrict__ sterm, float* __restrict__ partial, int n_params,
                                                   double* __restrict__ spart, const int* pred) {
    if (pred && *pred) return;
    const int chunk = blockIdx.x, n0 = chunk * CHUNK, n1 = (B < n0 + CHUNK ? B : n0 + CHUNK);
    if (blockIdx.y == gridDim.y - 1) {
        if (threadIdx.x < NSTAT) {
            double acc = 0.0;
            for (int n = n0; n < n1; ++n) acc = acc + (double)sterm[(size_t)n * SW + threadIdx.x];
            spart[chunk * NSTAT + threadIdx.x] = acc;
        }
        return;
    }
    const int e = blockIdx.y * P_NT + threadIdx.x;
    if (e >= n_elems) return;
    const BElem el = elems[e];
    float acc = 0.0f;
    for (int n = n0; n < n1; ++n) acc = acc + el.src[(size_t)n * el.stride];
    partial[(size_t)chunk * n_params + el.off] = acc;
}

__global__ __launch_bounds__(P_NT) void k_ppo_reduce(const float* __restrict__ partial, int n_params, int n_chunks, int act_dim,
                                                     float ent_coef, float* __restrict__ grad, const int* pred) {
    if (pred && *pred) return;
    const int e = blockIdx.x * P_NT + threadIdx.x;
    if (e >= n_params) return;
    float g = partial[e];
    for (int c = 1; c < n_chunks; ++c) g = g + partial[(size_t)c * n_params + e];
    if (e < act_dim) g = g + (-ent_coef);
    grad[e] = g;
}

// COMBINED (mrp_ppo_apply_device): the statistics are k_ppo_combine's, and kl_stop_ref reads the combined
// approx_kl from coef[1]; spart, n_chunks, B and stats are not used
template <bool COMBINED>
__global__ __launch_bounds__(P_NT) void k_ppo_norm(const float* __restrict__ grad, int n_params, double max_norm,
                                                   const double* __restrict__ spart, int n_chunks, int B,
                                                   float* __restrict__ coef, float* __restrict__ stats, int* words,
                                                   double kl_limit) {
    if (words && words[W_STOPPED]) return;
    __shared__ double part[P_NT];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int e = t; e < n_params; e += P_NT) {
        const double g = (double)grad[e];
        acc = acc + g * g;
    }
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int i = 0; i < P_NT; ++i) sum = sum + part[i];
        const double q = max_norm / (sqrt(sum) + 1e-6);
        coef[0] = (float)(q < 1.0 ? q : 1.0);
    } else if (COMBINED) {
        if (t == 1 && words && kl_limit >= 0.0 && (double)coef[1] > kl_limit) words[W_STOPPED] = 1;
    } else if (t <= NSTAT) {
        double sum = 0.0;
        for (int c = 0; c < n_chunks; ++c) sum = sum + spart[c * NSTAT + (t - 1)];
        const float sv = (float)(sum * (1.0 / (double)B));
        stats[t - 1] = sv;
        // kl_stop_ref: this minibatch is not applied and nothing after it runs (kl_limit = 1.5 * target_kl, < 0: none)
        if (t - 1 == S_KL && words && kl_limit >= 0.0 && (double)sv > kl_limit) words[W_STOPPED] = 1;
    }
}

// combine_ref: element e of the R rows of `parts` (row stride `stride` floats) added in ascending row order,
// then times inv_r = float32(1 / R).  Elements [0, n_params) are the gradient, [n_params, n_params + NSTAT) the
// statistics: those go to `stats`, and approx_kl also to `kl` for k_ppo_norm<true>.
__global__ __launch_bounds__(P_NT) void k_ppo_combine(const float* __restrict__ parts, int R, size_t stride, int n_params,
                                                      float inv_r, float* __restrict__ grad, float* __restrict__ stats,
                                                      float* __restrict__ kl, const int* words) {
    if (words[W_STOPPED]) return;
    const int e = blockIdx.x * P_NT + threadIdx.x;
    if (e >= n_params + NSTAT) return;
    float g = parts[e];
    for (int r = 1; r < R; ++r) g = g + parts[(size_t)r * stride + e];
    g = g * inv_r;
    if (e < n_params) {
        grad[e] = g;
    } else {
        stats[e - n_params] = g;
        if (e - n_params == S_KL) kl[0] = g;
    }
}

struct AdamK { float b1, omb1, b2, omb2, sqrt_bc2, step, eps; };

// the two device images of a parameter: `fwd` indexes the policy's image (k_policy's layout), `row` the
// row-major image of the hidden weights (-1: none)
__global__ __launch_bounds__(P_NT) void k_ppo_adam(int n_params, int act_dim, const float* __restrict__ grad,
                                                   const float* __restrict__ coef, float* __restrict__ param,
                                                   float* __restrict__ m, float* __restrict__ v, const int* __restrict__ fwd,
                                                   const int* __restrict__ row, float* __restrict__ image,
                                                   float* __restrict__ rows, float* __restrict__ std, AdamK k, int* words) {
    if (words && words[W_STOPPED]) return;
    const int e = blockIdx.x * P_NT + threadIdx.x;
    if (e == 0 && words) words[W_APPLIED] = words[W_APPLIED] + 1;
    if (e >= n_params) return;
    const float g = grad[e] * coef[0];
    const float mn = (k.b1 * m[e]) + (k.omb1 * g);
    const float vn = (k.b2 * v[e]) + ((k.omb2 * g) * g);
    const float denom = (sqrtf(vn) / k.sqrt_bc2) + k.eps;
    const float p = param[e] - k.step * (mn / denom);
    m[e] = mn; v[e] = vn; param[e] = p;
    image[fwd[e]] = p;
    if (row[e] >= 0) rows[row[e]] = p;
    if (e < act_dim) std[e] = mrp::exp_f32(p);
}

// the master copy and the row-major image from the policy's image (after mrp_policy_set_params)
__global__ __launch_bounds__(P_NT) void k_ppo_import(int n_params, const float* __restrict__ image, const int* __restrict__ fwd,
                                                     const int* __restrict__ row, float* __restrict__ param,
                                                     float* __restrict__ rows) {
    const int e = blockIdx.x * P_NT + threadIdx.x;
    if (e >= n_params) return;
    const float p = image[fwd[e]];
    param[e] = p;
    if (row[e] >= 0) rows[row[e]] = p;
}

// the six rollout fields of a minibatch call: what the caller holds, and the optimiser's staging buffers
struct Fields { const float *obs, *act, *old_v, *old_lp, *adv, *ret; };
struct Stage { float *obs, *act, *old_v, *old_lp, *adv, *ret; };

// grid (chunks, row groups of a chunk): staged row n = field row idx[n] (n itself without an index); row
// group 0 also sums the chunk's advantages in sample order in float64 (sum_adv)
__global__ __launch_bounds__(P_NT) void k_ppo_gather(const int* pred, int* words, int B, const long long* __restrict__ idx,
                                                     long long n_rows, Fields f, Stage s, int D, int A, int sum_adv,
                                                     double* __restrict__ advpart) {
    if (*pred) return;
    __shared__ long long rows[G_ROWS];
    __shared__ float adv_s[CHUNK];
    const int tid = threadIdx.x, n0 = blockIdx.x * CHUNK, r0 = n0 + blockIdx.y * G_ROWS;
    if (r0 >= B) return;
    auto row_of = [&](int n) {
        long long r = idx ? idx[n] : (long long)n;
        if (r < 0 || r >= n_rows) { r = 0; words[W_BAD_INDEX] = 1; }
        return r;
    };
    const int cnt = B - r0 < G_ROWS ? B - r0 : G_ROWS;
    if (tid < cnt) {
        const long long r = row_of(r0 + tid);
        rows[tid] = r;
        const int n = r0 + tid;
        s.old_lp[n] = f.old_lp[r]; s.adv[n] = f.adv[r]; s.ret[n] = f.ret[r];
        if (f.old_v) s.old_v[n] = f.old_v[r];
    }
    __syncthreads();
    for (int e = tid; e < cnt * D; e += P_NT) {
        const int row = e / D, k = e - row * D;
        s.obs[(size_t)(r0 + row) * D + k] = f.obs[(size_t)rows[row] * D + k];
    }
    for (int e = tid; e < cnt * A; e += P_NT) {
        const int row = e / A, k = e - row * A;
        s.act[(size_t)(r0 + row) * A + k] = f.act[(size_t)rows[row] * A + k];
    }
    if (sum_adv && blockIdx.y == 0) {
        const int c = B - n0 < CHUNK ? B - n0 : CHUNK;
        if (tid < c) adv_s[tid] = f.adv[row_of(n0 + tid)];
        __syncthreads();
        if (tid == 0) {
            double acc = 0.0;
            for (int i = 0; i < c; ++i) acc = acc + (double)adv_s[i];
            advpart[blockIdx.x] = acc;
        }
    }
}

// normalize_adv_ref on the staged advantages, a workgroup per chunk.  sum[] and sq[] hold the chunks' float64
// partials; PHASE 0 writes sq[chunk] = the sequential sum of (adv - mean)^2, PHASE 1 writes adv in place.
template <int PHASE>
__global__ __launch_bounds__(P_NT) void k_ppo_advnorm(const int* pred, int B, int n_chunks, float* __restrict__ adv,
                                                      const double* __restrict__ sum, double* sq) {
    if (*pred) return;
    __shared__ double sh[CHUNK];
    __shared__ double bc[2];
    const int tid = threadIdx.x, n0 = blockIdx.x * CHUNK, n = n0 + tid;
    if (tid == 0) {
        double acc = 0.0;
        for (int c = 0; c < n_chunks; ++c) acc = acc + sum[c];
        bc[0] = acc * (1.0 / (double)B);
        if (PHASE == 1) {
            double q = 0.0;
            for (int c = 0; c < n_chunks; ++c) q = q + sq[c];
            bc[1] = sqrt(q / (double)(B - 1)) + 1e-8;
        }
    }
    __syncthreads();
    const double dev = n < B ? (double)adv[n] - bc[0] : 0.0;
    if (PHASE == 0) {
        sh[tid] = dev * dev;
        __syncthreads();
        if (tid == 0) {
            const int c = B - n0 < CHUNK ? B - n0 : CHUNK;
            double acc = 0.0;
            for (int i = 0; i < c; ++i) acc = acc + sh[i];
            sq[blockIdx.x] = acc;
        }
    } else if (n < B) {
        adv[n] = (float)(dev / bc[1]);
    }
}

__global__ void k_exp(const float* __restrict__ x, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = mrp::exp_f32(x[i]);
}

thread_local std::string g_ppo_create_error;

}  // namespace

struct mrp_ppo {
    mrp_policy* policy = nullptr;
    int device = 0, max_batch = 0, max_chunks = 0, n_params = 0, n_tiles = 0, n_elems = 0, seen_version = -1;
    PpoNet pn = {};
    float* d_ws = nullptr;        // activations, deltas, terms
    float* d_rows = nullptr;      // row-major image of the hidden weights
    float* d_vec = nullptr;       // param, grad, m, v (n_params each), coef, the combined approx_kl
    float* d_partial = nullptr;   // [max_chunks][n_params]
    double* d_spart = nullptr;    // [max_chunks][NSTAT]
    int* d_idx = nullptr;         // fwd[n_params], row[n_params]
    WTile* d_tiles = nullptr;
    BElem* d_elems = nullptr;
    float* d_stage = nullptr;     // the staged minibatch: obs, actions, old_values, old_log_probs, advantages, returns
    double* d_advpart = nullptr;  // [2][max_chunks]: the chunks' advantage sums, then their sums of squared deviations
    int* d_words = nullptr;       // stopped, applied, bad_index
    std::string err;
    float* param() const { return d_vec; }
    float* grad() const { return d_vec + n_params; }
    float* m() const { return d_vec + 2 * (size_t)n_params; }
    float* v() const { return d_vec + 3 * (size_t)n_params; }
    float* coef() const { return d_vec + 4 * (size_t)n_params; }
    Stage stage() const {
        const size_t mb = (size_t)max_batch;
        float* q = d_stage + mb * (pn.net.obs_dim + pn.net.act_dim);
        return Stage{d_stage, d_stage + mb * pn.net.obs_dim, q, q + mb, q + 2 * mb, q + 3 * mb};
    }
};

namespace {

// the one way an entry refuses a call: "<who>: <what>" where its last_error reads it
int fail(std::string& err, const char* who, const char* what, int rc = MRP_E_ARG) {
    err = std::string(who) + ": " + what;
    return rc;
}

const char* const NO_PARAMS = "no parameters yet (mrp_policy_set_params)";   // with MRP_E_STATE
// the ABI's seven Adam scalars, which carry these names in every entry that takes them
#define ADAM_K (AdamK{beta1, one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, step_size, eps})

// the master copy and the row-major image follow the policy's parameters when those were set since the last call
void import_if_stale(mrp_ppo* o, hipStream_t st) {
    const mrp_policy* p = o->policy;
    if (o->seen_version != p->version) {
        const int P = o->n_params;
        hipLaunchKernelGGL(k_ppo_import, dim3((P + P_NT - 1) / P_NT), dim3(P_NT), 0, st, P, p->d_params, o->d_idx, o->d_idx + P,
                           o->param(), o->d_rows);
        o->seen_version = p->version;
    }
}

// clip + Adam on the object's own gradient; `words`: the progress words of a predicated call (null: none)
int ppo_adam_launch(mrp_ppo* o, hipStream_t st, AdamK k, int* words) {
    const int P = o->n_params;
    mrp_policy* p = o->policy;
    hipLaunchKernelGGL(k_ppo_adam, dim3((P + P_NT - 1) / P_NT), dim3(P_NT), 0, st, P, p->net.act_dim, o->grad(), o->coef(), o->param(),
                       o->m(), o->v(), o->d_idx, o->d_idx + P, p->d_params, o->d_rows, const_cast<float*>(p->net.std), k, words);
    MRP_HIPCHK(o, hipGetLastError());
    return MRP_OK;
}

// One minibatch, as every entry hands it over.  `in`: the caller's six arrays (old_v is read under cv >= 0); with `index`
// the minibatch is rows index[0..B) of their n_rows rows, gathered into the stage, where `normalize` takes the advantages
// too.  `words`: the progress words of a predicated call (null: none).  With `d_grad` the gradient alone: no clip, no
// Adam, no stop; else the step, with `adam` and the stop above 1.5 * target_kl (negative: none).
struct Minibatch {
    const char* who; hipStream_t st; int B; Fields in; float clip, ent_coef; double vf_coef; float* d_stats;   // every entry's
    const long long* index = nullptr; long long n_rows = 0; bool normalize = false; float cv = -1.0f; int* words = nullptr;
    double target_kl = -1.0, max_norm = 1.0; float* d_grad = nullptr; AdamK adam = {};
};

int ppo_minibatch(mrp_ppo* o, Minibatch a) {
    const int B = a.B;
    if (B < 1) return fail(o->err, a.who, "B < 1");
    if (B > o->max_batch) return fail(o->err, a.who, "B > max_batch");
    if (!a.in.obs || !a.in.act || !a.in.old_lp || !a.in.adv || !a.in.ret || !a.d_stats) return fail(o->err, a.who, "null pointer");
    if (!(a.cv < 0.0f) && !a.in.old_v) return fail(o->err, a.who, "clip_range_vf is set and d_old_values is null");
    if (a.index && a.n_rows < 1) return fail(o->err, a.who, "n_rows < 1");
    if (a.cv < 0.0f) a.in.old_v = nullptr;
    const Net& net = o->pn.net;
    const size_t f = sizeof(float), rows = a.index ? (size_t)a.n_rows : (size_t)B;
    if (const char* what = check_outputs({{a.index, (size_t)B * sizeof(long long)}, {a.in.obs, rows * net.obs_dim * f},
                                          {a.in.act, rows * net.act_dim * f}, {a.in.old_v, rows * f}, {a.in.old_lp, rows * f},
                                          {a.in.adv, rows * f}, {a.in.ret, rows * f}},
                                         {{a.d_stats, NSTAT * f}, {a.d_grad, (size_t)o->n_params * f}}))
        return fail(o->err, a.who, what);
    if (!o->policy->ready) return fail(o->err, a.who, NO_PARAMS, MRP_E_STATE);
    MRP_HIPCHK(o, hipSetDevice(o->device));
    const hipStream_t st = a.st;
    const int P = o->n_params, n_chunks = (B + CHUNK - 1) / CHUNK;
    Fields in = a.in;
    const bool norm = a.normalize && B > 1;      // SB3 skips a minibatch of one sample
    if (a.index || norm) {
        const Stage sg = o->stage();
        const int first = B < CHUNK ? B : CHUNK;
        hipLaunchKernelGGL(k_ppo_gather, dim3(n_chunks, (first + G_ROWS - 1) / G_ROWS), dim3(P_NT), 0, st, a.words, a.words, B, a.index,
                           (long long)rows, in, sg, net.obs_dim, net.act_dim, norm ? 1 : 0, o->d_advpart);
        if (norm) {
            double* sq = o->d_advpart + o->max_chunks;
            hipLaunchKernelGGL(k_ppo_advnorm<0>, dim3(n_chunks), dim3(P_NT), 0, st, a.words, B, n_chunks, sg.adv, o->d_advpart, sq);
            hipLaunchKernelGGL(k_ppo_advnorm<1>, dim3(n_chunks), dim3(P_NT), 0, st, a.words, B, n_chunks, sg.adv, o->d_advpart, sq);
        }
        in = Fields{sg.obs, sg.act, in.old_v ? sg.old_v : nullptr, sg.old_lp, sg.adv, sg.ret};
    }
    import_if_stale(o, st);
    float* g = a.d_grad ? a.d_grad : o->grad();
    hipLaunchKernelGGL(k_ppo_fb, dim3((B + P_TILE - 1) / P_TILE), dim3(P_NT), 0, st, o->pn, B, in.obs, in.act, in.old_lp, in.adv, in.ret,
                       a.clip, (float)(2.0 * a.vf_coef), (float)(1.0 / (double)B), in.old_v, a.cv, a.words);
    const int waves = o->n_tiles * n_chunks;
    hipLaunchKernelGGL(k_ppo_wgrad, dim3((waves + 3) / 4), dim3(P_NT), 0, st, o->d_tiles, o->n_tiles, B, in.obs, net.obs_dim,
                       o->d_partial, P, a.words);
    hipLaunchKernelGGL(k_ppo_bsum, dim3(n_chunks, (o->n_elems + P_NT - 1) / P_NT + 1), dim3(P_NT), 0, st, o->d_elems, o->n_elems, B,
                       o->pn.sterm, o->d_partial, P, o->d_spart, a.words);
    hipLaunchKernelGGL(k_ppo_reduce, dim3((P + P_NT - 1) / P_NT), dim3(P_NT), 0, st, o->d_partial, P, n_chunks, net.act_dim, a.ent_coef,
                       g, a.words);
    hipLaunchKernelGGL(k_ppo_norm<false>, dim3(1), dim3(P_NT), 0, st, g, P, a.d_grad ? 1.0 : a.max_norm, o->d_spart, n_chunks, B,
                       o->coef(), a.d_stats, a.words, a.d_grad || a.target_kl < 0.0 ? -1.0 : 1.5 * a.target_kl);
    MRP_HIPCHK(o, hipGetLastError());
    return a.d_grad ? MRP_OK : ppo_adam_launch(o, st, a.adam, a.words);
}

}  // namespace

extern "C" {

const char* mrp_ppo_last_error(const mrp_ppo* o) { return o ? o->err.c_str() : g_ppo_create_error.c_str(); }

int mrp_ppo_n_params(const mrp_ppo* o) { return o ? o->n_params : MRP_E_ARG; }   // mrp_policy_n_params of its policy

void mrp_ppo_destroy(mrp_ppo* o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    (void)hipDeviceSynchronize();
    void* ptrs[] = {o->d_ws, o->d_rows, o->d_vec, o->d_partial, o->d_spart, o->d_idx, o->d_tiles, o->d_elems,
                    o->d_stage, o->d_advpart, o->d_words};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    delete o;
}

int mrp_ppo_create(mrp_policy* policy, int max_batch, mrp_ppo** out) {
    std::string& err = g_ppo_create_error;
    err.clear();
    const char* who = "mrp_ppo_create";
    if (!out) return fail(err, who, "null out");
    *out = nullptr;
    if (!policy) return fail(err, who, "null policy");
    if (max_batch < 1 || max_batch > (1 << 20)) return fail(err, who, "max_batch outside 1..1048576");
    mrp_ppo* o = new (std::nothrow) mrp_ppo();
    if (!o) return fail(err, who, "out of host memory");
    o->policy = policy; o->device = policy->device; o->max_batch = max_batch;
    o->max_chunks = (max_batch + CHUNK - 1) / CHUNK;
    const Net& net = policy->net;
    PpoNet& pn = o->pn;
    pn.net = net;
    const int S = net.n_shared, NP = net.n_pi, NV = net.n_vf, nl = S + NP + NV, A = net.act_dim, D = net.obs_dim;
    std::vector<const Layer*> layers;
    for (int i = 0; i < S; ++i) layers.push_back(&net.shared[i]);
    for (int i = 0; i < NP; ++i) layers.push_back(&net.pi[i]);
    for (int i = 0; i < NV; ++i) layers.push_back(&net.vf[i]);
    // the input of hidden layer li: -1 the observations, else a layer index
    auto input_of = [&](int li) { return li == 0 ? -1 : (li == S || li == S + NP) ? S - 1 : li - 1; };
    // the row-major image [N][pad32(K)] of every hidden layer's weights, one behind the other
    size_t rows_floats = 0;
    std::vector<size_t> rows_at(nl);
    for (int li = 0; li < nl; ++li) { rows_at[li] = rows_floats; rows_floats += (size_t)layers[li]->N * pad32(layers[li]->K); }
    // one walk of the policy's parameter map (flat order): the two image indices of every element, and where
    // each layer's weight and bias begin in the flat vector
    std::vector<int> fwd, row;
    std::vector<int> w_off(nl + 2), b_off(nl + 2);
    for (const ParamRef& r : policy->map) {
        const bool hidden_weight = r.slot >= 0 && r.slot < nl && r.k >= 0;
        const int flat = (int)fwd.size();
        if (r.slot >= 0 && r.j == 0 && r.k == 0) w_off[r.slot] = flat;
        if (r.slot >= 0 && r.j == 0 && r.k < 0) b_off[r.slot] = flat;
        fwd.push_back(r.image);
        row.push_back(hidden_weight ? (int)(rows_at[r.slot] + (size_t)r.j * pad32(layers[r.slot]->K) + r.k) : -1);
    }
    const int P = o->n_params = (int)fwd.size();
    // the workspace: activations and deltas per hidden layer, the heads' deltas, the log_std and statistics terms
    size_t ws = 0;
    std::vector<size_t> act_at(nl), delta_at(nl);
    for (int li = 0; li < nl; ++li) {
        act_at[li] = ws; ws += (size_t)max_batch * layers[li]->Npad;
        delta_at[li] = ws; ws += (size_t)max_batch * layers[li]->Npad;
    }
    const size_t dact_at = ws, dval_at = ws + (size_t)max_batch * HW, ls_at = ws + 2 * (size_t)max_batch * HW;
    const size_t st_at = ws + 3 * (size_t)max_batch * HW;
    ws = st_at + (size_t)max_batch * SW;
    hipError_t e = hipSetDevice(o->device);
    auto alloc = [&](void** q, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(q, bytes ? bytes : 4);
        if (e == hipSuccess) e = hipMemset(*q, 0, bytes ? bytes : 4);
    };
    alloc((void**)&o->d_ws, ws * sizeof(float));
    // one padded row more than the images hold: with a single output row (K2 == 0) hidden_layer's tail still
    // requests k-step 0 for both halves of the wave, and the lanes of the upper half read the row behind
    // the image (the value is not used; in k_policy's image the bias follows the weights)
    alloc((void**)&o->d_rows, (rows_floats + P_MAXW) * sizeof(float));
    alloc((void**)&o->d_vec, (4 * (size_t)P + 4) * sizeof(float));
    alloc((void**)&o->d_partial, (size_t)o->max_chunks * P * sizeof(float));
    alloc((void**)&o->d_spart, (size_t)o->max_chunks * NSTAT * sizeof(double));
    alloc((void**)&o->d_idx, 2 * (size_t)P * sizeof(int));
    alloc((void**)&o->d_stage, (size_t)max_batch * (D + A + 4) * sizeof(float));
    alloc((void**)&o->d_advpart, 2 * (size_t)o->max_chunks * sizeof(double));
    alloc((void**)&o->d_words, NWORDS * sizeof(int));
    if (e == hipSuccess) {
        for (int li = 0; li < nl; ++li) {
            const Layer& L = *layers[li];
            pn.act[li] = o->d_ws + act_at[li];
            pn.delta[li] = o->d_ws + delta_at[li];
            pn.bwd[li] = Layer{o->d_rows + rows_at[li], nullptr, L.N, L.K, pad32(L.K)};
        }
        pn.delta[L_ACT] = o->d_ws + dact_at; pn.delta[L_VAL] = o->d_ws + dval_at;
        pn.lsterm = o->d_ws + ls_at; pn.sterm = o->d_ws + st_at;
    }
    // the weight-gradient tiles and the bias elements
    std::vector<WTile> tiles;
    std::vector<BElem> elems;
    auto add_layer = [&](const float* delta, int dstride, int in, int N, int K, int woff, int boff) {
        const float* x = in < 0 ? nullptr : pn.act[in];
        const int xstride = in < 0 ? D : layers[in]->Npad;
        for (int j0 = 0; j0 < N; j0 += 32)
            for (int k0 = 0; k0 < K; k0 += 32) tiles.push_back(WTile{delta, x, dstride, xstride, j0, k0, N, K, woff});
        for (int j = 0; j < N; ++j) elems.push_back(BElem{delta + j, dstride, boff + j});
    };
    if (e == hipSuccess) {
        for (int i = 0; i < A; ++i) elems.push_back(BElem{pn.lsterm + i, HW, i});
        for (int li = 0; li < nl; ++li) add_layer(pn.delta[li], layers[li]->Npad, input_of(li), layers[li]->N, layers[li]->K, w_off[li], b_off[li]);
        const int in_pi = NP ? S + NP - 1 : S - 1, in_vf = NV ? S + NP + NV - 1 : S - 1;
        add_layer(pn.delta[L_ACT], HW, in_pi, A, net.act.K, w_off[nl], b_off[nl]);
        add_layer(pn.delta[L_VAL], HW, in_vf, 1, net.val.K, w_off[nl + 1], b_off[nl + 1]);
        o->n_tiles = (int)tiles.size(); o->n_elems = (int)elems.size();
        alloc((void**)&o->d_tiles, tiles.size() * sizeof(WTile));
        alloc((void**)&o->d_elems, elems.size() * sizeof(BElem));
    }
    if (e == hipSuccess) e = hipMemcpy(o->d_idx, fwd.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->d_idx + P, row.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->d_tiles, tiles.data(), tiles.size() * sizeof(WTile), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->d_elems, elems.data(), elems.size() * sizeof(BElem), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        err = std::string("mrp_ppo_create: ") + hipGetErrorString(e);
        mrp_ppo_destroy(o);
        return MRP_E_HIP;
    }
    *out = o;
    return MRP_OK;
}

int mrp_ppo_grad_device(mrp_ppo* o, void* hip_stream, int B, const float* d_obs, const float* d_actions, const float* d_old_log_probs,
                        const float* d_advantages, const float* d_returns, float clip_range, float ent_coef, double vf_coef,
                        float* d_grad, float* d_stats) {
    if (!o) return MRP_E_ARG;
    if (!d_grad) return fail(o->err, "mrp_ppo_grad_device", "null pointer");
    Minibatch a{"mrp_ppo_grad_device", (hipStream_t)hip_stream, B, {d_obs, d_actions, nullptr, d_old_log_probs, d_advantages, d_returns},
                clip_range, ent_coef, vf_coef, d_stats};
    a.d_grad = d_grad;
    return ppo_minibatch(o, a);
}

int mrp_ppo_step_device(mrp_ppo* o, void* hip_stream, int B, const float* d_obs, const float* d_actions, const float* d_old_log_probs,
                        const float* d_advantages, const float* d_returns, float clip_range, float ent_coef, double vf_coef,
                        double max_grad_norm, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float sqrt_bc2,
                        float step_size, float eps, float* d_stats) {
    if (!o) return MRP_E_ARG;
    Minibatch a{"mrp_ppo_step_device", (hipStream_t)hip_stream, B, {d_obs, d_actions, nullptr, d_old_log_probs, d_advantages, d_returns},
                clip_range, ent_coef, vf_coef, d_stats};
    a.max_norm = max_grad_norm; a.adam = ADAM_K;
    return ppo_minibatch(o, a);
}

int mrp_ppo_begin_device(mrp_ppo* o, void* hip_stream) {
    if (!o) return MRP_E_ARG;
    MRP_HIPCHK(o, hipSetDevice(o->device));
    MRP_HIPCHK(o, hipMemsetAsync(o->d_words, 0, NWORDS * sizeof(int), (hipStream_t)hip_stream));
    return MRP_OK;
}

int mrp_ppo_minibatch_device(mrp_ppo* o, void* hip_stream, int B, const long long* d_index, long long n_rows, const float* d_obs,
                             const float* d_actions, const float* d_old_values, const float* d_old_log_probs,
                             const float* d_advantages, const float* d_returns, int normalize_advantage, float clip_range,
                             float clip_range_vf, double target_kl, float ent_coef, double vf_coef, double max_grad_norm,
                             float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float sqrt_bc2,
                             float step_size, float eps, float* d_grad, float* d_stats) {
    if (!o) return MRP_E_ARG;
    Minibatch a{"mrp_ppo_minibatch_device", (hipStream_t)hip_stream, B,
                {d_obs, d_actions, d_old_values, d_old_log_probs, d_advantages, d_returns}, clip_range, ent_coef, vf_coef, d_stats};
    a.index = d_index; a.n_rows = n_rows; a.normalize = normalize_advantage != 0; a.cv = clip_range_vf;
    a.words = o->d_words; a.target_kl = target_kl; a.max_norm = max_grad_norm; a.d_grad = d_grad; a.adam = ADAM_K;
    return ppo_minibatch(o, a);
}

int mrp_ppo_apply_device(mrp_ppo* o, void* hip_stream, int R, const float* d_parts, long long part_stride, double target_kl,
                         double max_grad_norm, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float sqrt_bc2,
                         float step_size, float eps, float* d_stats) {
    if (!o) return MRP_E_ARG;
    const char* who = "mrp_ppo_apply_device";
    if (R < 1 || R > 64) return fail(o->err, who, "R outside 1..64");
    if (!d_parts || !d_stats) return fail(o->err, who, "null pointer");
    const int P = o->n_params;
    if (part_stride < (long long)P + NSTAT) return fail(o->err, who, "part_stride < n_params + 5");
    const size_t f = sizeof(float);
    if (const char* what = check_outputs({{d_parts, (size_t)R * (size_t)part_stride * f}}, {{d_stats, NSTAT * f}})) return fail(o->err, who, what);
    if (!o->policy->ready) return fail(o->err, who, NO_PARAMS, MRP_E_STATE);
    MRP_HIPCHK(o, hipSetDevice(o->device));
    const hipStream_t st = (hipStream_t)hip_stream;
    import_if_stale(o, st);
    hipLaunchKernelGGL(k_ppo_combine, dim3((P + NSTAT + P_NT - 1) / P_NT), dim3(P_NT), 0, st, d_parts, R, (size_t)part_stride, P,
                       (float)(1.0 / (double)R), o->grad(), d_stats, o->coef() + 1, o->d_words);
    hipLaunchKernelGGL(k_ppo_norm<true>, dim3(1), dim3(P_NT), 0, st, o->grad(), P, max_grad_norm, nullptr, 0, 0, o->coef(), nullptr,
                       o->d_words, target_kl < 0.0 ? -1.0 : 1.5 * target_kl);
    return ppo_adam_launch(o, st, ADAM_K, o->d_words);
}

int mrp_ppo_progress(mrp_ppo* o, void* hip_stream, int* stopped, int* applied) {
    if (!o) return MRP_E_ARG;
    if (!stopped || !applied) { o->err = "mrp_ppo_progress: null pointer"; return MRP_E_ARG; }
    int w[NWORDS] = {};
    MRP_HIPCHK(o, hipSetDevice(o->device));
    MRP_HIPCHK(o, hipStreamSynchronize((hipStream_t)hip_stream));
    MRP_HIPCHK(o, hipMemcpy(w, o->d_words, sizeof(w), hipMemcpyDeviceToHost));
    *stopped = w[W_STOPPED]; *applied = w[W_APPLIED];
    if (w[W_BAD_INDEX]) {
        o->err = "mrp_ppo_progress: an index outside [0, n_rows) since mrp_ppo_begin_device (row 0 was read in its place)";
        return MRP_E_ARG;
    }
    return MRP_OK;
}

int mrp_ppo_get_staged(mrp_ppo* o, int B, float* obs, float* actions, float* old_values, float* old_log_probs, float* advantages,
                       float* returns) {
    if (!o) return MRP_E_ARG;
    if (B < 1 || B > o->max_batch) { o->err = "mrp_ppo_get_staged: B outside 1..max_batch"; return MRP_E_ARG; }
    MRP_HIPCHK(o, hipSetDevice(o->device));
    MRP_HIPCHK(o, hipDeviceSynchronize());
    const Stage sg = o->stage();
    const size_t nB = (size_t)B * sizeof(float);
    const struct { float* dst; const float* src; size_t bytes; } copies[] = {
        {obs, sg.obs, nB * o->pn.net.obs_dim}, {actions, sg.act, nB * o->pn.net.act_dim}, {old_values, sg.old_v, nB},
        {old_log_probs, sg.old_lp, nB}, {advantages, sg.adv, nB}, {returns, sg.ret, nB}};
    for (const auto& c : copies)
        if (c.dst) MRP_HIPCHK(o, hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost));
    return MRP_OK;
}

int mrp_ppo_get_state(mrp_ppo* o, float* m, float* v) {
    if (!o) return MRP_E_ARG;
    if (!m || !v) { o->err = "mrp_ppo_get_state: null pointer"; return MRP_E_ARG; }
    MRP_HIPCHK(o, hipSetDevice(o->device));
    MRP_HIPCHK(o, hipDeviceSynchronize());
    MRP_HIPCHK(o, hipMemcpy(m, o->m(), (size_t)o->n_params * sizeof(float), hipMemcpyDeviceToHost));
    MRP_HIPCHK(o, hipMemcpy(v, o->v(), (size_t)o->n_params * sizeof(float), hipMemcpyDeviceToHost));
    return MRP_OK;
}

int mrp_ppo_set_state(mrp_ppo* o, const float* m, const float* v) {
    if (!o) return MRP_E_ARG;
    if (!m || !v) { o->err = "mrp_ppo_set_state: null pointer"; return MRP_E_ARG; }
    MRP_HIPCHK(o, hipSetDevice(o->device));
    MRP_HIPCHK(o, hipDeviceSynchronize());
    MRP_HIPCHK(o, hipMemcpy(o->m(), m, (size_t)o->n_params * sizeof(float), hipMemcpyHostToDevice));
    MRP_HIPCHK(o, hipMemcpy(o->v(), v, (size_t)o->n_params * sizeof(float), hipMemcpyHostToDevice));
    return MRP_OK;
}

int mrp_selftest_exp(int device, const float* x, float* out, int n) {
    return selftest_elementwise(device, x, out, nullptr, n, [](dim3 grid, dim3 block, const float* dx, float* dy, float*, int cnt) {
        hipLaunchKernelGGL(k_exp, grid, block, 0, 0, dx, dy, cnt);
    });
}

}  // extern "C"
