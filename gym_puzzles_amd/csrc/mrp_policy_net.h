// mrp_policy_net.h -- what the device policy's forward kernel (mrp_policy.hip) and the PPO update
// (mrp_ppo.hip) share: the Net the kernels take by value and the device code of a hidden layer
// (v_mfma_f32_32x32x2_f32 over activations in LDS) and of a narrow head.  See mrp_policy.hip for the
// kernel shape and the lane maps, mrp_policy_layout.h for the policy object and its parameter map.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mrp.h"
#include "mrp_math.h"

namespace mrp_pol {

constexpr int P_NT = 256;        // 4 waves
constexpr int P_TILE = 32;       // lanes (rows) per workgroup
constexpr int P_LDA = 258;       // LDS row stride in floats: rows land 2 banks apart, so the A read
                                 // (32 rows x 2 consecutive k) touches 64 different banks
constexpr int P_MAXW = 256, P_MAXA = 16, P_MAXL = 4;
constexpr int P_U = 8;          // k-steps of a hidden layer whose operands are in flight together
constexpr int P_HS = P_MAXA + 1; // head outputs per row: act_dim means, then the value
constexpr int STREAM_U1 = 4, STREAM_U2 = 5;   // rng_u01 stream ids (1-3: resets and synthetic actions)

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Layer { const float* w; const float* b; int K, N, Npad; };   // w packed [K][Npad], b [Npad]
struct Head { const float* w; const float* b; int K, Kpad; };        // w [out][Kpad]: torch's rows, padded to 4 floats
struct Net {
    int obs_dim, act_dim, n_shared, n_pi, n_vf, relu;
    Layer shared[P_MAXL], pi[P_MAXL], vf[P_MAXL];
    Head act, val;
    const float* log_std; const float* std;
};

static __device__ __forceinline__ float activate(float v, int relu) { return relu ? mrp::fmax_(v, 0.0f) : mrp::tanh_f32(v); }

// dst[32][N] = act(src[32][K] . W + b); src and dst are different LDS buffers.  BACKWARD (the PPO
// update's s = delta . W over torch's row-major image): the chain starts from +0 and dst takes the
// accumulator as it is.
template <bool BACKWARD = false>
static __device__ __forceinline__ void hidden_layer(const Layer& L, const float* __restrict__ src, float* __restrict__ dst, int relu) {
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 31, h = l >> 5;
    const int K2 = L.K & ~1, ntiles = L.Npad >> 5;
    const float* ap = src + c * P_LDA + h;                 // A[i = l & 31][k = l >> 5]
    for (int t = wave; t < ntiles; t += 4) {
        const int col = t * 32 + c;
        const float* wp = L.w + (size_t)h * L.Npad + col;  // B[k = l >> 5][j = l & 31]
        const float bias = BACKWARD ? 0.0f : L.b[col];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias;
        // k-steps in chunks of P_U: the next chunk's operands are requested before the chunk in hand
        // runs, so the L2 latency of a B row hides behind P_U matrix instructions of 64 cycles each
        const int nchunk = K2 / (2 * P_U);
        float a0[P_U], b0[P_U], a1[P_U] = {}, b1[P_U] = {};
        if (nchunk > 0) {
#pragma unroll
            for (int u = 0; u < P_U; ++u) { a0[u] = ap[2 * u]; b0[u] = wp[(size_t)(2 * u) * L.Npad]; }
        }
        int k = 0;
        for (int ch = 0; ch < nchunk; ++ch, k += 2 * P_U) {
            if (ch + 1 < nchunk) {
#pragma unroll
                for (int u = 0; u < P_U; ++u) {
                    a1[u] = ap[k + 2 * (P_U + u)];
                    b1[u] = wp[(size_t)(k + 2 * (P_U + u)) * L.Npad];
                }
            }
#pragma unroll
            for (int u = 0; u < P_U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], b0[u], acc, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < P_U; ++u) { a0[u] = a1[u]; b0[u] = b1[u]; }
        }
        // the last, partial chunk: its loads go out together (an index past the end reads k-step 0 again
        // and is not used), its matrix instructions run under wave-uniform tests
#pragma unroll
        for (int u = 0; u < P_U; ++u) {
            const int kk = k + 2 * u < K2 ? k + 2 * u : 0;
            a0[u] = ap[kk]; b0[u] = wp[(size_t)kk * L.Npad];
        }
#pragma unroll
        for (int u = 0; u < P_U; ++u)
            if (k + 2 * u < K2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], b0[u], acc, 0, 0, 0);
        // C/D: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        if (L.K & 1) {
            const float wv = L.w[(size_t)K2 * L.Npad + col];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                acc[r] = __builtin_fmaf(src[row * P_LDA + K2], wv, acc[r]);
            }
        }
        if (col < L.N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                dst[row * P_LDA + col] = BACKWARD ? acc[r] : activate(acc[r], relu);
            }
        }
    }
}

// out[row][o0 + o] = fmaf chain over src[row][0..K) and row o of w, from b[o]; 32 rows x 8 outputs at a time.
// The rows of w are padded to Kpad (a multiple of 4) in the device image, so 4 weights come per load.
static __device__ __forceinline__ void head(const Head& H, int n_out, const float* __restrict__ src, float* __restrict__ out, int o0) {
    const int row = threadIdx.x & 31, nq = H.K >> 2;
    const float* x = src + row * P_LDA;
    for (int o = threadIdx.x >> 5; o < n_out; o += P_NT / 32) {
        const float* w = H.w + (size_t)o * H.Kpad;
        const float4* w4 = reinterpret_cast<const float4*>(w);
        float acc = H.b[o];
        int q = 0;
        for (; q + P_U <= nq; q += P_U) {
            float4 wv[P_U];
#pragma unroll
            for (int u = 0; u < P_U; ++u) wv[u] = w4[q + u];
#pragma unroll
            for (int u = 0; u < P_U; ++u) {
                const float* xk = x + 4 * (q + u);
                acc = __builtin_fmaf(xk[0], wv[u].x, acc);
                acc = __builtin_fmaf(xk[1], wv[u].y, acc);
                acc = __builtin_fmaf(xk[2], wv[u].z, acc);
                acc = __builtin_fmaf(xk[3], wv[u].w, acc);
            }
        }
        for (int k = 4 * q; k < H.K; ++k) acc = __builtin_fmaf(x[k], w[k], acc);
        out[row * P_HS + o0 + o] = acc;
    }
}

}  // namespace mrp_pol
