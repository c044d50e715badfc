// mrp_policy.hip -- SB3's ActorCriticPolicy with MlpExtractor on the device: forward pass,
// diagonal-Gaussian sampling, log-prob, value and action clipping for a batch of lanes in ONE
// launch (DESIGN.md "Device policy").  The rule, which k_policy matches bit for bit, is
// gym_puzzles_amd/policy.py's policy_ref:
//   linear  : y[j] = fma(x[K-1], W[j][K-1], ... fma(x[0], W[j][0], b[j])), float32, k ascending
//   act     : tanh_f32 (mrp_math.h) or max(x, 0)
//   sample  : action = mean + std * eps; clipped = min(max(action, -1), 1);
//             log_prob = sum_i ((-(d_i * d_i)) / (2 * (std_i * std_i)) - log_std_i) - log(sqrt(2 pi)),
//             d = action - mean, the sum ascending from +0, every operation float32 and rounded alone
//
// Kernel shape: a workgroup of 4 waves takes a tile of 32 lanes through the whole network.  The
// activations of a layer live in LDS ([32][LDA] float, three buffers: the trunk's output stays while
// the policy tower runs); a hidden layer is v_mfma_f32_32x32x2_f32 with the bias as the initial
// accumulator -- on gfx950 that instruction is bit for bit the k-ordered fmaf chain of the rule --
// each wave owning the 32-column tiles w, w + 4, ... of the layer's output.  The weights were packed
// at set_params into [K][Npad] (Npad a multiple of 32, pad columns zero), so a wave's B operand of
// one k-step is two contiguous 128-byte rows streamed from L2.  An odd K's last term is an explicit
// fmaf on the accumulator registers (a zero pad k-step would turn an accumulator of -0 into +0).
// The narrow heads (act_dim, 1 outputs) are explicit fmaf chains on the VALU over torch's [out][in]
// rows, and the epilogue runs in the same launch.  Rows past n_lanes compute on zero observations
// and write nothing.  No atomics.
#include <hip/hip_runtime.h>

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

// a tower of n layers from buffer `in`, writing alternately to buffers a and b; returns the buffer of its output
__device__ __forceinline__ int tower(const Layer* L, int n, float* lds, int in, int a, int b, int relu) {
    for (int i = 0; i < n; ++i) {
        const int out = (i & 1) ? b : a;
        hidden_layer(L[i], lds + in * (P_TILE * P_LDA), lds + out * (P_TILE * P_LDA), relu);
        __syncthreads();
        in = out;
    }
    return in;
}

__global__ __launch_bounds__(P_NT) void k_policy(const Net net, int n_lanes, const float* __restrict__ obs,
                                                 const float* __restrict__ eps_in, uint64_t seed, uint64_t lane_offset,
                                                 uint64_t counter, int deterministic, int values_only,
                                                 float* __restrict__ actions, float* __restrict__ clipped,
                                                 float* __restrict__ values, float* __restrict__ log_probs,
                                                 float* __restrict__ eps_out) {
    __shared__ float lds[3 * P_TILE * P_LDA];
    __shared__ float hs[P_TILE * P_HS];     // the heads' outputs, then the log-prob terms
    const int tid = threadIdx.x, base = blockIdx.x * P_TILE;
    const int D = net.obs_dim, A = net.act_dim, relu = net.relu;
    for (int e = tid; e < P_TILE * D; e += P_NT) {
        const int row = e / D, k = e - row * D;
        const int lane = base + row;
        lds[row * P_LDA + k] = lane < n_lanes ? obs[(size_t)lane * D + k] : 0.0f;
    }
    __syncthreads();
    const int T = tower(net.shared, net.n_shared, lds, 0, 1, 0, relu);   // the trunk ping-pongs in buffers 0 and 1
    if (!values_only) {
        const int po = tower(net.pi, net.n_pi, lds, T, 1 - T, 2, relu);
        head(net.act, A, lds + po * (P_TILE * P_LDA), hs, 0);
        __syncthreads();                                                 // the value tower reuses the policy tower's buffers
    }
    const int vo = tower(net.vf, net.n_vf, lds, T, 1 - T, 2, relu);
    head(net.val, 1, lds + vo * (P_TILE * P_LDA), hs, P_MAXA);
    __syncthreads();
    const int row = tid & 31, lane = base + row;
    if (values && tid < P_TILE && lane < n_lanes) values[lane] = hs[row * P_HS + P_MAXA];
    if (values_only) return;
    float term[(P_MAXA + 7) / 8];
#pragma unroll
    for (int s = 0; s < (P_MAXA + 7) / 8; ++s) {
        const int i = (tid >> 5) + 8 * s;
        term[s] = 0.0f;
        if (i < A && lane < n_lanes) {
            const size_t e = (size_t)lane * A + i;
            const float m = hs[row * P_HS + i];
            const float sd = net.std[i];
            float eps = 0.0f, a = m;
            if (!deterministic) {
                if (eps_in) {
                    eps = eps_in[e];
                } else {   // Box-Muller in float64, u1 in (0, 1]
                    const uint64_t ctr = counter * (uint64_t)A + (uint64_t)i, gl = lane_offset + (uint64_t)lane;
                    const double u1 = 1.0 - mrp::rng_u01(seed, gl, STREAM_U1, ctr), u2 = mrp::rng_u01(seed, gl, STREAM_U2, ctr);
                    eps = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
                }
                a = m + sd * eps;
            }
            if (eps_out) eps_out[e] = eps;
            actions[e] = a;
            if (clipped) clipped[e] = mrp::fmin_(mrp::fmax_(a, -1.0f), 1.0f);
            const float d = a - m;
            const float q = (-(d * d)) / (2.0f * (sd * sd));
            term[s] = (q - net.log_std[i]) - 0x1.d67f1cp-1f;   // float32(log(sqrt(2 pi)))
        }
    }
    __syncthreads();                       // every mean has been read: hs now takes the terms
#pragma unroll
    for (int s = 0; s < (P_MAXA + 7) / 8; ++s) {
        const int i = (tid >> 5) + 8 * s;
        if (i < A) hs[row * P_HS + i] = term[s];
    }
    __syncthreads();
    if (tid < P_TILE && lane < n_lanes && log_probs) {
        float sum = 0.0f;
        for (int i = 0; i < A; ++i) sum = sum + hs[row * P_HS + i];
        log_probs[lane] = sum;
    }
}

__global__ void k_tanh(const float* __restrict__ x, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = mrp::tanh_f32(x[i]);
}

thread_local std::string g_policy_create_error;

int policy_launch(mrp_policy* p, void* hip_stream, int n_lanes, const float* d_obs, const float* d_eps_in, uint64_t seed,
                  uint64_t lane_offset, uint64_t counter, int deterministic, int values_only, float* d_actions, float* d_clipped,
                  float* d_values, float* d_log_probs, float* d_eps_out) {
    MRP_HIPCHK(p, hipSetDevice(p->device));
    const dim3 grid((unsigned)(((long long)n_lanes + P_TILE - 1) / P_TILE)), block(P_NT);
    hipLaunchKernelGGL(k_policy, grid, block, 0, (hipStream_t)hip_stream, p->net, n_lanes, d_obs, d_eps_in, seed, lane_offset,
                       counter, deterministic, values_only, d_actions, d_clipped, d_values, d_log_probs, d_eps_out);
    MRP_HIPCHK(p, hipGetLastError());
    return MRP_OK;
}

}  // namespace

extern "C" {

const char* mrp_policy_last_error(const mrp_policy* p) { return p ? p->err.c_str() : g_policy_create_error.c_str(); }

void mrp_policy_destroy(mrp_policy* p) {
    if (!p) return;
    if (p->d_params) {
        (void)hipSetDevice(p->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(p->d_params);
    }
    delete p;
}

int mrp_policy_create(int device, int obs_dim, int act_dim, int n_shared, int n_pi, int n_vf, const int* widths, int activation,
                      mrp_policy** out) {
    std::string& err = g_policy_create_error;
    err.clear();
    auto bad = [&](const char* what) { err = std::string("mrp_policy_create: ") + what; return MRP_E_ARG; };
    if (!out) return bad("null out");
    *out = nullptr;
    if (obs_dim < 1 || obs_dim > P_MAXW) return bad("obs_dim outside 1..256");
    if (act_dim < 1 || act_dim > P_MAXA) return bad("act_dim outside 1..16");
    if (n_shared < 0 || n_pi < 0 || n_vf < 0 || n_shared + (n_pi > n_vf ? n_pi : n_vf) > P_MAXL)
        return bad("layer counts: n_shared + max(n_pi, n_vf) must be 0..4");
    if (activation != MRP_POLICY_TANH && activation != MRP_POLICY_RELU) return bad("activation is neither tanh nor relu");
    const int nl = n_shared + n_pi + n_vf;
    if (nl > 0 && !widths) return bad("null widths");
    for (int i = 0; i < nl; ++i)
        if (widths[i] < 1 || widths[i] > P_MAXW) return bad("a layer width outside 1..256");
    if (const int rc = select_device(device, err)) {
        if (rc == MRP_E_ARG) err.insert(0, "mrp_policy_create: ");
        return rc;
    }
    mrp_policy* p = new (std::nothrow) mrp_policy();
    if (!p) return bad("out of host memory");
    p->device = device; p->n_layers = nl;
    for (int i = 0; i < nl; ++i) p->widths[i] = widths[i];
    p->net.obs_dim = obs_dim; p->net.act_dim = act_dim; p->net.n_shared = n_shared; p->net.n_pi = n_pi; p->net.n_vf = n_vf;
    p->net.relu = activation == MRP_POLICY_RELU;
    p->n_floats = layout(p, nullptr);
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipMalloc(&p->d_params, p->n_floats * sizeof(float))) != hipSuccess) {
        err = std::string("mrp_policy_create: ") + hipGetErrorString(e);
        p->d_params = nullptr;
        mrp_policy_destroy(p);
        return MRP_E_HIP;
    }
    layout(p, p->d_params);
    p->map = param_map(*p);
    *out = p;
    return MRP_OK;
}

int mrp_policy_n_params(const mrp_policy* p) { return p ? (int)p->map.size() : MRP_E_ARG; }

int mrp_policy_set_params(mrp_policy* p, const float* flat, const float* std) {
    if (!p) return MRP_E_ARG;
    if (!flat || !std) { p->err = "mrp_policy_set_params: null pointer"; return MRP_E_ARG; }
    std::vector<float> h(p->n_floats, 0.0f);   // the pad columns and pad rows stay zero
    for (size_t e = 0; e < p->map.size(); ++e) h[p->map[e].image] = flat[e];
    for (int i = 0; i < p->net.act_dim; ++i) h[(p->net.std - p->d_params) + i] = std[i];
    MRP_HIPCHK(p, hipSetDevice(p->device));
    MRP_HIPCHK(p, hipDeviceSynchronize());   // no launch still reads the old parameters
    MRP_HIPCHK(p, hipMemcpy(p->d_params, h.data(), p->n_floats * sizeof(float), hipMemcpyHostToDevice));
    p->ready = 1;
    ++p->version;
    return MRP_OK;
}

int mrp_policy_get_params(mrp_policy* p, float* flat, float* std) {
    if (!p) return MRP_E_ARG;
    if (!flat || !std) { p->err = "mrp_policy_get_params: null pointer"; return MRP_E_ARG; }
    if (!p->ready) { p->err = "mrp_policy_get_params: no parameters yet (mrp_policy_set_params)"; return MRP_E_STATE; }
    std::vector<float> h(p->n_floats);
    MRP_HIPCHK(p, hipSetDevice(p->device));
    MRP_HIPCHK(p, hipDeviceSynchronize());   // every launch that writes the parameters has finished
    MRP_HIPCHK(p, hipMemcpy(h.data(), p->d_params, p->n_floats * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < p->map.size(); ++e) flat[e] = h[p->map[e].image];
    for (int i = 0; i < p->net.act_dim; ++i) std[i] = h[(p->net.std - p->d_params) + i];
    return MRP_OK;
}

int mrp_policy_act_device(mrp_policy* p, void* hip_stream, int n_lanes, const float* d_obs, const float* d_eps_in, uint64_t seed,
                          uint64_t lane_offset, uint64_t counter, int deterministic, float* d_actions, float* d_clipped,
                          float* d_values, float* d_log_probs, float* d_eps_out) {
    if (!p) return MRP_E_ARG;
    auto bad = [&](const char* what) { p->err = std::string("mrp_policy_act_device: ") + what; return MRP_E_ARG; };
    if (n_lanes < 1) return bad("n_lanes < 1");
    if (!d_obs || !d_actions) return bad("null pointer");
    const size_t n = (size_t)n_lanes * sizeof(float), nO = n * p->net.obs_dim, nA = n * p->net.act_dim;
    if (const char* what = check_outputs({{d_obs, nO}, {d_eps_in, nA}},
                                         {{d_actions, nA}, {d_clipped, nA}, {d_values, n}, {d_log_probs, n}, {d_eps_out, nA}}))
        return bad(what);
    if (!p->ready) { p->err = "mrp_policy_act_device: no parameters yet (mrp_policy_set_params)"; return MRP_E_STATE; }
    return policy_launch(p, hip_stream, n_lanes, d_obs, d_eps_in, seed, lane_offset, counter, deterministic ? 1 : 0, 0, d_actions,
                         d_clipped, d_values, d_log_probs, d_eps_out);
}

int mrp_policy_values_device(mrp_policy* p, void* hip_stream, int n_lanes, const float* d_obs, float* d_values) {
    if (!p) return MRP_E_ARG;
    auto bad = [&](const char* what) { p->err = std::string("mrp_policy_values_device: ") + what; return MRP_E_ARG; };
    if (n_lanes < 1) return bad("n_lanes < 1");
    if (!d_obs || !d_values) return bad("null pointer");
    const size_t n = (size_t)n_lanes * sizeof(float);
    if (const char* what = check_outputs({{d_obs, n * p->net.obs_dim}}, {{d_values, n}})) return bad(what);
    if (!p->ready) { p->err = "mrp_policy_values_device: no parameters yet (mrp_policy_set_params)"; return MRP_E_STATE; }
    return policy_launch(p, hip_stream, n_lanes, d_obs, nullptr, 0, 0, 0, 1, 1, nullptr, nullptr, d_values, nullptr, nullptr);
}

int mrp_selftest_tanh(int device, const float* x, float* out, int n) {
    return selftest_elementwise(device, x, out, nullptr, n, [](dim3 grid, dim3 block, const float* dx, float* dy, float*, int cnt) {
        hipLaunchKernelGGL(k_tanh, grid, block, 0, 0, dx, dy, cnt);
    });
}

}  // extern "C"
