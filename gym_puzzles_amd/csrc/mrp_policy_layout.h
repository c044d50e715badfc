// mrp_policy_layout.h -- where every parameter of the device policy lives, stated once: the policy
// object, the layout of its device image, and the map from the flat parameter order of include/mrp.h
// to that image.  mrp_policy_set_params scatters through the map, mrp_policy_get_params gathers, and
// the PPO update (mrp_ppo.hip) takes its index tables from it.  Host only, and no HIP runtime call:
// tests/policy_layout_check.cpp walks the map on the CPU.
#pragma once
#include <string>
#include <vector>

#include "mrp_host.h"
#include "mrp_policy_net.h"

namespace mrp_pol {

// One parameter; its index in the map is its flat index.  `image` is its float offset in the device
// image.  `slot` is its layer: the hidden layers in the order of `widths` (trunk, policy tower, value
// tower), then the action head (n_layers) and the value head (n_layers + 1); SLOT_LOG_STD for log_std.
// (j, k) is its place in torch's weight [out = j][in = k]; k = -1 for element j of a bias or of log_std.
struct ParamRef { int image, slot, j, k; };
constexpr int SLOT_LOG_STD = -1;

}  // namespace mrp_pol

struct mrp_policy {
    int device = 0, ready = 0, n_layers = 0;
    int version = 0;                 // counts mrp_policy_set_params calls: mrp_ppo re-imports its master copy when it moves
    int widths[3 * mrp_pol::P_MAXL] = {};
    mrp_pol::Net net = {};
    float* d_params = nullptr;
    size_t n_floats = 0;
    std::vector<mrp_pol::ParamRef> map;   // param_map(), built once by mrp_policy_create
    std::string err;
};

namespace mrp_pol {

// the device image of the parameters: per hidden layer the packed weights [K][Npad] and bias [Npad],
// then the heads' rows (padded to 4 floats), log_std and std; fills the Net's pointers relative to `base`
inline size_t layout(mrp_policy* p, float* base) {
    Net& n = p->net;
    size_t off = 0;
    auto take = [&](size_t count) { float* q = base ? base + off : nullptr; off += (count + 3) & ~(size_t)3; return q; };
    int li = 0;
    auto towers = [&](Layer* L, int count, int K) {
        for (int i = 0; i < count; ++i, ++li) {
            L[i].K = K; L[i].N = p->widths[li]; L[i].Npad = mrp_host::pad32(L[i].N);
            L[i].w = take((size_t)K * L[i].Npad);
            L[i].b = take(L[i].Npad);
            K = L[i].N;
        }
        return K;
    };
    const int kt = towers(n.shared, n.n_shared, n.obs_dim);
    n.act.K = towers(n.pi, n.n_pi, kt);
    n.val.K = towers(n.vf, n.n_vf, kt);
    n.act.Kpad = (n.act.K + 3) & ~3; n.val.Kpad = (n.val.K + 3) & ~3;
    n.act.w = take((size_t)n.act_dim * n.act.Kpad); n.act.b = take(n.act_dim);
    n.val.w = take(n.val.Kpad); n.val.b = take(1);
    n.log_std = take(n.act_dim); n.std = take(n.act_dim);
    return off;
}

// The parameters in the flat order of include/mrp.h (SB3's parameters()): log_std, then trunk, policy
// tower, value tower, action head, value head, each weight row-major [out][in], then bias.  Needs the
// Net's pointers laid out relative to p.d_params (layout(&p, p.d_params)); std is no parameter.
inline std::vector<ParamRef> param_map(const mrp_policy& p) {
    const Net& n = p.net;
    std::vector<ParamRef> map;
    auto at = [&](const float* q) { return (int)(q - p.d_params); };
    for (int i = 0; i < n.act_dim; ++i) map.push_back({at(n.log_std) + i, SLOT_LOG_STD, i, -1});
    int slot = 0;
    // a layer of `outs` rows whose weight [j][k] sits at w + j * sj + k * sk
    auto layer = [&](const float* w, const float* b, int outs, int K, int sj, int sk) {
        for (int j = 0; j < outs; ++j)
            for (int k = 0; k < K; ++k) map.push_back({at(w) + j * sj + k * sk, slot, j, k});
        for (int j = 0; j < outs; ++j) map.push_back({at(b) + j, slot, j, -1});
        ++slot;
    };
    auto towers = [&](const Layer* L, int count) {
        for (int i = 0; i < count; ++i) layer(L[i].w, L[i].b, L[i].N, L[i].K, 1, L[i].Npad);   // packed [K][Npad]
    };
    towers(n.shared, n.n_shared); towers(n.pi, n.n_pi); towers(n.vf, n.n_vf);
    layer(n.act.w, n.act.b, n.act_dim, n.act.K, n.act.Kpad, 1);                                  // torch's rows, padded
    layer(n.val.w, n.val.b, 1, n.val.K, n.val.Kpad, 1);
    return map;
}

}  // namespace mrp_pol
