// Host walk of the device policy's parameter map (gym_puzzles_amd/csrc/mrp_policy_layout.h), the one
// enumeration that mrp_policy_set_params, mrp_policy_get_params and mrp_ppo_create share.
// tests/test_policy_layout.py builds this host-only with the address and undefined-behaviour sanitizers
// and compares what it prints with a numpy restatement of the device image.
//   usage : policy_layout_check obs_dim act_dim n_shared n_pi n_vf [width ...]
//   prints: "n_floats n_params", then one line per flat index: "image slot j k rowmajor", rowmajor
//           being the element's offset in torch's row-major weight [out][in] (j for a bias or log_std)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gym_puzzles_amd/csrc/mrp_policy_layout.h"

using namespace mrp_pol;

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    mrp_policy p;
    Net& n = p.net;
    n.obs_dim = std::atoi(argv[1]); n.act_dim = std::atoi(argv[2]);
    n.n_shared = std::atoi(argv[3]); n.n_pi = std::atoi(argv[4]); n.n_vf = std::atoi(argv[5]);
    p.n_layers = n.n_shared + n.n_pi + n.n_vf;
    if (p.n_layers != argc - 6 || p.n_layers > 3 * P_MAXL) return 2;
    for (int i = 0; i < p.n_layers; ++i) p.widths[i] = std::atoi(argv[6 + i]);
    p.n_floats = layout(&p, nullptr);
    std::vector<float> image(p.n_floats);       // stands in for the device image: only its addresses are used
    p.d_params = image.data();
    if (layout(&p, p.d_params) != p.n_floats) return 1;
    p.map = param_map(p);
    // a slot's input width, as mrp_policy_create lays the layers out
    std::vector<int> K;
    for (int i = 0; i < n.n_shared; ++i) K.push_back(n.shared[i].K);
    for (int i = 0; i < n.n_pi; ++i) K.push_back(n.pi[i].K);
    for (int i = 0; i < n.n_vf; ++i) K.push_back(n.vf[i].K);
    K.push_back(n.act.K); K.push_back(n.val.K);
    std::printf("%zu %zu\n", p.n_floats, p.map.size());
    for (const ParamRef& r : p.map) {
        if (r.slot != SLOT_LOG_STD && (r.slot < 0 || r.slot >= (int)K.size())) return 1;
        std::printf("%d %d %d %d %d\n", r.image, r.slot, r.j, r.k, r.k < 0 ? r.j : r.j * K[r.slot] + r.k);
    }
    return 0;
}
