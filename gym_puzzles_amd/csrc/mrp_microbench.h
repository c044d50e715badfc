// mrp_microbench.h -- the v0 solver micro-benchmarks (mrp_debug_velbench / mrp_debug_posbench).
// Included by mrp_unit.hip after mrp_lane.h, for env 0's unit only: they run on World<0>, v0's
// tables and that unit's g_table, and are reached through velbench_launch / posbench_launch
// (mrp_ops.h), not through the EnvOps table.
#pragma once
#include "mrp_lane.h"

namespace {
// Diagnostic micro-benchmark of the lane-distributed velocity sweeps (mrp_debug_velbench): a
// synthetic v0 island of nc agent-block contacts with pcount manifold points each, swept `iters`
// times with the early exit off; out[block] = s_memtime cycles of the sweeps.
__global__ __launch_bounds__(BLOCK, MRP_STEP_WAVES_PER_EU) void k_velbench(int nc, int pcount, int iters, unsigned long long* out) {
    using W = World<0>;
    __shared__ Shared<0> sh;
    const int tid = threadIdx.x;
    EnvParams P{};
    W w(sh, g_table, P, tid);
    auto& is = sh.isl;
    // nc >= 100: a chain of nc - 100 contacts (contact i between bodies i and i + 1, all moving)
    const bool chain = nc >= 100;
    if (chain) nc -= 100;
    if (tid == 0) {
        is.nb = nc + 1; is.nc = nc;
        for (int b = 0; b <= nc; ++b) { is.vvx[b] = 0.3f * b - 0.1f; is.vvy[b] = 0.2f - 0.05f * b; is.vw[b] = b == 0 ? 0.01f : 0.0f; }
        for (int i = 0; i < nc; ++i) {
            VC& vc = sh.u.sol.vcs[i];
            const float ang = 0.7f * (float)i + 0.3f;
            vc.nx = __cosf(ang); vc.ny = __sinf(ang);
            vc.iaI = i + 1; vc.ibI = 0; vc.mA = 1.0f; vc.iA = 0.0f; vc.mB = 0.05f; vc.iB = 1.0f / 17.0833f; vc.friction = 0.44f;
            vc.pointCount = pcount;
            if (chain) { vc.iaI = i; vc.ibI = i + 1; vc.mA = 1.0f; vc.iA = 0.05f; }
            for (int j = 0; j < 2; ++j) {
                vc.rAx[j] = 0.1f * j - 0.2f; vc.rAy[j] = 0.75f; vc.rBx[j] = 0.4f + 0.3f * j; vc.rBy[j] = -0.6f;
                vc.ni[j] = 0.2f; vc.ti[j] = 0.01f; vc.vbias[j] = 0.0f; vc.nmass[j] = 0.9f; vc.tmass[j] = 0.8f;
            }
            vc.k0 = 1.2f; vc.k1 = 0.3f; vc.k3 = 1.1f; vc.nm0 = 0.9f; vc.nm1 = -0.2f; vc.nm3 = 0.95f;
        }
    }
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    int sw = nc == 1 ? w.solver_velocity_one(is, sh.u.sol.vcs, iters, false)
                     : (nc == 2 ? w.solver_velocity_two(is, sh.u.sol.vcs, iters, false) : -1);
    if (sw < 0) w.solver_velocity_lanes(is, sh.u.sol.vcs, iters, false);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    __syncthreads();
    if (tid == 0) out[blockIdx.x] = t1 - t0 + (is.vvx[0] == 12345.0f ? 1ull : 0ull);
}
// Diagnostic micro-benchmark of the position passes (mrp_debug_posbench): a synthetic island of nc
// static-wall contacts of pcount points on one moving block (body 0), walls alternately above and
// below it, each penetrating it by ~0.1 (the squeezed shape of the slowest v0 lanes: the passes never
// reach the exit test), solved by the dispatch of the step (register paths for 1-2 contacts, the
// lanes path above); out[2 * block] = s_memtime cycles, out[2 * block + 1] = passes run.
__global__ __launch_bounds__(BLOCK, MRP_STEP_WAVES_PER_EU) void k_posbench(int nc, int pcount, int iters, unsigned long long* out) {
    using W = World<0>;
    __shared__ Shared<0> sh;
    const int tid = threadIdx.x;
    EnvParams P{};
    W w(sh, g_table, P, tid);
    auto& is = sh.isl;
    if (tid == 0) {
        is.nb = nc + 1; is.nc = nc;
        is.pcx[0] = 0.0f; is.pcy[0] = 0.0f; is.pa[0] = 0.3f; is.vvx[0] = 0.0f; is.vvy[0] = 0.0f; is.vw[0] = 0.0f;
        for (int i = 0; i < nc; ++i) {
            const float up = (i & 1) ? -1.0f : 1.0f;   // wall above (normal down) or below (normal up)
            is.pcx[i + 1] = 0.05f * (float)i; is.pcy[i + 1] = up; is.pa[i + 1] = 0.0f;
            is.vvx[i + 1] = 0.0f; is.vvy[i + 1] = 0.0f; is.vw[i + 1] = 0.0f;
            VC& vc = sh.u.sol.vcs[i];
            PC& pc = sh.u.sol.pcs[i];
            vc.iaI = i + 1; vc.ibI = 0; vc.mA = 0.0f; vc.iA = 0.0f; vc.mB = 0.05f; vc.iB = 1.0f / 17.0833f;
            vc.pointCount = pcount;
            pc.type = MT_FACEA; pc.pointCount = pcount;
            pc.lnx = 0.0f; pc.lny = -up; pc.lpx0 = 0.0f; pc.lpy0 = -0.5f * up;
            pc.lpx[0] = -0.2f; pc.lpy[0] = 0.62f * up; pc.lpx[1] = 0.2f; pc.lpy[1] = 0.6f * up;
            pc.lcAx = 0.0f; pc.lcAy = 0.0f; pc.lcBx = 0.0f; pc.lcBy = 0.0f; pc.rA = 0.01f; pc.rB = 0.01f;
        }
    }
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    int n = w.solver_position_small(is, sh.u.sol.vcs, sh.u.sol.pcs, false, -1, -1, iters);
    if (n < 0) n = w.solver_position_lanes(is, sh.u.sol.vcs, sh.u.sol.pcs, false, -1, -1, iters);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    __syncthreads();
    if (tid == 0) { out[2 * blockIdx.x] = t1 - t0 + (is.pcx[0] == 12345.0f ? 1ull : 0ull); out[2 * blockIdx.x + 1] = (unsigned long long)n; }
}
}  // namespace
hipError_t mrp::posbench_launch(const EnvTables& v0, int nc, int pcount, int iters, int blocks, unsigned long long* d_out) {
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_table), &v0, sizeof(EnvTables));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_posbench, dim3(blocks), dim3(BLOCK), 0, nullptr, nc, pcount, iters, d_out);
    return hipGetLastError();
}
hipError_t mrp::velbench_launch(const EnvTables& v0, int nc, int pcount, int iters, int blocks, unsigned long long* d_out) {
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_table), &v0, sizeof(EnvTables));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_velbench, dim3(blocks), dim3(BLOCK), 0, nullptr, nc, pcount, iters, d_out);
    return hipGetLastError();
}
