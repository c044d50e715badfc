// mrp_pixels.h -- pixel observations: the next frame stack of every lane in one launch
// ('image' obs_type of the reference, multi_robot_puzzle_00.py:148-162,197-200).  Included by
// mrp_render.h, whose display list (Prim, add_*, xf_point) and rasteriser (hit) it reuses.
//
// Per lane the output is `depth` slots of H*W*C bytes, oldest first, newest last (the
// reference stacks its frames vertically, so a lane's block read as [depth*H][W][C] is the
// observation).  Slot k < depth-1 is slot k+1 of the previous stack, or zero for a fresh episode
// (no previous stack, or the lane's done byte set: the reference starts from np.zeros, :200, and
// under auto-reset the lane state is already the new episode's first state); slot depth-1 is the
// frame of the lane's current state, shaded exactly as k_render shades it.  C = 3 stores R, G, B;
// C = 1 stores the integer luma (77 R + 150 G + 29 B + 128) >> 8 (gym_puzzles_amd/pixels.py).
//
// Where k_render builds the display list on thread 0, the first wave builds it here one
// primitive per thread: which (body, fixture, vertex) primitive i draws depends only on the env's
// tables, so every thread walks the same short enumeration (scene_slot, uniform control flow) and
// then builds its own entry with the helpers build_scene uses.
#pragma once

namespace mrpr {

constexpr int PBLOCK = PIX_BLOCK;    // threads per workgroup (4 waves; the first builds the scene)
constexpr int PCHUNK = PIX_CHUNK;    // pixels of one workgroup; larger frames are split over gridDim.y
static_assert(MAXPRIM <= BLOCK, "one wave builds the display list, one primitive per thread");

// what a display-list entry draws (the branches of build_scene, in its order)
enum : int { S_NONE = -1, S_BORDER, S_GOAL_DOT, S_GOAL_RING, S_WALL, S_BLOCK, S_BLOCK_DISC, S_BLOCK_VERT, S_AGENT, S_AGENT_DISC, S_FINAL };
struct Slot { int kind, b, f, i; uint32_t rgb; };   // body, fixture (or border side), vertex

// Entry `want` of build_scene's display list; returns the length of the list.
template <int ENV>
__device__ __forceinline__ int scene_slot(const EnvTables& T, int want, Slot& s) {
    using D = Dims<ENV>;
    constexpr int NB = D::NB, ND = D::NA + D::NB;
    const uint32_t white = rgb8(255, 255, 255), grey = rgb8(128, 128, 128), wall = rgb8(51, 51, 51), blue = rgb8(58, 153, 255);
    int n = 0;
    auto at = [&](int kind, int b, int f, int i, uint32_t rgb) {
        if (n == want) { s.kind = kind; s.b = b; s.f = f; s.i = i; s.rgb = rgb; }
        ++n;
    };
    if (D::V == 0) {
        for (int k = 0; k < 4; ++k) at(S_BORDER, 0, k, 0, wall);
    } else if (D::V == 2) {
        for (int b = 0; b < NB; ++b) { at(S_GOAL_DOT, b, 0, 0, white); at(S_GOAL_RING, b, 0, 0, wall); }
    }
    for (int b = ND; b < ND + 4; ++b)
        for (int k = T.body_nfix[b] - 1; k >= 0; --k) at(S_WALL, b, T.body_fix0[b] + k, 0, wall);
    for (int b = 0; b < NB; ++b) {
        for (int k = T.body_nfix[b] - 1; k >= 0; --k) at(S_BLOCK, b, T.body_fix0[b] + k, 0, grey);
        at(S_BLOCK_DISC, b, 0, 0, white);
        for (int k = T.body_nfix[b] - 1; k >= 0; --k) {
            const int f = T.body_fix0[b] + k, cnt = T.shape[f].count;
            for (int i = 0; i < cnt; ++i) at(S_BLOCK_VERT, b, f, i, white);
        }
    }
    for (int b = NB; b < ND; ++b) {
        for (int k = T.body_nfix[b] - 1; k >= 0; --k) at(S_AGENT, b, T.body_fix0[b] + k, 0, k > 0 ? grey : white);
        at(S_AGENT_DISC, b, 0, 0, grey);
    }
    if (D::V != 2) at(S_FINAL, 0, 0, 0, blue);
    return n;
}

// build_scene's unfilled circle (it has no helper there: the v2 final-point ring, linewidth 5)
__device__ inline void add_ring(Prim* P, int& n, float fx, float fy, const RenderArgs& A, uint32_t rgb) {
    #pragma clang fp contract(off)
    if (n >= MAXPRIM) return;
    Prim& q = P[n++];
    const float h = 2.5f * A.lw_unit, ri = A.ring_r - h, ro = A.ring_r + h;
    q.type = P_RING; q.rgb = rgb; q.a = fx; q.b = fy; q.c = ri * ri; q.d = ro * ro; q.nv = 0;
    q.bx0 = fx - ro - BPAD; q.bx1 = fx + ro + BPAD; q.by0 = fy - ro - BPAD; q.by1 = fy + ro + BPAD;
}

// P[at] <- the entry `s` describes, with build_scene's arguments for it
template <int ENV>
__device__ __forceinline__ void build_slot(const LaneState<ENV>& S, const EnvTables& T, const RenderArgs& A, const Slot& s, Prim* P, int at) {
    #pragma clang fp contract(off)
    using D = Dims<ENV>;
    constexpr int ND = D::NA + D::NB;
    const float lg = D::V == 2 ? 0.015f : 0.16f, sm = D::V == 2 ? 0.0075f : 0.08f;
    int n = at;
    const int b = s.b;
    switch (s.kind) {
    case S_BORDER: {
        const float h = 1.5f * A.lw_unit, W = 640.0f / 30.0f, H = 480.0f / 30.0f;
        if (s.f == 0) add_rect(P, n, 1.0f - h, 1.0f - h, W - 1.0f + h, 1.0f + h, s.rgb);
        else if (s.f == 1) add_rect(P, n, W - 1.0f - h, 1.0f - h, W - 1.0f + h, H - 1.0f + h, s.rgb);
        else if (s.f == 2) add_rect(P, n, 1.0f - h, H - 1.0f - h, W - 1.0f + h, H - 1.0f + h, s.rgb);
        else add_rect(P, n, 1.0f - h, 1.0f - h, 1.0f + h, H - 1.0f + h, s.rgb);
        break;
    }
    case S_GOAL_DOT: case S_GOAL_RING: case S_FINAL: {
        const float fx = (float)(S.goal[b][0] * A.goal_scale), fy = (float)(S.goal[b][1] * A.goal_scale);
        if (s.kind == S_GOAL_DOT) add_circle(P, n, fx, fy, 0.0075f, s.rgb);
        else if (s.kind == S_GOAL_RING) add_ring(P, n, fx, fy, A, s.rgb);
        else add_circle(P, n, fx, fy, 25.0f / 30.0f, s.rgb);
        break;
    }
    case S_WALL: add_poly<ENV>(P, n, T, s.f, T.wall_px[b - ND], T.wall_py[b - ND], 0.0f, 1.0f, s.rgb); break;
    case S_BLOCK: case S_AGENT: add_poly<ENV>(P, n, T, s.f, S.xpx[b], S.xpy[b], S.xs[b], S.xc[b], s.rgb); break;
    case S_BLOCK_DISC: add_circle(P, n, S.cx[b], S.cy[b], lg, s.rgb); break;
    case S_BLOCK_VERT: {
        float x, y;
        xf_point(S.xpx[b], S.xpy[b], S.xs[b], S.xc[b], T.shape[s.f].v[s.i].x, T.shape[s.f].v[s.i].y, x, y);
        add_circle(P, n, x, y, sm, s.rgb);
        break;
    }
    case S_AGENT_DISC: add_circle(P, n, S.xpx[b], S.xpy[b], lg, s.rgb); break;
    default: break;
    }
}

typedef uint32_t __attribute__((__may_alias__)) pword_t;
typedef uint4 __attribute__((__may_alias__)) pquad_t;

// Thread g of `stride` copies its share of len bytes (src NULL: zeroes) in units of U where dst and
// src agree modulo sizeof(U); the bytes before the first and after the last whole unit move singly.
template <typename U>
__device__ __forceinline__ void move_units(uint8_t* dst, const uint8_t* src, size_t len, int g, int stride) {
    const size_t mis = (size_t)((0 - (uintptr_t)dst) & (sizeof(U) - 1));
    const size_t head = mis < len ? mis : len, nu = (len - head) / sizeof(U), tail = head + nu * sizeof(U);
    U* d = reinterpret_cast<U*>(dst + head);
    const U* s = src ? reinterpret_cast<const U*>(src + head) : nullptr;
    for (size_t i = (size_t)g; i < nu; i += (size_t)stride) d[i] = src ? s[i] : U{};
    const size_t ends = head + (len - tail);   // < 2 * sizeof(U)
    if ((size_t)g < ends) {
        const size_t k = (size_t)g < head ? (size_t)g : tail + ((size_t)g - head);
        dst[k] = src ? src[k] : (uint8_t)0;
    }
}
__device__ __forceinline__ void move_bytes(uint8_t* dst, const uint8_t* src, size_t len, int g, int stride) {
    const unsigned rel = src ? (unsigned)(((uintptr_t)dst ^ (uintptr_t)src) & 15) : 0u;
    if (rel == 0) move_units<pquad_t>(dst, src, len, g, stride);
    else if ((rel & 3) == 0) move_units<pword_t>(dst, src, len, g, stride);
    else
        for (size_t i = (size_t)g; i < len; i += (size_t)stride) dst[i] = src[i];
}

// k_render's pixel-centre mapping: row r from the top, and pixel `pix` (row-major from the top left), -> world
__device__ __forceinline__ float row_y(int r, int H, const RenderArgs& A) {
    #pragma clang fp contract(off)
    return ((float)(H - 1 - r) + 0.5f) * A.sy;
}
__device__ __forceinline__ void centre(int pix, int W, int H, const RenderArgs& A, float& x, float& y) {
    #pragma clang fp contract(off)
    const int r = pix / W, c = pix - r * W;
    x = ((float)c + 0.5f) * A.sx;
    y = row_y(r, H, A);
}
// colour of one pixel: k_render's walk (the last primitive drawn that contains the centre wins)
__device__ __forceinline__ uint32_t shade(const Prim* P, int np, int pix, int W, int H, const RenderArgs& A) {
    float x, y;
    centre(pix, W, H, A, x, y);
    for (int i = np - 1; i >= 0; --i)
        if (hit(P[i], x, y)) return P[i].rgb;
    return 0u;   // background: black
}
// The same walk for four consecutive pixels at once, each primitive read once for the four, over the
// primitives of `live` only (bit i: primitive i; from the top bit down, the walk's order).  The caller
// leaves out of `live` only primitives that hit() refuses for every pixel of the wave, so the colours
// are those of the one-pixel walk.
__device__ __forceinline__ void shade4(const Prim* P, unsigned long long live, int p0, int W, int H, const RenderArgs& A,
                                       uint32_t (&v)[4]) {
    #pragma clang fp contract(off)
    float x[4], y[4];
    int r = p0 / W, c = p0 - r * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[j] = ((float)c + 0.5f) * A.sx; y[j] = row_y(r, H, A);
        v[j] = 0u;   // background: black
        if (++c == W) { c = 0; ++r; }
    }
    unsigned open = 15u;   // bit j: pixel j has no colour yet
    while (live && open) {
        const int i = 63 - __builtin_clzll(live);
        live &= ~(1ull << i);
        const Prim& q = P[i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((open >> j & 1u) && hit(q, x[j], y[j])) { v[j] = q.rgb; open &= ~(1u << j); }
    }
}
__device__ __forceinline__ uint32_t luma(uint32_t rgb) {
    return (77u * (rgb & 255u) + 150u * ((rgb >> 8) & 255u) + 29u * (rgb >> 16) + 128u) >> 8;
}

// grid: (n_lanes, ceil(W*H / PCHUNK)): one workgroup per lane for frames of up to PCHUNK pixels (the
// observation sizes); a larger frame's pixels and slot bytes are dealt over the gridDim.y workgroups
// of its lane, each with its own copy of the display list.  The first wave builds the list while the
// other waves already move the older slots; after the barrier every thread shades groups of four
// consecutive pixels (PBLOCK groups apart, after a wave-wide cull of the list against the rows of the
// wave's 256 pixels) and stores each group as one dword (C = 1) or three (C = 3).  The groups start
// at the first pixel whose byte address is dword-aligned, so at most three pixels at either end of
// the frame are stored bytewise, whatever the sizes and the lane's offset.
template <int ENV>
__global__ __launch_bounds__(PBLOCK) void k_pixels(const uint32_t* __restrict__ state, int n_lanes, int W, int H, int C, int depth,
                                                   RenderArgs A, const uint8_t* __restrict__ done, const uint8_t* prev, uint8_t* next) {
    #pragma clang fp contract(off)
    __shared__ Prim P[MAXPRIM];
    __shared__ int np;
    const int lane = blockIdx.x, tid = threadIdx.x;
    if (lane >= n_lanes) return;
    const int g = blockIdx.y * PBLOCK + tid, stride = gridDim.y * PBLOCK;
    if (tid < MAXPRIM) {
        const LaneState<ENV>& S = *reinterpret_cast<const LaneState<ENV>*>(state + (size_t)lane * lane_words<ENV>());
        Slot s;
        s.kind = S_NONE;
        const int n = scene_slot<ENV>(g_table, tid, s);
        build_slot<ENV>(S, g_table, A, s, P, tid);
        if (tid == 0) np = n < MAXPRIM ? n : MAXPRIM;
    }
    const int NP = W * H;
    const size_t slot = (size_t)NP * C;
    uint8_t* dst = next + (size_t)lane * depth * slot;
    if (depth > 1) {
        const bool fresh = !prev || (done && done[lane]);
        move_bytes(dst, fresh ? nullptr : prev + (size_t)lane * depth * slot + slot, (size_t)(depth - 1) * slot, g, stride);
    }
    __syncthreads();
    uint8_t* o = dst + (size_t)(depth - 1) * slot;
    // the first pixel whose byte address o + C * head is dword-aligned (3 is its own inverse modulo 4)
    const int a = (int)((uintptr_t)o & 3), mis = C == 1 ? (4 - a) & 3 : a;
    const int head = mis < NP ? mis : NP, ng = (NP - head) / 4, tail = head + 4 * ng;
    // A wave's BLOCK groups of one trip are consecutive pixels, a band of a few rows.  Its threads
    // first cull the display list against that band in parallel, thread i looking at primitive i: one
    // whose padded box lies wholly above or below the band's pixel centres is refused by hit() for
    // every pixel of the wave, on the same two comparisons.  The ballot of the rest is the list the
    // wave walks.  The whole wave takes every trip (the ballot needs all its threads); a thread
    // without a group of its own in the last trip shades the frame's last group again and stores nothing.
    const int wl = tid & (BLOCK - 1);
    for (int qw = g - wl; qw < ng; qw += stride) {
        const int q = qw + wl;
        const bool mine = q < ng;
        const int p0 = head + 4 * (mine ? q : ng - 1);
        const int plo = head + 4 * qw, last = plo + 4 * BLOCK - 1, phi = last < NP ? last : NP - 1;
        const float ytop = row_y(plo / W, H, A), ybot = row_y(phi / W, H, A);
        const bool in_band = wl < np && !(ytop < P[wl].by0 || ybot > P[wl].by1);
        uint32_t v[4];
        shade4(P, __builtin_amdgcn_ballot_w64(in_band), p0, W, H, A, v);
        if (!mine) continue;
        if (C == 1) {
            *reinterpret_cast<pword_t*>(o + p0) = luma(v[0]) | (luma(v[1]) << 8) | (luma(v[2]) << 16) | (luma(v[3]) << 24);
        } else {   // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            pword_t* w = reinterpret_cast<pword_t*>(o + (size_t)p0 * 3);
            w[0] = v[0] | (v[1] << 24);
            w[1] = (v[1] >> 8) | (v[2] << 16);
            w[2] = (v[2] >> 16) | (v[3] << 8);
        }
    }
    if (g < head + (NP - tail)) {
        const int pix = g < head ? g : tail + (g - head);
        const uint32_t rgb = shade(P, np, pix, W, H, A);
        if (C == 1) {
            o[pix] = (uint8_t)luma(rgb);
        } else {
            uint8_t* b = o + (size_t)pix * 3;
            b[0] = (uint8_t)(rgb & 255); b[1] = (uint8_t)((rgb >> 8) & 255); b[2] = (uint8_t)(rgb >> 16);
        }
    }
}

}  // namespace mrpr
