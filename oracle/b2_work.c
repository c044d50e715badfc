/*
 * b2_work.c -- TEST INFRASTRUCTURE ONLY.  The work model of the checker build (OrWork: device sweep
 * counts, dependency levels, critical paths; tools/chain_model.py, tools/roofline_model.py), the
 * two-wave and paired-update cycle models (tools/two_wave_model.py) and the diagnostics behind the
 * findings in DESIGN.md.  None of it is Box2D: b2_oracle.c reports to it through the b2w_* calls of
 * b2_work.h and never reads it back, so the CPU-baseline builds (OR_NO_WORK) carry none of it.
 */
#include "b2_work.h"

#ifndef OR_NO_WORK
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the island bodies the contacts name: 1 + the largest index */
static int bodies_used(const Solver* s) {
    int nb = 0;
    for (int i = 0; i < s->count; ++i) {
        if (s->vcs[i].indexA + 1 > nb) nb = s->vcs[i].indexA + 1;
        if (s->vcs[i].indexB + 1 > nb) nb = s->vcs[i].indexB + 1;
    }
    return nb;
}
/* dependency levels of the island's Gauss-Seidel order: contact i waits for the last earlier
 * contact that shares one of its dynamic bodies (`dyn[k]`: island body k moves under this solve);
 * returns the level count, and the sum over levels of each level's largest point count */
static int work_levels(const Solver* s, const int* dyn, int* level_points) {
    int last[256], lvmax_pts[256];
    const int nb = bodies_used(s);
    for (int k = 0; k < nb && k < 256; ++k) last[k] = 0;
    int L = 0;
    for (int i = 0; i < s->count && i < 256; ++i) {
        const int a = s->vcs[i].indexA, b = s->vcs[i].indexB;
        int lv = 1;
        if (dyn[a] && last[a] + 1 > lv) lv = last[a] + 1;
        if (dyn[b] && last[b] + 1 > lv) lv = last[b] + 1;
        if (dyn[a]) last[a] = lv;
        if (dyn[b]) last[b] = lv;
        if (lv > L) { for (int k = L; k < lv; ++k) lvmax_pts[k] = 0; L = lv; }
        if (s->pcs[i].pointCount > lvmax_pts[lv - 1]) lvmax_pts[lv - 1] = s->pcs[i].pointCount;
    }
    int lp = 0;
    for (int k = 0; k < L; ++k) lp += lvmax_pts[k];
    if (level_points) *level_points = lp;
    return L;
}
/* critical path of `reps` repetitions of the island's Gauss-Seidel order, each contact lasting
 * its point count (by_points) or 1: a contact starts when the previous contacts that share one of
 * its dynamic bodies have finished (the sweeps unrolled, so sweep k+1 may overlap sweep k) */
static long work_pipe(const Solver* s, const int* dyn, int reps, int by_points) {
    long fin[256];
    const int nb = bodies_used(s);
    for (int k = 0; k < nb && k < 256; ++k) fin[k] = 0;
    long end = 0;
    for (int r = 0; r < reps; ++r)
        for (int i = 0; i < s->count; ++i) {
            const int a = s->vcs[i].indexA, b = s->vcs[i].indexB;
            long t = 0;
            if (dyn[a] && fin[a] > t) t = fin[a];
            if (dyn[b] && fin[b] > t) t = fin[b];
            t += by_points ? s->pcs[i].pointCount : 1;
            if (dyn[a]) fin[a] = t;
            if (dyn[b]) fin[b] = t;
            if (t > end) end = t;
        }
    return end;
}
/* diagnostic (b2o_period_diag): for islands whose sweeps never reach period 1 or 2, the earliest
 * sweep at which the state repeats with ANY period up to 64, histogrammed; [0] islands examined,
 * [1] of them with no repeat within `iters`, [2 + k] first repeat at sweep k (k < 190), and the
 * period histogram at [200 + p] */
static int g_period_diag = 0;
static long g_period_hist[300];
void b2o_period_diag(int on, long* out300) {
    if (out300) for (int i = 0; i < 300; ++i) out300[i] = g_period_hist[i];
    if (on >= 0) { g_period_diag = on; for (int i = 0; i < 300; ++i) g_period_hist[i] = 0; }
}
static int g_model_period = 0;   /* > 0: the work model counts sweeps as if periods up to this were detected */
void b2o_model_period(int p) { g_model_period = p; }
static int period_scan(const float* hist, int ns, int iters) {
    int first = -1, per = 0;
    const int pmax = g_model_period > 0 ? g_model_period : 64;
    for (int k = 1; k <= iters && first < 0; ++k)
        for (int p = 1; p <= pmax && p <= k; ++p)
            if (memcmp(hist + (size_t)k * ns, hist + (size_t)(k - p) * ns, sizeof(float) * (size_t)ns) == 0) {
                first = k; per = p; break;
            }
#pragma omp critical
    {
        g_period_hist[0]++;
        if (first < 0) g_period_hist[1]++;
        else { g_period_hist[2 + (first < 190 ? first : 189)]++; g_period_hist[200 + per]++; }
    }
    return first;
}

/* the per-sweep history that velocity_sweeps (b2_oracle.c) fills for the scan while a switch asks for one */
float* b2w_history(int ns, int iters) {
    if (!g_period_diag && g_model_period <= 0) return NULL;
    return (float*)malloc(sizeof(float) * (size_t)(ns > 0 ? ns : 1) * (size_t)(iters + 1));
}
int b2w_history_done(float* hist, int ns, int iters, int nc, int run) {
    if (run < 0 && nc > 0) {
        const int first = period_scan(hist, ns, iters);
        if (g_model_period > 0 && first > 0) run = first;
    }
    free(hist);
    return run;
}

/* diagnostic (b2o_model_2wave): the island's `sweeps` velocity sweeps (device
 * count, `iters` configured) priced on one wave, and split over two waves of one workgroup.  Each
 * wave runs its contacts in the island's Gauss-Seidel order; a contact starts when its wave is free
 * and every dynamic body it touches holds the value of the body's previous update in sequential order
 * (+x cycles when that update ran on the other wave: an LDS handoff), so the split is bit-exact by
 * construction.  At each early-exit compare point the waves meet (+b).  The partition (contact 0 on
 * wave 0) is the best of all 2^(nc-1) for nc <= 12 over the first min(sweeps, 8) sweeps.
 * cost[(p - 1) * 8 + n - 1] = cycles of one p-point contact update on a wave holding n contacts (n > 8
 * priced as 8), x = cycles of one handoff, b = cycles of the joint compare; cost NULL switches it off. */
static double g2w_cost[16], g2w_x = -1.0, g2w_b = 0.0, g2w_read = 0.0, g2w_pub = 0.0;
void b2o_model_2wave(const double* cost16, double x, double b) {
    if (!cost16) { g2w_x = -1.0; return; }
    /* OR_2W_READ / OR_2W_PUB: cycles a cross-wave dependency adds to the consumer's update (its LDS
     * read of the body) and to the producer's (the LDS write + flag), waiting or not */
    g2w_read = getenv("OR_2W_READ") ? atof(getenv("OR_2W_READ")) : 0.0;
    g2w_pub = getenv("OR_2W_PUB") ? atof(getenv("OR_2W_PUB")) : 0.0;
    for (int i = 0; i < 16; ++i) g2w_cost[i] = cost16[i];
    g2w_x = x; g2w_b = b;
}
static double twowave_run(const Solver* s, const int* dyn, int nb, unsigned mask, int sweeps, int iters, int barriers) {
    double fin[256], tw[2] = {0.0, 0.0};
    int own[256], n[2] = {0, 0};
    for (int i = 0; i < s->count; ++i) ++n[(mask >> i) & 1u];
    for (int k = 0; k < nb; ++k) { fin[k] = 0.0; own[k] = -1; }
    int have = (iters & 3) == 2;
    for (int r = 0; r < sweeps; ++r) {
        for (int i = 0; i < s->count; ++i) {
            const int w = (mask >> i) & 1u, ab[2] = {s->vcs[i].indexA, s->vcs[i].indexB};
            double t = tw[w], rd = 0.0, pub = 0.0;
            for (int j = 0; j < 2; ++j)
                if (dyn[ab[j]] && own[ab[j]] >= 0) {
                    const double ready = fin[ab[j]] + (own[ab[j]] != w ? g2w_x : 0.0);
                    if (own[ab[j]] != w) rd = g2w_read;   /* the LDS read of a body the other wave wrote */
                    if (ready > t) t = ready;
                }
            for (int j = 0; j < 2 && mask; ++j)   /* publishing a body the other wave updates next */
                if (dyn[ab[j]]) {
                    int nx = -1;
                    for (int q = 1; q <= s->count && nx < 0; ++q) {
                        const int k2 = (i + q) % s->count;
                        if (s->vcs[k2].indexA == ab[j] || s->vcs[k2].indexB == ab[j]) nx = k2;
                    }
                    if (nx >= 0 && (int)((mask >> nx) & 1u) != w) pub = g2w_pub;
                }
            const int nw = n[w] < 8 ? n[w] : 8, p = s->vcs[i].pointCount < 2 ? 0 : 1;
            t += rd + pub + g2w_cost[p * 8 + nw - 1];
            tw[w] = t;
            for (int j = 0; j < 2; ++j)
                if (dyn[ab[j]]) { fin[ab[j]] = t; own[ab[j]] = w; }
        }
        if (!barriers) continue;
        const int done = r + 1, left = iters - done, m = exit_mask(done);
        if ((left & m) == 0 && have) {
            const double t = (tw[0] > tw[1] ? tw[0] : tw[1]) + g2w_b;
            tw[0] = tw[1] = t;
        }
        if ((left & m) == 2) have = 1;
    }
    return tw[0] > tw[1] ? tw[0] : tw[1];
}
/* Paired contact updates on one wave (b2o_model_dual): the island's Gauss-Seidel stream of
 * `D` sweeps (item q = sweep q / nc, contact q % nc) cut into slots of one or two updates run by one
 * instruction stream in two lanes.  Greedy, in stream order: a slot takes the first unscheduled item
 * u and the first unscheduled item v after it (at most `window` items on) with u's point count that
 * shares no dynamic body with u nor with any unscheduled item between them -- so every body and
 * every contact sees its updates in the sequential order and the result is bit-exact.  out[t] =
 * u | v << 4 (v == u: a single); returns the slot count (or -1 when `cap` is too small). */
static int g_dual_mixed = 0;   /* model only: pairs of any point counts */
int b2o_dual_schedule(int nc, const int* ia, const int* ib, const int* dyn, const int* pcount, int D, int window,
                      unsigned char* out, int cap) {
    const int n = nc * D;
    unsigned char done[2048];
    if (n > 2048 || nc > 15) return -1;
    for (int q = 0; q < n; ++q) done[q] = 0;
    int t = 0, u = 0;
#define CONFL(p, q) ((dyn[ia[(p) % nc]] && (ia[(p) % nc] == ia[(q) % nc] || ia[(p) % nc] == ib[(q) % nc])) || \
                     (dyn[ib[(p) % nc]] && (ib[(p) % nc] == ia[(q) % nc] || ib[(p) % nc] == ib[(q) % nc])))
    while (u < n) {
        done[u] = 1;
        int v = u;
        for (int q = u + 1; q < n && q <= u + window; ++q) {
            if (done[q] || (!g_dual_mixed && pcount[q % nc] != pcount[u % nc]) || CONFL(u, q)) continue;
            int ok = 1;
            for (int r = u + 1; r < q && ok; ++r)
                if (!done[r] && CONFL(r, q)) ok = 0;
            if (ok) { v = q; break; }
        }
        done[v] = 1;
        if (t >= cap) return -1;
        out[t++] = (unsigned char)((u % nc) | ((v % nc) << 4));
        while (u < n && done[u]) ++u;
    }
#undef CONFL
    return t;
}
static double g_dual_factor = 0.0;
static int g_dual_window = 0, g_dual_nodrain = 0;
/* window < 0: |window|, and the stream never drains (the bound without early-exit meeting points) */
void b2o_model_dual(double factor, int window) {
    g_dual_factor = factor; g_dual_window = window < 0 ? -window : window; g_dual_nodrain = window < 0;
    g_dual_mixed = getenv("OR_DUAL_MIXED") != NULL;
}
/* the sweeps as the paired path would run them: segments between the early-exit events (snapshot
 * and compare sweeps, where the stream drains), each slot priced as one update x factor */
static double dual_run(const Solver* s, const int* dyn, int sweeps, int iters) {
    const int nc = s->count;
    int ia[16], ib[16], pc[16];
    for (int i = 0; i < nc; ++i) { ia[i] = s->vcs[i].indexA; ib[i] = s->vcs[i].indexB; pc[i] = s->vcs[i].pointCount; }
    unsigned char sl[2048];
    double t = 0.0;
    int k = 0;
    while (k < sweeps) {
        int e = g_dual_nodrain ? sweeps : k + 1;   /* next event sweep (or the end) */
        while (e < sweeps) {
            const int left = iters - e, m = exit_mask(e);
            if ((left & m) == 0 || (left & m) == 2) break;
            ++e;
        }
        const int D = e - k;
        const int ns = b2o_dual_schedule(nc, ia, ib, dyn, pc, D, g_dual_window, sl, 2048);
        if (ns < 0) return -1.0;
        for (int q = 0; q < ns; ++q) {
            const int u = sl[q] & 15, p = pc[u] < 2 ? 0 : 1;
            t += g2w_cost[p * 8 + (nc < 8 ? nc : 8) - 1] * g_dual_factor;
        }
        k = e;
    }
    return t;
}
static void work_model_2wave(const Solver* s, const int* dyn, int sweeps, int iters, OrWork* k) {
    if (g2w_x < 0.0 || s->count < 1) return;
    if (g_dual_factor > 0.0) {   /* b2o_model_dual: vel_2wave holds the paired one-wave path */
        const double one = twowave_run(s, dyn, 256, 0u, sweeps, iters, 0);
        double d = s->count >= 3 && s->count <= 15 ? dual_run(s, dyn, sweeps, iters) : one;
        if (d < 0.0) d = one;
        k->vel_1wave += (long)(one + 0.5);
        k->vel_2wave += (long)(d + 0.5);
        return;
    }
    const int nb = bodies_used(s);
    if (nb > 256) return;
    const double one = twowave_run(s, dyn, nb, 0u, sweeps, iters, 0);
    double two = one;
    if (s->count >= 2 && s->count <= 12) {
        unsigned best = 0u;
        double bt = 0.0;
        const int probe = sweeps < 8 ? sweeps : 8;
        for (unsigned m = 0; m < (1u << (s->count - 1)); ++m) {
            const unsigned mask = m << 1;   /* contact 0 stays on wave 0 */
            const double t = twowave_run(s, dyn, nb, mask, probe, iters, 0);
            if (m == 0 || t < bt) { bt = t; best = mask; }
        }
        two = twowave_run(s, dyn, nb, best, sweeps, iters, 1);
        if (best == 0u || two > one) two = one;   /* a split that does not pay stays on one wave */
    }
    k->vel_1wave += (long)(one + 0.5);
    k->vel_2wave += (long)(two + 0.5);
}

/* diagnostic (b2o_topo_diag(1); b2o_topo_diag(2) also records 1- and 2-contact islands): island
 * topologies of 3- and 4-contact islands, weighted by sweeps run:
 * per contact (A slot, B slot, point count) with body slots numbered by first appearance and static
 * bodies as slot 7; 64 distinct signatures kept */
static int g_topo_diag = 0;
static long g_topo_sig[64], g_topo_w[64];
static void topo_record(const Solver* s, const Island* is, int sweeps) {
    int slot[256], ns = 0;
    for (int k = 0; k < 256; ++k) slot[k] = -1;
    long sig = s->count;
    for (int i = 0; i < s->count; ++i) {
        const int ab[2] = {s->vcs[i].indexA, s->vcs[i].indexB};
        int sl[2];
        for (int j = 0; j < 2; ++j) {
            const Body* b = is->bodies[ab[j]];
            if (b->invMass == 0.0f && b->invI == 0.0f) { sl[j] = 7; continue; }
            if (slot[ab[j]] < 0) slot[ab[j]] = ns++;
            sl[j] = slot[ab[j]];
        }
        sig = sig * 1000 + sl[0] * 100 + sl[1] * 10 + s->vcs[i].pointCount;
    }
#pragma omp critical
    {
        int k = 0;
        while (k < 64 && g_topo_w[k] && g_topo_sig[k] != sig) ++k;
        if (k < 64) { g_topo_sig[k] = sig; g_topo_w[k] += sweeps * (long)s->count; }
    }
}
/* b2o_topo_diag(3): print (stderr, first 60) the contact list of islands with >= 5 contacts that run
 * >= 100 sweeps: per contact "A-B/points", body slots by first appearance, static bodies as S */
static int g_topo_printed = 0;
static void topo_print(const Solver* s, const Island* is, int sweeps) {
    char buf[512];
    int slot[256], ns = 0, n = 0;
    for (int k = 0; k < 256; ++k) slot[k] = -1;
    n += snprintf(buf + n, sizeof(buf) - n, "nc %d sweeps %3d:", s->count, sweeps);
    for (int i = 0; i < s->count && n < 480; ++i) {
        const int ab[2] = {s->vcs[i].indexA, s->vcs[i].indexB};
        char c[2];
        for (int j = 0; j < 2; ++j) {
            const Body* b = is->bodies[ab[j]];
            if (b->invMass == 0.0f && b->invI == 0.0f) { c[j] = 'S'; continue; }
            if (slot[ab[j]] < 0) slot[ab[j]] = ns++;
            c[j] = (char)('0' + slot[ab[j]]);
        }
        n += snprintf(buf + n, sizeof(buf) - n, " %c-%c/%d", c[0], c[1], s->vcs[i].pointCount);
    }
#pragma omp critical
    {
        if (g_topo_printed < 100000) { fprintf(stderr, "%s\n", buf); ++g_topo_printed; }
    }
}
void b2o_topo_diag(int on, long* sig64, long* w64) {
    g_topo_printed = 0;
    for (int k = 0; k < 64; ++k) { if (sig64) sig64[k] = g_topo_sig[k]; if (w64) w64[k] = g_topo_w[k]; }
    if (on >= 0) { g_topo_diag = on; for (int k = 0; k < 64; ++k) { g_topo_sig[k] = 0; g_topo_w[k] = 0; } }
}

/* diagnostic (b2o_lcp_cases): how often each case of the 2-point block solver applies (cases 1-4,
 * then "no solution"), counted over every 2-point velocity update since the last reset (slots 5-7
 * stay 0); reported by the sweep loop's solver_solve_velocity, one atomic add per update */
static long g_lcp[8];
void b2w_lcp_case(int k) { _Pragma("omp atomic") g_lcp[k]++; }
void b2o_lcp_cases(long* out8, int reset) {
    for (int k = 0; k < 8; ++k) { if (out8) out8[k] = g_lcp[k]; if (reset) g_lcp[k] = 0; }
}

/* ---- what the restatement reports (b2_work.h) ---- */
static void dynamic_bodies(const Island* is, int* dyn) {
    for (int k = 0; k < is->bodyCount && k < 256; ++k) dyn[k] = is->bodies[k]->invMass > 0.0f || is->bodies[k]->invI > 0.0f;
}
void b2w_island_solved(World* w, const Island* is, const Solver* s, int sweeps, int iters, int passes) {
    if (g_topo_diag && g_topo_diag < 3 && is->contactCount >= (g_topo_diag > 1 ? 1 : 3) && is->contactCount <= 4) topo_record(s, is, sweeps);
    if (g_topo_diag == 3 && is->contactCount >= 5 && sweeps >= 100) topo_print(s, is, sweeps);
    if (is->contactCount <= 0) return;
    int dyn[256], lp = 0, pts = 0, n1 = 0, n2 = 0;
    dynamic_bodies(is, dyn);
    const int L = work_levels(s, dyn, &lp);
    for (int i = 0; i < s->count; ++i) { pts += s->pcs[i].pointCount; if (s->vcs[i].pointCount == 2) ++n2; else ++n1; }
    OrWork* k = &w->work;
    k->islands += 1; k->vel_sweeps += sweeps;
    k->vel_upd1 += (long)sweeps * n1; k->vel_upd2 += (long)sweeps * n2; k->vel_levels += (long)sweeps * L;
    k->pos_passes += passes; k->pos_points += (long)passes * pts; k->pos_level_points += (long)passes * lp;
    k->vel_pipe += work_pipe(s, dyn, sweeps, 0);
    k->pos_pipe += work_pipe(s, dyn, passes, 1);
    work_model_2wave(s, dyn, sweeps, iters, k);
    const long units = (long)sweeps * s->count + (long)passes * pts;
    k->isl_units += units;
    w->stepIslSum += units;
    if (units > w->stepIslMax) w->stepIslMax = units;
}
void b2w_toi_positions(OrWork* k, const Island* is, const Solver* s, int toiIndexA, int toiIndexB, int passes) {
    int dyn[256], lp = 0, pts = 0;
    for (int q = 0; q < is->bodyCount && q < 256; ++q) dyn[q] = q == toiIndexA || q == toiIndexB;
    work_levels(s, dyn, &lp);
    for (int i = 0; i < s->count; ++i) pts += s->pcs[i].pointCount;
    k->toi_pos_points += (long)passes * pts; k->toi_pos_level_points += (long)passes * lp;
    k->pos_pipe += work_pipe(s, dyn, passes, 1);
}
void b2w_toi_sweeps(OrWork* k, const Island* is, const Solver* s, int sweeps) {
    int dyn[256];
    dynamic_bodies(is, dyn);
    const int L = work_levels(s, dyn, NULL);
    k->toi_vel_upd += (long)sweeps * s->count; k->toi_vel_levels += (long)sweeps * L;
    k->vel_pipe += work_pipe(s, dyn, sweeps, 0);
}
/* what solving the step's independent islands concurrently would take off the chain */
void b2w_step_done(World* w) {
    w->work.isl_concurrent_save += w->stepIslSum - w->stepIslMax;
    w->stepIslSum = 0; w->stepIslMax = 0;
}
#endif
