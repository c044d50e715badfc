/*
 * b2_work.h -- TEST INFRASTRUCTURE ONLY.  Internal to oracle/: the solver and island types that
 * b2_oracle.c (the Box2D restatement) and b2_work.c (the work model and its diagnostics) share, the
 * device's early-exit compare schedule, and the few calls by which the restatement reports to the
 * model.  With OR_NO_WORK (the CPU-baseline builds) those calls are empty.
 */
#ifndef MRP_B2_WORK_H
#define MRP_B2_WORK_H

#include "b2_oracle.h"

/* ---------------------------------------------------------------- contact solver [B2 b2ContactSolver.h] */
typedef struct { V2 c; float a; } Position;
typedef struct { V2 v; float w; } Velocity;
typedef struct { V2 rA, rB; float normalImpulse, tangentImpulse, normalMass, tangentMass, velocityBias; } VCPoint;
typedef struct {
    VCPoint points[2]; V2 normal; float nm[4]; /* normalMass ex.x ex.y ey.x ey.y */ float K[4];
    int indexA, indexB; float invMassA, invMassB, invIA, invIB, friction, restitution, tangentSpeed;
    int pointCount, contactIndex;
} VC;
typedef struct {
    V2 localPoints[2]; V2 localNormal, localPoint; int indexA, indexB; float invMassA, invMassB;
    V2 localCenterA, localCenterB; float invIA, invIB; int type; float radiusA, radiusB; int pointCount;
} PC;
typedef struct {
    float dt, inv_dt, dtRatio; int velocityIterations, positionIterations, warmStarting;
} TimeStep;
typedef struct {
    TimeStep step; Position* positions; Velocity* velocities; Contact** contacts; int count; VC* vcs; PC* pcs;
} Solver;
typedef struct {   /* [B2 b2Island.h] */
    Body** bodies; Contact** contacts; Position* positions; Velocity* velocities;
    int bodyCount, contactCount, bodyCapacity, contactCapacity;
} Island;

/* The device's early-exit compare schedule (mrp_world.h exit_mask, EXIT_DENSE = 32 /
 * EXIT_SPARSE = 16): after sweep `done` the state is compared with the snapshot of two sweeps
 * earlier when (iters - done) & mask == 0 and snapshotted when it is 2.  One definition for the
 * sweep loop (b2_oracle.c velocity_sweeps) and the cycle models (b2_work.c). */
#define OR_EXIT_DENSE 32
#define OR_EXIT_SPARSE 16
static inline int exit_mask(int done) { return done > OR_EXIT_DENSE ? OR_EXIT_SPARSE - 1 : 3; }

/* ---------------------------------------------------------------- restatement -> work model */
#ifndef OR_NO_WORK
/* a discrete island is solved: the device runs `sweeps` of the `iters` velocity sweeps, then `passes` position passes */
void b2w_island_solved(World* w, const Island* is, const Solver* s, int sweeps, int iters, int passes);
/* a TOI island's position passes are done (only the TOI pair moved); then its velocity sweeps */
void b2w_toi_positions(OrWork* k, const Island* is, const Solver* s, int toiIndexA, int toiIndexB, int passes);
void b2w_toi_sweeps(OrWork* k, const Island* is, const Solver* s, int sweeps);
void b2w_step_done(World* w);   /* a world step is complete */
/* per-sweep state history of one island for the period scan: NULL unless b2o_period_diag or
 * b2o_model_period asks for it, else room for iters + 1 states of ns floats.  b2w_history_done
 * frees it and returns the sweep count to report (`run`: the device's, -1 = no exit). */
float* b2w_history(int ns, int iters);
int b2w_history_done(float* hist, int ns, int iters, int nc, int run);
void b2w_lcp_case(int k);   /* the 2-point block solver took case k (0-3, 4 = no solution) */

/* ---------------------------------------------------------------- switches and diagnostics of the checker
 * (exported for tools/ and tests/; each is described at its definition in b2_work.c) */
void b2o_period_diag(int on, long* out300);
void b2o_model_period(int p);
void b2o_model_2wave(const double* cost16, double x, double b);
void b2o_model_dual(double factor, int window);
int b2o_dual_schedule(int nc, const int* ia, const int* ib, const int* dyn, const int* pcount, int D, int window,
                      unsigned char* out, int cap);
void b2o_topo_diag(int on, long* sig64, long* w64);
void b2o_lcp_cases(long* out8, int reset);
#else
static inline void b2w_island_solved(World* w, const Island* is, const Solver* s, int sweeps, int iters, int passes) {}
static inline void b2w_toi_positions(OrWork* k, const Island* is, const Solver* s, int toiIndexA, int toiIndexB, int passes) {}
static inline void b2w_toi_sweeps(OrWork* k, const Island* is, const Solver* s, int sweeps) {}
static inline void b2w_step_done(World* w) {}
static inline float* b2w_history(int ns, int iters) { return 0; }
static inline int b2w_history_done(float* hist, int ns, int iters, int nc, int run) { return run; }
static inline void b2w_lcp_case(int k) {}
#endif

#endif
