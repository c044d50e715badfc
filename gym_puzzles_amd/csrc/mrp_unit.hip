// mrp_unit.hip -- one env id's lane kernels and launch table (see mrp_lane.h, mrp_ops.h).
// build.py compiles this file once per row of the registry (mrp_config.h) with -DMRP_ENV=<id>.
#include "mrp_lane.h"
#if MRP_ENV == 0
#include "mrp_microbench.h"   // env 0's unit also carries the v0 solver micro-benchmarks
#endif

MRP_DEFINE_ENV_OPS(MRP_ENV)
