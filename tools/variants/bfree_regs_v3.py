# A/B (round 6): v3's TOI sub-step solve is 180 sweeps of a one-contact island on the
# register path; here the branch-free block-solver selection runs on the register paths only (one- and
# two-contact islands: MRP_VEL_BFREE_REGS), the lanes path keeps the case loop.
EDITS = [("mrp_world.h", "            if constexpr (MRP_VEL_BFREE && (!MRP_VEL_BFREE_LANES || Pick::LANES)) {",
          "            if constexpr (MRP_VEL_BFREE && (MRP_VEL_BFREE_LANES ? Pick::LANES : (MRP_VEL_BFREE_REGS ? !Pick::LANES : true))) {"),
         ("mrp_world.h", "#ifndef MRP_VEL_BFREE_LANES\n", "#ifndef MRP_VEL_BFREE_REGS\n#define MRP_VEL_BFREE_REGS 0\n#endif\n#ifndef MRP_VEL_BFREE_LANES\n")]
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gym_puzzles_amd.build import UNIT_FLAGS  # noqa: E402

FLAGS = {5: list(UNIT_FLAGS[5]) + ["-DMRP_VEL_BFREE=1", "-DMRP_VEL_BFREE_REGS=1"]}
