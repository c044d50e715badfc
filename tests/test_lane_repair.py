"""The contact-slot rule and the high-water-mark repair of mrp_set_state, checked on the host.

k_step moves only the contact slots below LaneState::cHW and rebuilds the others from one rule
(mrp_world.h contact_slot_init); mrp_set_state raises an understated mark with
StateIO<ENV>::repair_marks (mrp_lane.h), pure host arithmetic on the lane words.
tests/lane_repair_check.cpp runs both on hand-built lanes of the smallest layout (env 15, C = 14)
and of the granule unit's (env 2, C = 53): an all-initial lane, one non-initial word in slots 0, 1
and C - 1 of each of the 24 contact arrays, stored marks above the found one, above C and below 0,
and the rule's values. The GPU test test_set_state_repairs_understated_contact_mark checks the
same repair end to end.
"""
from __future__ import annotations

import os
import subprocess

import pytest

from test_packed import _hipcc

HERE = os.path.dirname(os.path.abspath(__file__))


def test_contact_slot_rule_and_mark_repair(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    exe = tmp_path / "lane_repair_check"
    from gym_puzzles_amd.build import FLAGS
    # the library's flags, host side only (no device code in the check)
    flags = [f for f in FLAGS if not f.startswith("--offload-arch") and f != "-fPIC"]
    subprocess.run([hipcc, *flags, "-x", "hip", "--cuda-host-only", os.path.join(HERE, "lane_repair_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    lines = dict((ln.split()[0], (int(ln.split()[1]), int(ln.split()[2])))
                 for ln in r.stdout.strip().splitlines() if not ln.startswith("#"))
    # per layout: 1 layout check, C + 2 values of the rule, 3 * 24 single-word lanes, 10 mark cases
    assert lines == {"env15": (0, 14 + 85), "env2": (0, 53 + 85)}, r.stdout
    assert r.returncode == 0
