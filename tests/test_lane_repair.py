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

import hostprog


def test_contact_slot_rule_and_mark_repair(tmp_path):
    # the library's flags, host side only (no device code in the check)
    r = hostprog.run(hostprog.build("lane_repair_check.cpp", tmp_path / "lane_repair_check", hostprog.library_flags()))
    print(r.stdout)
    lines = dict((ln.split()[0], (int(ln.split()[1]), int(ln.split()[2])))
                 for ln in r.stdout.strip().splitlines() if not ln.startswith("#"))
    # per layout: 1 layout check, C + 2 values of the rule, 3 * 24 single-word lanes, 10 mark cases
    assert lines == {"env15": (0, 14 + 85), "env2": (0, 53 + 85)}, r.stdout
    assert r.returncode == 0
