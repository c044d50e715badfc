"""The packed-pair identities of the solver cores (mrp_math.h, P2), checked on the host.

The velocity and position cores issue the two halves of each b2Vec2 operation as one
v_pk_mul_f32 / v_pk_add_f32. The arms are stored as perps, the tangent is formed from the
normal, and rotations are (c, s) pairs. tests/packed_check.cpp compares every packed form with
the scalar V2 form it replaces, bit for bit, on 2 M random finite inputs per identity, including
signed zeros and subnormals. It is built with hipcc and the library's numerics flags. The GPU
tests check the same claim end to end: trajectories bitwise equal to the oracle.
"""
from __future__ import annotations

import hostprog


def test_packed_pair_identities(tmp_path):
    # the library's numerics flags, host side only (no device code in the check)
    r = hostprog.run(hostprog.build("packed_check.cpp", tmp_path / "packed_check", hostprog.library_flags()))
    lines = dict((ln.split()[0], (int(ln.split()[1]), int(ln.split()[2]))) for ln in r.stdout.strip().splitlines())
    assert set(lines) == {"cross_sv", "cross", "cross_from_perp", "dot", "mul_rv", "tangent", "v_minus_mP", "v_plus_mP"}
    for name, (bad, n) in lines.items():
        assert n == 2000000 and bad == 0, f"{name}: {bad} of {n} packed results differ from the scalar form"
    assert r.returncode == 0
