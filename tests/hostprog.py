"""Build and run a stand-alone host program (a tests/*_check.cpp with its own main) with hipcc, host side only:
no device code is built.  A support module of tests/test_packed.py, test_lane_repair.py and test_policy_layout.py."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def library_flags():
    """The library's flags, host side only."""
    from gym_puzzles_amd.build import FLAGS
    return [f for f in FLAGS if not f.startswith("--offload-arch") and f != "-fPIC"]


def build(source, exe, flags, host_flags=()):
    """Compiles tests/``source`` to ``exe``: ``flags`` go before ``-x hip --cuda-host-only`` and ``host_flags``
    behind it.  Skips the test when there is no hipcc."""
    cc = hipcc()
    if cc is None:
        pytest.skip("hipcc not available")
    subprocess.run([cc, *flags, "-x", "hip", "--cuda-host-only", *host_flags, os.path.join(HERE, source), "-o", str(exe)],
                   check=True, capture_output=True)
    return str(exe)


def run(exe, *argv):
    return subprocess.run([str(exe), *argv], capture_output=True, text=True)
