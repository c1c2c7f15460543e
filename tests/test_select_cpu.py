"""swarmrl_amd/csrc/swarm_select.h, the variant selection of the host launch
layers, as a host-only program: tests/csrc/select_selftest.cpp includes that
header alone and checks that bools hands every one of the 2^k flag
combinations (k = 1..4) to the callee as the same values in the same
positions, that the cone-bin selector gives 4, 8, 16, 32 at nb = 1, 4, 5, 8, 9,
16, 17, 32, and that the sort-chunk selector switches exactly between 4096 and
4097."""

import os
import subprocess

from conftest import ROOT


def test_selectors(tmp_path):
    exe = tmp_path / "select_selftest"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I", str(ROOT / "swarmrl_amd" / "csrc"), "-o", str(exe),
                    str(ROOT / "tests" / "csrc" / "select_selftest.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "select: ok" in r.stdout
