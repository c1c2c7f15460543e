"""swarmrl_amd/csrc/swarm_pack.h, the packing contract between the cluster
builds and the run kernels, as a host-only program:
tests/csrc/pack_selftest.cpp includes that header alone, restates the builds'
64-lane layout step as a serial prefix sum and places every cluster of random
and worst-case cluster multisets (1 to 4096 particles, plain and one-pass
classes, singleton fill off and on) with pack_base.  Checked: a cluster's
lanes lie in one wave, no two clusters share a slot, no wave is empty, the
waves stay within slots_per_env, the free tail lanes take the singletons
first, free_class agrees with a linear search, and the wave pair word, the
big-cluster pair word and the class word round-trip over their fields."""

import os
import subprocess

from conftest import ROOT


def test_packing_contract(tmp_path):
    exe = tmp_path / "pack_selftest"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I", str(ROOT / "swarmrl_amd" / "csrc"), "-o", str(exe),
                    str(ROOT / "tests" / "csrc" / "pack_selftest.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "pack: ok" in r.stdout
