"""swarmrl_amd/csrc/swarm_plan.h and swarm_sizes.h, the engine's path choices
and buffer sizes, as a host-only program: tests/csrc/plan_selftest.cpp includes
those two headers alone and prints what swarm::plan_engine decides for a fixed
grid of engines (both sides of every threshold, every override at unset, 0, 1
and x, every refusal), one line per row.

The lines are compared with tests/plan_rows_parent.txt.  That table was not
made by the code under test: it was printed by swarm_engine_create itself, on
an MI355X, at the commit before plan_engine existed (a temporary print of the
same fields at the end of the function, the grid driven through the C ABI;
rows it refuses before it touches the device need none).
Results are bit-identical on every path, so this comparison is the only test
that notices a threshold that slipped.  A row whose expected line changes on
purpose (a new path, a retuned threshold) is edited here by hand, with the
measurement that justifies it in DESIGN.md.

The program also asserts, without the table, the implications between the
flags, the LDS bound of every launch the plan selects and the buffer count."""

import ctypes
import os
import subprocess

from conftest import ROOT


def test_plan_rows_match_the_parent_commit(tmp_path):
    exe = tmp_path / "plan_selftest"
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I", str(ROOT / "swarmrl_amd" / "csrc"), "-o", str(exe),
                    str(ROOT / "tests" / "csrc" / "plan_selftest.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert got[-1] == "plan: ok"
    want = (ROOT / "tests" / "plan_rows_parent.txt").read_text().splitlines()
    assert len(want) == 112
    assert len(got) - 1 == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_create_refuses_bad_species_before_it_touches_the_device():
    """The two refusals of swarm_engine_create that the plan does not see: a
    null species array (with the other null arguments) and a species index
    outside [0, n_species).  Both come before the first HIP call."""
    from swarmrl_amd import _capi

    lib = _capi.lib()
    p = _capi.SwarmParams()
    p.n_dims, p.periodic, p.n_species = 2, 1, 2
    p.box[:] = [40.0, 40.0, 40.0]
    p.time_step, p.kT, p.wca_epsilon = 1e-3, 1.0, 1.0
    for s in range(2):
        p.radius[s], p.gamma_t[s], p.gamma_r[s] = 1.0, 1.0, 1.0
    out = ctypes.c_void_p(1)

    def create(species):
        return lib.swarm_engine_create(ctypes.byref(p), 1, 4, species, ctypes.byref(out))

    assert create(None) == _capi.SWARM_EINVAL
    assert lib.swarm_last_error() == b"null argument"
    for bad in (2, -1):
        assert create((ctypes.c_int32 * 4)(0, 1, bad, 0)) == _capi.SWARM_EINVAL
        assert lib.swarm_last_error() == b"species index out of range"
        assert out.value is None  # *out is cleared once the arguments are there
