"""
ctypes wrapper of the Langevin restatement (tests/csrc/langevin_oracle.c),
TEST INFRASTRUCTURE ONLY.  The library is built by ``__graft_entry__.build()``
into tests/csrc/liblangevinoracle.so; when it is missing it is built here,
with the CPU oracle's compiler flags (-ffp-contract=off: every fp32 operation
rounded on its own).
"""

from __future__ import annotations

import ctypes
import os
import pathlib
import subprocess

import numpy as np

from oracle import oracle

_DIR = pathlib.Path(__file__).resolve().parent / "csrc"
SRC = _DIR / "langevin_oracle.c"
LIB_PATH = _DIR / "liblangevinoracle.so"
# oracle/Makefile's CFLAGS
CFLAGS = ["-O3", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-fast-math",
          "-fopenmp"]
_P = ctypes.c_void_p


def build() -> pathlib.Path:
    import fcntl

    with open(_DIR / ".langevin_build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        tmp = LIB_PATH.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", str(tmp), str(SRC),
                        "-lm"], check=True)
        os.replace(tmp, LIB_PATH)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            build()
        L = ctypes.CDLL(str(LIB_PATH))
        pp = ctypes.POINTER(oracle.Params)
        ci, cd = ctypes.c_int, ctypes.c_double
        L.or_flow_sample.restype = None
        L.or_flow_sample.argtypes = [_P, ci, ci, ci, _P, _P]
        L.or_lv_run.restype = ci
        L.or_lv_run.argtypes = [pp, ci, _P, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_uint64, ci,
                                ctypes.c_uint32, _P, ci, _P, _P, _P, _P, _P, ci, ci, _P, _P, ci,
                                ci, cd, _P]
        L.or_lv_sd_run.restype = ci
        L.or_lv_sd_run.argtypes = [pp, ci, _P, _P, _P, _P, _P, _P, _P, ci, cd, cd, _P, ci, _P, ci,
                                   ci, _P, _P, ci, ci, cd]
        _lib = L
    return _lib


_ptr = oracle._ptr


def flow_sample(u, q):
    """u (nx, ny, 1, 3) fp32, q [3, n] uint32 box fractions -> (2, n) fp32."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    assert u.ndim == 4 and u.shape[2] == 1 and u.shape[3] == 3
    q = np.ascontiguousarray(q, dtype=np.uint32)
    n = q.shape[1]
    out = np.zeros((2, n), np.float32)
    lib().or_flow_sample(_ptr(u), u.shape[0], u.shape[1], n, _ptr(q), _ptr(out))
    return out


def _fields(potential, flow):
    """potential: None or (phi (nx, ny, 1), h [3]); flow: None or
    (u (nx, ny, 1, 3), gamma).  Returns the C arguments and what keeps them
    alive."""
    phi = ph = u = None
    pn, un, gam = (0, 0), (0, 0), 0.0
    if potential is not None:
        phi = np.ascontiguousarray(potential[0], dtype=np.float32)
        assert phi.ndim == 3 and phi.shape[2] == 1
        ph = np.ascontiguousarray(potential[1], dtype=np.float64)
        pn = phi.shape[:2]
    if flow is not None:
        u = np.ascontiguousarray(flow[0], dtype=np.float32)
        assert u.ndim == 4 and u.shape[2] == 1 and u.shape[3] == 3
        un, gam = u.shape[:2], float(flow[1])
    return phi, pn, ph, u, un, gam


def _walls(walls):
    if not walls:
        return None, 0
    return oracle.make_walls(walls)


def lv_run(params, state, vel, omega, species, f_swim, torque_z, n_steps, step0=0, env=0,
           f_ext=None, walls=None, prev=None, potential=None, flow=None):
    """n_steps Langevin sub-steps of one env.  state: {"q", "img", "ang"};
    vel [3, n], omega [n] fp32.  Returns (state, vel, omega, info) with
    info = {"pairs" (ordered pairs in range, summed over the sub-steps),
    "violations"}.  prev: as oracle.bd_run (reuse_forces)."""
    st = oracle._copy_state(state)
    n = st["ang"].shape[0]
    v = np.array(vel, dtype=np.float32, order="C", copy=True).reshape(3, n)
    w = np.array(omega, dtype=np.float32, order="C", copy=True).reshape(n)
    sp = np.ascontiguousarray(species, dtype=np.uint8)
    fs = np.ascontiguousarray(f_swim, dtype=np.float32)
    tz = np.ascontiguousarray(torque_z, dtype=np.float32)
    fe = None if f_ext is None else np.ascontiguousarray(f_ext, dtype=np.float32)
    f0 = t0 = a0 = None
    if prev is not None:
        f0 = np.ascontiguousarray(prev["f"], dtype=np.float32)
        t0 = np.ascontiguousarray(prev["t"], dtype=np.float32)
        a0 = np.ascontiguousarray(prev["ang"], dtype=np.uint32)
    warr, nw = _walls(walls)
    phi, pn, ph, u, un, gam = _fields(potential, flow)
    viol = np.zeros(1, np.uint64)
    stats = np.zeros(1, np.int64)
    rc = lib().or_lv_run(ctypes.byref(params), n, _ptr(st["q"]), _ptr(st["img"]), _ptr(st["ang"]),
                         _ptr(v), _ptr(w), _ptr(sp), _ptr(fs), _ptr(tz), _ptr(fe), int(step0),
                         int(n_steps), int(env),
                         None if warr is None else ctypes.cast(warr, _P), nw, _ptr(viol),
                         _ptr(f0), _ptr(t0), _ptr(a0), _ptr(phi), int(pn[0]), int(pn[1]),
                         _ptr(ph), _ptr(u), int(un[0]), int(un[1]), gam, _ptr(stats))
    if rc != 0:
        raise ValueError(f"or_lv_run failed ({rc})")
    return st, v, w, {"pairs": int(stats[0]), "violations": int(viol[0])}


class ReuseForces:
    """oracle.ReuseForces for an env under the Langevin thermostat."""

    def __init__(self, state):
        n = state["q"].shape[1]
        self.prev = {"f": np.zeros(n, np.float32), "t": np.zeros(n, np.float32),
                     "ang": np.asarray(state["ang"], np.uint32).copy()}

    def run(self, params, state, vel, omega, species, f_swim, torque, n_steps, **kw):
        out = lv_run(params, state, vel, omega, species, f_swim, torque, n_steps, prev=self.prev,
                     **kw)
        self.prev = {"f": np.asarray(f_swim, np.float32).copy(),
                     "t": np.asarray(torque, np.float32).copy(), "ang": out[0]["ang"].copy()}
        return out


def sd_run(params, state, species, n_steps, gamma=0.1, max_disp=0.1, f_ext=None, walls=None,
           potential=None, flow=None):
    """The overlap removal with the potential and the flow (at v = 0)."""
    st = oracle._copy_state(state)
    n = st["ang"].shape[0]
    sp = np.ascontiguousarray(species, dtype=np.uint8)
    fs = np.zeros(n, np.float32)
    tz = np.zeros(n, np.float32)
    fe = None if f_ext is None else np.ascontiguousarray(f_ext, dtype=np.float32)
    warr, nw = _walls(walls)
    phi, pn, ph, u, un, gam = _fields(potential, flow)
    steps = lib().or_lv_sd_run(ctypes.byref(params), n, _ptr(st["q"]), _ptr(st["img"]),
                               _ptr(st["ang"]), _ptr(sp), _ptr(fs), _ptr(tz), _ptr(fe),
                               int(n_steps), float(gamma), float(max_disp),
                               None if warr is None else ctypes.cast(warr, _P), nw, _ptr(phi),
                               int(pn[0]), int(pn[1]), _ptr(ph), _ptr(u), int(un[0]), int(un[1]),
                               gam)
    return st, steps
