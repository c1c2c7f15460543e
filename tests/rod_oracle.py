"""
ctypes wrapper of the rod restatement (tests/csrc/rod_oracle.c), TEST
INFRASTRUCTURE ONLY.  The library is built by ``__graft_entry__.build()``
into tests/csrc/librodoracle.so; when it is missing it is built here, with the
CPU oracle's compiler flags (-ffp-contract=off: every fp32 operation rounded
on its own).
"""

from __future__ import annotations

import ctypes
import os
import pathlib
import subprocess

import numpy as np

from oracle import oracle

_DIR = pathlib.Path(__file__).resolve().parent / "csrc"
SRC = _DIR / "rod_oracle.c"
LIB_PATH = _DIR / "librodoracle.so"
# oracle/Makefile's CFLAGS
CFLAGS = ["-O3", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-fast-math",
          "-fopenmp"]
_P = ctypes.c_void_p


class Rod(ctypes.Structure):
    """swarm_rod_t (declared independently of the product binding)."""
    _fields_ = [
        ("first", ctypes.c_int32),
        ("n", ctypes.c_int32),
        ("delta", ctypes.c_double),
        ("fixed", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


def build() -> pathlib.Path:
    import fcntl

    with open(_DIR / ".rod_build.lock", "w") as lock:
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
        pr = ctypes.POINTER(Rod)
        L.or_rod_snap.restype = ctypes.c_int
        L.or_rod_snap.argtypes = [pp, ctypes.c_int, _P, _P, _P, pr]
        L.or_rod_bd_run.restype = ctypes.c_int
        L.or_rod_bd_run.argtypes = [pp, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, ctypes.c_uint64,
                                    ctypes.c_int, ctypes.c_uint32, _P, _P, pr, _P, _P, _P, _P, _P,
                                    _P, _P]
        L.or_rod_sd_run.restype = ctypes.c_int
        L.or_rod_sd_run.argtypes = [pp, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, ctypes.c_int,
                                    ctypes.c_double, ctypes.c_double, pr]
        _lib = L
    return _lib


def make_rod(first, n, delta, fixed=True) -> Rod:
    r = Rod()
    r.first, r.n, r.delta, r.fixed = int(first), int(n), float(delta), 1 if fixed else 0
    return r


def slot(b: int) -> int:
    """Signed slot of rod particle b (0: the centre)."""
    if b == 0:
        return 0
    k = b - 1
    return (-1) ** k * (k // 2 + 1)


_ptr = oracle._ptr


def snap(params, state, rod):
    """The beads onto the centre's line (what the engine does when the rod is set)."""
    st = oracle._copy_state(state)
    n = st["ang"].shape[0]
    rc = lib().or_rod_snap(ctypes.byref(params), n, _ptr(st["q"]), _ptr(st["img"]),
                           _ptr(st["ang"]), ctypes.byref(rod))
    assert rc == 0
    return st


def bd_run(params, state, species, f_swim, torque_z, n_steps, rod, step0=0, env=0, f_ext=None,
           prev=None):
    """n_steps BD sub-steps of one env with a rod.  Returns (state, info):
    info = {"F", "S" (int64 [2], 2^-24 units), "tau", "sigma" (the rod's
    forces on the colloids, int64 [2]) of the LAST sub-step, "contacts"
    (colloid-rod pairs in range, all sub-steps), "vel", "omega"}.  prev: as
    oracle.bd_run (reuse_forces)."""
    st = oracle._copy_state(state)
    n = st["ang"].shape[0]
    sp = np.ascontiguousarray(species, dtype=np.uint8)
    fs = np.ascontiguousarray(f_swim, dtype=np.float32)
    tz = np.ascontiguousarray(torque_z, dtype=np.float32)
    fe = None if f_ext is None else np.ascontiguousarray(f_ext, dtype=np.float32)
    vel = np.zeros((3, n), np.float32)
    om = np.zeros(n, np.float32)
    f0 = t0 = a0 = None
    if prev is not None:
        f0 = np.ascontiguousarray(prev["f"], dtype=np.float32)
        t0 = np.ascontiguousarray(prev["t"], dtype=np.float32)
        a0 = np.ascontiguousarray(prev["ang"], dtype=np.uint32)
    sums = np.zeros(4, np.int64)
    tau = np.zeros(1, np.float32)
    sigma = np.zeros(2, np.int64)
    contacts = np.zeros(1, np.int64)
    rc = lib().or_rod_bd_run(ctypes.byref(params), n, _ptr(st["q"]), _ptr(st["img"]),
                             _ptr(st["ang"]), _ptr(sp), _ptr(fs), _ptr(tz), _ptr(fe), int(step0),
                             int(n_steps), int(env), _ptr(vel), _ptr(om), ctypes.byref(rod),
                             _ptr(f0), _ptr(t0), _ptr(a0), _ptr(sums), _ptr(tau), _ptr(sigma),
                             _ptr(contacts))
    if rc != 0:
        raise ValueError(f"or_rod_bd_run failed ({rc})")
    info = {"F": sums[:2].copy(), "S": sums[2:].copy(), "tau": float(tau[0]),
            "sigma": sigma, "contacts": int(contacts[0]), "vel": vel, "omega": om}
    return st, info


class ReuseForces:
    """oracle.ReuseForces for a rod env (reuse_forces bookkeeping of one env)."""

    def __init__(self, state):
        n = state["q"].shape[1]
        self.prev = {"f": np.zeros(n, np.float32), "t": np.zeros(n, np.float32),
                     "ang": np.asarray(state["ang"], np.uint32).copy()}

    def run(self, params, state, species, f_swim, torque, n_steps, rod, **kw):
        st, info = bd_run(params, state, species, f_swim, torque, n_steps, rod, prev=self.prev,
                          **kw)
        self.prev = {"f": np.asarray(f_swim, np.float32).copy(),
                     "t": np.asarray(torque, np.float32).copy(), "ang": st["ang"].copy()}
        return st, info


def sd_run(params, state, species, n_steps, rod, gamma=0.1, max_disp=0.1, f_ext=None):
    st = oracle._copy_state(state)
    n = st["ang"].shape[0]
    sp = np.ascontiguousarray(species, dtype=np.uint8)
    fs = np.zeros(n, np.float32)
    tz = np.zeros(n, np.float32)
    fe = None if f_ext is None else np.ascontiguousarray(f_ext, dtype=np.float32)
    steps = lib().or_rod_sd_run(ctypes.byref(params), n, _ptr(st["q"]), _ptr(st["img"]),
                                _ptr(st["ang"]), _ptr(sp), _ptr(fs), _ptr(tz), _ptr(fe),
                                int(n_steps),
                                float(gamma), float(max_disp), ctypes.byref(rod))
    return st, steps
