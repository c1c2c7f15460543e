"""
ctypes wrapper of the ellipsoid restatement (tests/csrc/ellipsoid_oracle.c),
TEST INFRASTRUCTURE ONLY.  The library is built by ``__graft_entry__.build()``
into tests/csrc/libellipsoidoracle.so; when it is missing it is built here,
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
SRC = _DIR / "ellipsoid_oracle.c"
LIB_PATH = _DIR / "libellipsoidoracle.so"
# oracle/Makefile's CFLAGS
CFLAGS = ["-O3", "-fPIC", "-std=c11", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-fast-math",
          "-fopenmp"]
MAX_SPECIES = 16
_P = ctypes.c_void_p


class Ellipsoids(ctypes.Structure):
    """swarm_ellipsoids_t (declared independently of the product binding)."""
    _fields_ = [
        ("aspect_ratio", ctypes.c_double),
        ("gamma_par", ctypes.c_double * MAX_SPECIES),
        ("gamma_perp", ctypes.c_double * MAX_SPECIES),
    ]


def build() -> pathlib.Path:
    import fcntl

    with open(_DIR / ".ellipsoid_build.lock", "w") as lock:
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
        pe = ctypes.POINTER(Ellipsoids)
        L.or_ell_pair.restype = ctypes.c_int
        L.or_ell_pair.argtypes = [pp, pe] + 6 * [ctypes.c_float] + [_P, _P]
        L.or_ell_bd_run.restype = ctypes.c_int
        L.or_ell_bd_run.argtypes = [pp, pe, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P,
                                    ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, _P, _P, _P, _P,
                                    _P, _P]
        L.or_ell_sd_run.restype = ctypes.c_int
        L.or_ell_sd_run.argtypes = [pp, pe, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, ctypes.c_int,
                                    ctypes.c_double, ctypes.c_double]
        _lib = L
    return _lib


def make_ellipsoids(aspect_ratio, gamma_par, gamma_perp) -> Ellipsoids:
    """gamma_par / gamma_perp: one value per species."""
    e = Ellipsoids()
    e.aspect_ratio = float(aspect_ratio)
    for s, (a, b) in enumerate(zip(np.atleast_1d(gamma_par), np.atleast_1d(gamma_perp))):
        e.gamma_par[s], e.gamma_perp[s] = float(a), float(b)
    return e


_ptr = oracle._ptr


def pair(params, ell, rx, ry, ui, uj):
    """The fp32 pair term of species (0, 0): (F_x, F_y, T_z) on i for
    r = x_j - x_i and the directors ui, uj (fp32 pairs); in_range, deep."""
    out = np.zeros(3, np.float32)
    deep = ctypes.c_int(0)
    rc = lib().or_ell_pair(ctypes.byref(params), ctypes.byref(ell), float(rx), float(ry),
                           float(ui[0]), float(ui[1]), float(uj[0]), float(uj[1]), _ptr(out),
                           ctypes.byref(deep))
    return out, bool(rc), bool(deep.value)


def bd_run(params, ell, state, species, f_swim, torque_z, n_steps, step0=0, env=0, f_ext=None,
           prev=None):
    """n_steps BD sub-steps of one env of ellipsoids.  Returns (state, info):
    info = {"pairs", "torque_pairs", "deep" (ordered pairs in range, those
    with a non-zero torque, deep overlaps; summed over the sub-steps), "vel",
    "omega"}.  prev: as oracle.bd_run (reuse_forces)."""
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
    stats = np.zeros(3, np.int64)
    rc = lib().or_ell_bd_run(ctypes.byref(params), ctypes.byref(ell), n, _ptr(st["q"]),
                             _ptr(st["img"]), _ptr(st["ang"]), _ptr(sp), _ptr(fs), _ptr(tz),
                             _ptr(fe), int(step0), int(n_steps), int(env), _ptr(vel), _ptr(om),
                             _ptr(f0), _ptr(t0), _ptr(a0), _ptr(stats))
    if rc != 0:
        raise ValueError(f"or_ell_bd_run failed ({rc})")
    info = {"pairs": int(stats[0]), "torque_pairs": int(stats[1]), "deep": int(stats[2]),
            "vel": vel, "omega": om}
    return st, info


class ReuseForces:
    """oracle.ReuseForces for an env of ellipsoids."""

    def __init__(self, state):
        n = state["q"].shape[1]
        self.prev = {"f": np.zeros(n, np.float32), "t": np.zeros(n, np.float32),
                     "ang": np.asarray(state["ang"], np.uint32).copy()}

    def run(self, params, ell, state, species, f_swim, torque, n_steps, **kw):
        st, info = bd_run(params, ell, state, species, f_swim, torque, n_steps, prev=self.prev,
                          **kw)
        self.prev = {"f": np.asarray(f_swim, np.float32).copy(),
                     "t": np.asarray(torque, np.float32).copy(), "ang": st["ang"].copy()}
        return st, info


def sd_run(params, ell, state, species, n_steps, gamma=0.1, max_disp=0.1, f_ext=None):
    st = oracle._copy_state(state)
    n = st["ang"].shape[0]
    sp = np.ascontiguousarray(species, dtype=np.uint8)
    fs = np.zeros(n, np.float32)
    tz = np.zeros(n, np.float32)
    fe = None if f_ext is None else np.ascontiguousarray(f_ext, dtype=np.float32)
    steps = lib().or_ell_sd_run(ctypes.byref(params), ctypes.byref(ell), n, _ptr(st["q"]),
                                _ptr(st["img"]), _ptr(st["ang"]), _ptr(sp), _ptr(fs), _ptr(tz),
                                _ptr(fe), int(n_steps), float(gamma), float(max_disp))
    return st, steps
