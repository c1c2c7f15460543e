"""
CPU restatement of the gridded external potential (a helper, not a test):
the fixed fp32 sequence of swarmrl_amd/csrc/swarm_potential.cuh (DESIGN.md
section 3) in numpy uint64 / float32, operation for operation, and oracle runs
with the potential: the existing CPU oracle called one sub-step at a time with
f_ext = float32(f_ext + F(q)), F evaluated at that sub-step's folded
positions.  (Single-step oracle calls chained with step0 = step + s equal one
multi-step call bit for bit; prev, the reuse_forces record, goes to sub-step 0
only.)
"""

import numpy as np

from oracle import oracle

_F = np.float32
TWO32 = 1 << 32


def grid_coords(q, n):
    """Per axis: (i0, i1, t) of the uint32 box fractions q for n cells."""
    n = int(n)
    P = np.asarray(q, np.uint32).astype(np.uint64) * np.uint64(n)
    Pp = (P + np.uint64(n * TWO32 - (1 << 31))) % np.uint64(n * TWO32)
    i0 = (Pp >> np.uint64(32)).astype(np.int64)
    i1 = (i0 + 1) % n
    t = ((Pp & np.uint64(0xFFFFFFFF)) >> np.uint64(8)).astype(_F) * _F(2.0 ** -24)
    return i0, i1, t


def inv_spacing(h):
    """inv_h_a = (float)(1.0 / h_a), h_a in fp64."""
    return (1.0 / np.asarray(h, np.float64)).astype(_F)


def _lerp(u, v, t):
    return u + t * (v - u)


def potential_force(phi, q, inv_h, dims):
    """phi (nx, ny, nz) fp32, q [3, N] uint32, inv_h [3] fp32 -> F [3, N] fp32
    (dims = 2: nz = 1 and F[2] = 0)."""
    phi = np.asarray(phi)
    assert phi.dtype == np.float32 and phi.ndim == 3
    inv_h = np.asarray(inv_h)
    assert inv_h.dtype == np.float32
    q = np.asarray(q, np.uint32)
    F = np.zeros((3, q.shape[1]), _F)
    x0, x1, tx = grid_coords(q[0], phi.shape[0])
    y0, y1, ty = grid_coords(q[1], phi.shape[1])
    if dims == 2:
        assert phi.shape[2] == 1
        p = phi[:, :, 0]
        p00, p10, p01, p11 = p[x0, y0], p[x1, y0], p[x0, y1], p[x1, y1]
        a = p10 - p00
        b = p11 - p01
        gx = a + ty * (b - a)
        c = p01 - p00
        d = p11 - p10
        gy = c + tx * (d - c)
        F[0] = -(gx * inv_h[0])
        F[1] = -(gy * inv_h[1])
        return F
    z0, z1, tz = grid_coords(q[2], phi.shape[2])
    ix, iy, iz = (x0, x1), (y0, y1), (z0, z1)
    p = [[[phi[ix[i], iy[j], iz[k]] for k in range(2)] for j in range(2)] for i in range(2)]
    # x: the differences along x at (y, z), along y, then along z
    u = [_lerp(p[1][0][k] - p[0][0][k], p[1][1][k] - p[0][1][k], ty) for k in range(2)]
    F[0] = -(_lerp(u[0], u[1], tz) * inv_h[0])
    # y: the differences along y at (x, z), along x, then along z
    u = [_lerp(p[0][1][k] - p[0][0][k], p[1][1][k] - p[1][0][k], tx) for k in range(2)]
    F[1] = -(_lerp(u[0], u[1], tz) * inv_h[1])
    # z: the differences along z at (x, y), along x, then along y
    u = [_lerp(p[0][j][1] - p[0][j][0], p[1][j][1] - p[1][j][0], tx) for j in range(2)]
    F[2] = -(_lerp(u[0], u[1], ty) * inv_h[2])
    assert F.dtype == np.float32
    return F


def reference_force(phi, pos, h):
    """fp64 restatement of the reference's construction (espresso.py:1026-1036
    and ESPResSo's PotentialField): the field padded by one cell with
    mode="wrap", element (0, 0, 0) of the padded array at -h / 2, linear
    interpolation, F = -grad.  pos (N, 3) folded positions."""
    phi = np.asarray(phi, np.float64)
    h = np.asarray(h, np.float64)
    pad = np.pad(phi, pad_width=1, mode="wrap")
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    g = (pos + 0.5 * h) / h  # padded element k sits at (k - .5) h
    i0 = np.floor(g).astype(np.int64)
    t = g - i0
    F = np.zeros((3, n))
    for a in range(3):  # (2-D: one cell along z, its padded copies equal, F_z = 0)
        b, c = [k for k in range(3) if k != a]
        acc = np.zeros(n)
        for cb in range(2):
            for cc in range(2):
                lo, hi = [None] * 3, [None] * 3
                lo[a], hi[a] = i0[:, a], i0[:, a] + 1
                lo[b] = hi[b] = i0[:, b] + cb
                lo[c] = hi[c] = i0[:, c] + cc
                wb = t[:, b] if cb else 1.0 - t[:, b]
                wc = t[:, c] if cc else 1.0 - t[:, c]
                acc += (pad[tuple(hi)] - pad[tuple(lo)]) * wb * wc
        F[a] = -acc / h[a]
    return F


def _fe(f_ext, F):
    base = np.zeros_like(F) if f_ext is None else np.asarray(f_ext, _F)
    return (base + F).astype(_F)


def bd_run_potential(params, state, species, f_swim, torque_z, n_steps, phi, inv_h, step0=0,
                     env=0, f_ext=None, walls=None, violations=None, prev=None, trace=None):
    """oracle.bd_run with the potential: one call per sub-step.  trace: a
    list that receives every sub-step's q (the trajectory)."""
    vel = om = None
    for s in range(n_steps):
        F = potential_force(phi, state["q"], inv_h, 2)
        state, vel, om = oracle.bd_run(params, state, species, f_swim, torque_z, 1,
                                       step0=step0 + s, env=env, f_ext=_fe(f_ext, F),
                                       walls=walls, violations=violations,
                                       prev=prev if s == 0 else None)
        if trace is not None:
            trace.append(state["q"].copy())
    return state, vel, om


def bd_run3_potential(params, state, species, f_swim, torque, n_steps, phi, inv_h, step0=0,
                      env=0, f_ext=None, walls=None, violations=None, prev=None, trace=None):
    vel = om = None
    for s in range(n_steps):
        F = potential_force(phi, state["q"], inv_h, 3)
        state, vel, om = oracle.bd_run3(params, state, species, f_swim, torque, 1,
                                        step0=step0 + s, env=env, f_ext=_fe(f_ext, F),
                                        walls=walls, violations=violations,
                                        prev=prev if s == 0 else None)
        if trace is not None:
            trace.append(state["q"].copy())
    return state, vel, om


def sd_run_potential(params, state, species, n_steps, phi, inv_h, dims=2, gamma=0.1,
                     max_disp=0.1, f_swim=None, torque=None, f_ext=None, walls=None, trace=None):
    """The overlap removal with the potential (2-D: torque is torque_z).  A
    step without any force moves nothing, so running all n_steps equals the
    engine's early exit.  trace: a list that receives every step's q."""
    for _ in range(n_steps):
        F = potential_force(phi, state["q"], inv_h, dims)
        if dims == 3:
            state, _ = oracle.sd_run3(params, state, species, 1, gamma, max_disp, f_swim=f_swim,
                                      torque=torque, f_ext=_fe(f_ext, F), walls=walls)
        else:
            state, _ = oracle.sd_run(params, state, species, 1, gamma, max_disp, f_swim=f_swim,
                                     torque_z=torque, f_ext=_fe(f_ext, F), walls=walls)
        if trace is not None:
            trace.append(state["q"].copy())
    return state


def crossed_centre_planes(trace, q_start, shape, dims):
    """Per particle: did its cell index i0 (the half-cell-shifted grid
    coordinate) change along any axis between consecutive recorded sub-steps,
    i.e. did it cross a cell-centre plane."""
    prev = [grid_coords(q_start[a], shape[a])[0] for a in range(dims)]
    crossed = np.zeros(q_start.shape[1], bool)
    for q in trace:
        cur = [grid_coords(q[a], shape[a])[0] for a in range(dims)]
        for a in range(dims):
            crossed |= cur[a] != prev[a]
        prev = cur
    return crossed
