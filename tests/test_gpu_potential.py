"""
The gridded external potential (espresso.py:995-1036;
swarm_engine_set_potential_field, swarm_potential.cuh) in every integrator
path that reads the external force, bit for bit against the CPU oracle driven
one sub-step at a time with f_ext + F(q) (tests/potential_ref.py):

  run_wave              k_cluster_run / k_cluster_run_wide, table / in-kernel normals
  run_big_clusters      the check workgroup's big-cluster run
  block_env_run         the exact re-run (and the periodic 2-D overlap removal)
  k_nl_step2            2-D neighbour-list window
  block_global_run      non-periodic boxes (BD and overlap removal), with walls too
  block_global_run3     k_global3 (BD and overlap removal)
  run_wave3             k_cluster_run3
  k_nl_step3            3-D neighbour-list window

and through SwarmEngine.add_external_potential: the drift down a linear
potential at kT = 0, and the reference's use, a circular arena from a step
potential (CI/espresso_tests/unit_tests/test_flow.py:73-89).

Every bit-exact case uses a smooth plus random potential on an anisotropic
grid with nx != ny and no power of two, fine enough that at least a tenth of
the particles cross a cell-centre plane during the run (asserted from the
oracle's trajectory), particles inside the first and the last half cell of
every axis, and a constant external force of fp64 values that fp32 does not
represent beside it.  Nothing is left out of any comparison: q, img, ang (dir
in 3-D) and the velocities of every particle of every env.
"""

import numpy as np
import pytest
import torch

import potential_ref as pr
from oracle import oracle

pytestmark = pytest.mark.gpu

KEYS2 = ("q", "img", "ang")
KEYS3 = ("q", "img", "dir")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


# ------------------------------------------------------------------ helpers
def _grad_bound(phi, h, dims):
    """An upper bound of |F| anywhere: the interpolated gradient along an
    axis is a convex combination of neighbour differences over the spacing."""
    g = [np.max(np.abs(np.roll(phi, -1, axis=a) - phi)) / h[a] for a in range(dims)]
    return float(np.sqrt(np.sum(np.square(g))))


def _field(rng, shape, box, fmax, dims=2):
    """Smooth plus random potential, scaled so |F| <= fmax everywhere.
    Returns (phi fp32, h fp64 [3], inv_h fp32 [3])."""
    shape = tuple(shape)
    assert shape[0] != shape[1] and all(s & (s - 1) for s in shape[:dims])
    h = np.asarray(box, float) / np.asarray(shape)
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    phi = (np.sin(2 * np.pi * (i + 0.5) / shape[0]) * np.cos(4 * np.pi * (j + 0.5) / shape[1])
           + 0.5 * np.cos(2 * np.pi * (k + 0.5) / shape[2]) + 0.02 * rng.normal(size=shape))
    phi = (phi * (0.999 * fmax / _grad_bound(phi, h, dims))).astype(np.float32)
    assert _grad_bound(phi.astype(np.float64), h, dims) <= fmax
    return phi, h, pr.inv_spacing(h)


def _set_potential(h, phi, spacing):
    """swarm_engine_set_potential_field on a Harness (phi None: remove)."""
    h.native.bind_stream()
    if phi is None:
        h.native.call("swarm_engine_set_potential_field", None, 0, 0, 0, None)
        return
    p = np.ascontiguousarray(phi, np.float32)
    s = np.ascontiguousarray(spacing, np.float64)
    h.native.call("swarm_engine_set_potential_field", p.ctypes.data, p.shape[0], p.shape[1],
                  p.shape[2], s.ctypes.data)


def _pin_half_cells(pos, box, shape, dims):
    """Particles 2 a and 2 a + 1 into the first and the last half cell of axis a."""
    for a in range(dims):
        hc = 0.5 * box[a] / shape[a]
        pos[2 * a, a] = 0.3 * hc
        pos[2 * a + 1, a] = box[a] - 0.3 * hc
    return pos


def _half_cells_occupied(states, shape, dims):
    for a in range(dims):
        P = np.concatenate([s["q"][a] for s in states]).astype(np.uint64) * np.uint64(shape[a])
        if not (np.any(P < (1 << 31)) and np.any(P >= shape[a] * (1 << 32) - (1 << 31))):
            return False
    return True


def _forces(rng, E, n, scale, xy_max=None):
    """[E][N][3] float64 constant forces that fp32 does not represent."""
    f = rng.normal(size=(E, n, 3)) * scale
    if xy_max is not None:
        norm = np.hypot(f[..., 0], f[..., 1])
        f[..., :2] *= np.minimum(1.0, xy_max / norm)[..., None]
    assert np.all(f != 0.0) and np.any(f.astype(np.float32) != f)
    return f


def _fe(f_ext, e):
    return np.ascontiguousarray(f_ext[e].T).astype(np.float32)


def _eq(got, ref, keys):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), k


def _compare(h, states, vels, keys=KEYS2):
    got = h.download()
    vel = h.velocities()
    n = h.n
    for e in range(h.E):
        _eq(got[e], states[e], keys)
        assert np.array_equal(vel[:, e * n:(e + 1) * n], vels[e]), e


def _max_force(phi, inv_h, states, dims):
    F = np.concatenate([pr.potential_force(phi, s["q"], inv_h, dims) for s in states], axis=1)
    return float(np.max(np.sqrt(np.sum(np.square(F.astype(np.float64)), axis=0))))


def _lattice(rng, k, a, lo, jitter):
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2)
    pos = np.zeros((k * k, 3))
    pos[:, :2] = lo + (g + 0.5) * a + rng.uniform(-jitter, jitter, (k * k, 2))
    th = 2 * np.pi * rng.random(k * k)
    return pos, np.stack([np.cos(th), np.sin(th), np.zeros(k * k)], 1)


def _run_chunks_2d(h, states, sp, f_ext, phi, inv_h, chunks, draw_actions, walls=None,
                   expect=None, tag=""):
    """Chunks of BD sub-steps on the engine and the oracle (with and without
    the potential); compares after every chunk, checks the window statistics
    with expect(fb, waves), returns the share of env 0's particles that
    crossed a cell-centre plane and env 0's oracle state without the potential."""
    E, n = h.E, h.n
    plain = states[0]
    q_start = states[0]["q"].copy()
    trace = []
    step = 0
    for nsteps in chunks:
        f, t = draw_actions(E * n)
        h.set_actions(f, t)
        h.integrate(nsteps)
        vels = []
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            states[e], v, _ = pr.bd_run_potential(
                h.op, states[e], sp, f[s], t[s], nsteps, phi, inv_h, step0=step, env=e,
                f_ext=_fe(f_ext, e), walls=walls, trace=trace if e == 0 else None)
            vels.append(v)
        plain, _, _ = oracle.bd_run(h.op, plain, sp, f[:n], t[:n], nsteps, step0=step,
                                    f_ext=_fe(f_ext, 0), walls=walls)
        step += nsteps
        _compare(h, states, vels)
        fb, waves = h.window_stats()
        print(tag, "window", nsteps, "fallback", fb, "waves", waves)
        if expect is not None:
            assert expect(fb, waves), (fb, waves)
    assert not np.array_equal(plain["q"], states[0]["q"])  # the oracle without the potential
    crossed = pr.crossed_centre_planes(trace, q_start, phi.shape, 2)
    print(tag, "crossed a cell-centre plane:", crossed.mean())
    return crossed.mean(), plain


# ------------------------------------------------------------ 1. run_wave
@pytest.mark.parametrize("table", ["0", "1"])
@pytest.mark.parametrize("wide", ["0", "1"])
def test_run_wave_potential_bit_exact(wide, table, monkeypatch):
    """k_cluster_run (wide = 0) and k_cluster_run_wide (1), normals drawn in
    the kernel (table = 0) or read from the table (1): 3 envs of 300 dilute
    swimmers of two species (area fraction 0.1) after the overlap removal,
    chunks of 37, 1 and 100 sub-steps on cluster waves without fallback
    (|F| <= 4, |f_ext| <= 1, f_swim <= 4.5: below the 10 force units such
    windows run without fallback)."""
    from gpu_harness import Harness, species_list

    monkeypatch.setenv("SWARMRL_AMD_WIDE_RUN", wide)
    monkeypatch.setenv("SWARMRL_AMD_NOISE_TABLE", table)
    rng = np.random.default_rng(201)
    E, n = 3, 300
    L = float(np.sqrt(n * np.pi / 0.1))
    box = [L, L, L]
    shape = (139, 97, 1)
    sp = rng.integers(0, 2, n)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 42, species_list(), sp, n_envs=E)
    states = []
    for _ in range(E):
        pos = np.zeros((n, 3))
        pos[:, :2] = rng.random((n, 2)) * L
        th = 2 * np.pi * rng.random(n)
        states.append(oracle.state_from_positions(
            _pin_half_cells(pos, box, shape, 2),
            np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1), box))
    h.upload(states)
    h.sd(300)
    states = [oracle.sd_run(h.op, s, sp, 300)[0] for s in states]
    assert _half_cells_occupied(states, shape, 2)
    phi, spacing, inv_h = _field(rng, shape, box, 4.0)
    assert _max_force(phi, inv_h, states, 2) <= 4.0
    f_ext = _forces(rng, E, n, 0.5, xy_max=1.0)
    h.set_external_force(f_ext)
    _set_potential(h, phi, spacing)

    def actions(m):
        return (rng.uniform(1.0, 4.5, m).astype(np.float32),
                rng.normal(size=m).astype(np.float32) * 5)

    frac, _ = _run_chunks_2d(h, states, sp, f_ext, phi, inv_h, (37, 1, 100), actions,
                             expect=lambda fb, w: np.all(fb == 0) and np.all(w > 0),
                             tag=f"run_wave wide {wide} table {table}")
    assert frac >= 0.1


def test_run_wave_potential_alone_throughput_bit_exact(monkeypatch):
    """k_cluster_run<false, false, false, true>: the potential as its only
    variant flag (one species, no walls; SWARMRL_AMD_WIDE_RUN=0 for the
    throughput kernel and SWARMRL_AMD_NOISE_TABLE=0 for normals drawn in the
    kernel, which so small an engine would otherwise read from the table): 2
    envs of 64 colloids on a jittered lattice, chunks of 20, 1 and 40
    sub-steps on cluster waves without fallback."""
    from gpu_harness import Harness, species_list

    monkeypatch.setenv("SWARMRL_AMD_WIDE_RUN", "0")
    monkeypatch.setenv("SWARMRL_AMD_NOISE_TABLE", "0")
    rng = np.random.default_rng(221)
    E, k, a = 2, 8, 6.0
    n, L = k * k, k * a
    box = [L, L, L]
    shape = (13, 11, 1)
    sp = np.zeros(n, int)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 42, species_list()[:1], sp, n_envs=E)
    states = []
    for _ in range(E):
        pos, dirs = _lattice(rng, k, a, 0.0, 1.0)
        states.append(oracle.state_from_positions(pos, dirs, box))
    h.upload(states)
    phi, spacing, inv_h = _field(rng, shape, box, 4.0)
    f_ext = _forces(rng, E, n, 0.5, xy_max=1.0)
    h.set_external_force(f_ext)
    _set_potential(h, phi, spacing)

    def actions(m):
        return (rng.uniform(1.0, 4.5, m).astype(np.float32),
                rng.normal(size=m).astype(np.float32) * 5)

    _run_chunks_2d(h, states, sp, f_ext, phi, inv_h, (20, 1, 40), actions,
                   expect=lambda fb, w: np.all(fb == 0) and np.all(w > 0),
                   tag="run_wave potential alone")


def test_run_wave3_potential_alone_bit_exact(monkeypatch):
    """k_cluster_run3 with the potential as its only variant flag (one
    species, no walls): 2 envs of 120 colloids on a jittered cubic lattice,
    chunks of 20 and 1 sub-steps on cluster waves without fallback."""
    from gpu_harness import Harness, species_list
    from test_gpu_3d_cluster import _lattice3

    monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "1")
    monkeypatch.setenv("SWARMRL_AMD_NLIST", "0")
    rng = np.random.default_rng(222)
    E, n = 2, 120
    shape = (7, 5, 3)
    lat = [_lattice3(rng, n, a=6.0) for _ in range(E)]
    L = lat[0][2]
    box = [L, L, L]
    sp = np.zeros(n, int)
    states = [oracle.state3_from_positions(p, d, box) for p, d, _ in lat]
    h = Harness(box, 1e-3, 1.0239, 1.0239, 17, species_list()[:1], sp, n_envs=E, n_dims=3)
    h.upload(states)
    phi, spacing, inv_h = _field(rng, shape, box, 4.0, dims=3)
    f_ext = _forces(rng, E, n, 0.5)
    h.set_external_force(f_ext)
    _set_potential(h, phi, spacing)
    plain = states[0]
    step = 0
    for nsteps in (20, 1):
        f = rng.uniform(1.0, 4.5, E * n).astype(np.float32)
        tq = rng.normal(scale=5.0, size=(3, E * n)).astype(np.float32)
        h.set_torque_xy(tq[:2])
        h.set_actions(f, tq[2])
        h.integrate(nsteps)
        vels = []
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            states[e], v, _ = pr.bd_run3_potential(
                h.op, states[e], sp, f[s], tq[:, s], nsteps, phi, inv_h, step0=step, env=e,
                f_ext=_fe(f_ext, e))
            vels.append(v)
        plain, _, _ = oracle.bd_run3(h.op, plain, sp, f[:n], tq[:, :n], nsteps, step0=step,
                                     f_ext=_fe(f_ext, 0))
        step += nsteps
        _compare(h, states, vels, KEYS3)
        fb, waves = h.window_stats()
        print("3-D potential alone window", nsteps, "fallback", fb, "waves", waves)
        assert np.all(fb == 0) and np.all(waves > 0), (fb, waves)
    assert not np.array_equal(plain["q"], states[0]["q"])  # the oracle without the potential


# ----------------------------------- 2. run_big_clusters, 3. the exact re-run
def _patch_box(rng, n_free, shape):
    """One 10 x 10 patch at 2.5 um spacing (a cluster wider than a wave) and
    n_free free colloids in a 200 um box; the first four free colloids sit in
    the first / last half cells."""
    pts = [(40.0 + 2.5 * gx, 40.0 + 2.5 * gy) for gx in range(10) for gy in range(10)]
    hc = [0.5 * 200.0 / shape[0], 0.5 * 200.0 / shape[1]]
    pts += [(0.3 * hc[0], 150.0), (200.0 - 0.3 * hc[0], 120.0), (150.0, 0.3 * hc[1]),
            (120.0, 200.0 - 0.3 * hc[1])]

    def d2(p, q):  # minimum image
        dx, dy = abs(p[0] - q[0]), abs(p[1] - q[1])
        return min(dx, 200.0 - dx) ** 2 + min(dy, 200.0 - dy) ** 2

    while len(pts) < 100 + n_free:
        p = rng.random(2) * 200.0
        if min(d2(p, q) for q in pts) > 16.0:
            pts.append((p[0], p[1]))
    n = len(pts)
    pos = np.zeros((n, 3))
    pos[:, :2] = pts
    a = 2 * np.pi * rng.random(n)
    return pos, np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)


def test_big_clusters_potential_bit_exact():
    """run_big_clusters: the 100-colloid patch runs in the check's workgroup
    (no fallback), the free colloids on cluster waves beside it; two windows."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(202)
    box = [200.0, 200.0, 200.0]
    shape = (283, 211, 1)
    pos, dirs = _patch_box(rng, 200, shape)
    n = len(pos)
    sp = np.zeros(n, int)
    states = [oracle.state_from_positions(pos, dirs, box)]
    assert _half_cells_occupied(states, shape, 2)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 5, species_list()[:1], sp)
    h.upload(states)
    phi, spacing, inv_h = _field(rng, shape, box, 4.0)
    assert _max_force(phi, inv_h, states, 2) <= 4.0
    f_ext = _forces(rng, 1, n, 0.3, xy_max=0.5)
    h.set_external_force(f_ext)
    _set_potential(h, phi, spacing)
    start = states[0]["q"].copy()

    def actions(m):
        return (rng.uniform(1.0, 5.0, m).astype(np.float32),
                rng.choice([-5.0, 2.0, 5.0], m).astype(np.float32))

    frac, plain = _run_chunks_2d(h, states, sp, f_ext, phi, inv_h, (100, 60), actions,
                                 expect=lambda fb, w: fb[0] == 0 and w[0] > 0,
                                 tag="big clusters")
    assert frac >= 0.1
    assert not np.array_equal(start[:, :100], states[0]["q"][:, :100])
    # the patch's members (the part of the env that run_big_clusters
    # integrates: 100 linked colloids fit no 64-lane wave, and the window did
    # not fall back) felt the field: with the same noise and actions but
    # without the potential every one of them ends elsewhere
    moved = np.any(plain["q"][:2, :100] != states[0]["q"][:2, :100], axis=0)
    assert np.all(moved), np.count_nonzero(~moved)


@pytest.mark.parametrize("reuse", [False, True])
def test_exact_rerun_potential_bit_exact(reuse):
    """block_env_run as the exact re-run: the second window's potential
    carries a tent of slope -+300 force units on the two halves of the box
    (6 um in 100 sub-steps, past the skin), replaced at the C level between
    the windows: that window fails its check and runs again from its snapshot
    on the global path with that window's field; the windows before and after
    do not.  With reuse_forces sub-step 0 reuses the swim force and torque
    only: the field is evaluated at the current position in every sub-step."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(203)
    box = [200.0, 200.0, 200.0]
    shape = (283, 211, 1)
    pos, dirs = _patch_box(rng, 200, shape)
    n = len(pos)
    sp = np.zeros(n, int)
    st = oracle.state_from_positions(pos, dirs, box)
    assert _half_cells_occupied([st], shape, 2)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 5, species_list()[:1], sp, reuse=reuse)
    h.upload([st])
    prev = oracle.ReuseForces(st).prev if reuse else None
    phi, spacing, inv_h = _field(rng, shape, box, 4.0)
    xc = (np.arange(shape[0]) + 0.5) * spacing[0]
    tent = (-300.0 * np.minimum(xc, 200.0 - xc))[:, None, None]  # F = +300 left, -300 right
    phi_big = (phi.astype(np.float64) + tent).astype(np.float32)
    f_ext = _forces(rng, 1, n, 0.3, xy_max=0.5)
    h.set_external_force(f_ext)
    plain = st
    q_start = st["q"].copy()
    trace = []
    step = 0
    seen = []
    for nsteps, big in ((100, False), (100, True), (60, False)):
        field = phi_big if big else phi
        _set_potential(h, field, spacing)
        f = rng.uniform(1.0, 5.0, n).astype(np.float32)
        t = rng.choice([-5.0, 2.0, 5.0], n).astype(np.float32)
        h.set_actions(f, t)
        h.integrate(nsteps)
        st, vel, _ = pr.bd_run_potential(h.op, st, sp, f, t, nsteps, field, inv_h, step0=step,
                                         f_ext=_fe(f_ext, 0), prev=prev, trace=trace)
        if reuse:
            prev = {"f": f.copy(), "t": t.copy(), "ang": st["ang"].copy()}
        plain, _, _ = oracle.bd_run(h.op, plain, sp, f, t, nsteps, step0=step,
                                    f_ext=_fe(f_ext, 0))
        step += nsteps
        _compare(h, [st], [vel])
        fb, waves = h.window_stats()
        seen.append(int(fb[0]))
        print("re-run reuse", reuse, "window", nsteps, "big", big, "fallback", fb, "waves", waves)
    assert seen[1] == 2 and seen[0] != 2 and seen[2] != 2, seen
    assert not np.array_equal(plain["q"], st["q"])
    assert pr.crossed_centre_planes(trace, q_start, shape, 2).mean() >= 0.1


# ------------------------------------------------------------ 4. k_nl_step2
def test_nlist2_potential_bit_exact(monkeypatch):
    """One k_nl_step2 launch per sub-step: 2 envs of 1600 colloids of two
    species on a jittered lattice of spacing 3, chunks of 100, 1 and 37; every
    window passed its check without cluster waves."""
    from gpu_harness import Harness, species_list

    monkeypatch.setenv("SWARMRL_AMD_NLIST", "1")
    rng = np.random.default_rng(204)
    E, k = 2, 40
    n = k * k
    L = 3.0 * k
    box = [L, L, L]
    shape = (173, 131, 1)
    sp = rng.integers(0, 2, n)
    states = []
    for _ in range(E):
        pos, dirs = _lattice(rng, k, 3.0, 0.0, 0.3)
        # the lattice's outer rows sit 1.5 +- 0.3 from the faces: one colloid
        # of a row into the half cell at the face, its periodic neighbour to
        # 2.15 from the face (2.25 apart, and 2.05 or more from the next row)
        for a, (g_first, g_last) in enumerate(((0, 5), (10, 15))):
            hc = 0.5 * L / shape[a]

            def idx(outer, g, a=a):
                return outer * k + g if a == 0 else g * k + outer

            pos[idx(0, g_first), a] = 0.3 * hc
            pos[idx(k - 1, g_first), a] = L - 2.15
            pos[idx(k - 1, g_last), a] = L - 0.3 * hc
            pos[idx(0, g_last), a] = 2.15
        states.append(oracle.state_from_positions(pos, dirs, box))
    assert _half_cells_occupied(states, shape, 2)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 21, species_list(), sp, n_envs=E)
    h.upload(states)
    phi, spacing, inv_h = _field(rng, shape, box, 4.0)
    f_ext = _forces(rng, E, n, 0.5, xy_max=1.0)
    h.set_external_force(f_ext)
    _set_potential(h, phi, spacing)

    def actions(m):
        return (rng.uniform(1.0, 4.5, m).astype(np.float32),
                rng.normal(size=m).astype(np.float32) * 5)

    frac, _ = _run_chunks_2d(h, states, sp, f_ext, phi, inv_h, (100, 1, 37), actions,
                             expect=lambda fb, w: np.all(fb == 0) and np.all(w == 0),
                             tag="nlist2")
    assert frac >= 0.1


# ------------------------------------------------------ 5. block_global_run
@pytest.mark.parametrize("with_walls", [False, True])
def test_global_path_nonperiodic_potential_bit_exact(with_walls, monkeypatch):
    """block_global_run (non-periodic boxes) with the cluster path switched
    off: the overlap removal with the potential set, then chunks of 60, 1 and
    40 sub-steps.  Without walls colloids start outside the box and pairs sit
    close across its faces: a colloid outside the box feels the wrapped field
    at its folded position (the image counters do not enter).  With confining
    walls on the box faces (a lattice inside them, on a 23 x 19 grid whose
    half cells are wider than a colloid's radius, so four colloids sit inside
    them without touching a wall): walls and potential compose."""
    from gpu_harness import Harness, species_list
    from test_gpu_nonperiodic import _straddling

    monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "0")
    rng = np.random.default_rng(205)
    E = 2
    walls = None
    if with_walls:
        k, L = 17, 60.0
        n = k * k
        walls = [{"kind": 0, "normal": [1, 0, 0], "offset": 0.0},
                 {"kind": 0, "normal": [-1, 0, 0], "offset": -L},
                 {"kind": 0, "normal": [0, 1, 0], "offset": 0.0},
                 {"kind": 0, "normal": [0, -1, 0], "offset": -L}]
        # half a cell wider than a colloid's radius, so a colloid can sit in
        # the first / last half cell without touching the wall
        shape = (23, 19, 1)
    else:
        n, L = 300, 50.0
        shape = (71, 53, 1)
    box = [L, L, L]
    sp = rng.integers(0, 2, n)
    states = []
    for _ in range(E):
        if with_walls:
            pos, dirs = _lattice(rng, k, 3.3, 0.0, 0.15)
            # 1.15 from a wall: outside its range (radius <= 1), inside the
            # half cells (1.30 and 1.58 wide); index = gx k + gy
            pos[0 * k + 3, 0], pos[(k - 1) * k + 5, 0] = 1.15, L - 1.15
            pos[7 * k + 0, 1], pos[9 * k + (k - 1), 1] = 1.15, L - 1.15
        else:
            pos, dirs = _straddling(rng, n, L)
            # folded into the half cells from outside the box and from inside
            hc = [0.5 * L / shape[0], 0.5 * L / shape[1]]
            pos[30, 0], pos[31, 0] = L + 0.3 * hc[0], -0.3 * hc[0]
            pos[32, 1], pos[33, 1] = 0.3 * hc[1], L - 0.3 * hc[1]
        states.append(oracle.state_from_positions(pos, dirs, box))
    if not with_walls:
        assert np.count_nonzero(states[0]["img"][:2]) > 20
    assert _half_cells_occupied(states, shape, 2)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 8, species_list(), sp, n_envs=E, periodic=False)
    h.upload(states)
    if with_walls:
        h.set_walls(walls)
    phi, spacing, inv_h = _field(rng, shape, box, 6.0)
    f_ext = _forces(rng, E, n, 1.0)
    h.set_external_force(f_ext)
    _set_potential(h, phi, spacing)
    h.sd(150)
    before = states
    states = [pr.sd_run_potential(h.op, s, sp, 150, phi, inv_h, f_ext=_fe(f_ext, e), walls=walls)
              for e, s in enumerate(states)]
    got = h.download()
    for e in range(E):
        _eq(got[e], states[e], KEYS2)
    no_pot = oracle.sd_run(h.op, before[0], sp, 150, f_ext=_fe(f_ext, 0), walls=walls)[0]
    assert not np.array_equal(no_pot["q"], states[0]["q"])

    def actions(m):
        scale = 3.0 if with_walls else 10.0
        return (rng.normal(size=m).astype(np.float32) * scale,
                rng.normal(size=m).astype(np.float32) * 5)

    E_, n_ = h.E, h.n
    plain = states[0]
    q_start = states[0]["q"].copy()
    trace = []
    step = 0
    for nsteps in (60, 1, 40):
        f, t = actions(E_ * n_)
        h.set_actions(f, t)
        h.integrate(nsteps)
        vels = []
        for e in range(E_):
            s = slice(e * n_, (e + 1) * n_)
            states[e], v, _ = pr.bd_run_potential(
                h.op, states[e], sp, f[s], t[s], nsteps, phi, inv_h, step0=step, env=e,
                f_ext=_fe(f_ext, e), walls=walls, trace=trace if e == 0 else None)
            vels.append(v)
        plain, _, _ = oracle.bd_run(h.op, plain, sp, f[:n_], t[:n_], nsteps, step0=step,
                                    f_ext=_fe(f_ext, 0), walls=walls)
        step += nsteps
        _compare(h, states, vels)
        fb, waves = h.window_stats()
        print("global non-periodic walls", with_walls, "window", nsteps, "fallback", fb, "waves",
              waves)
        assert np.all(waves == 0) and np.all(fb == 0), (fb, waves)
    assert not np.array_equal(plain["q"], states[0]["q"])
    assert pr.crossed_centre_planes(trace, q_start, shape, 2).mean() >= 0.1


# ------------------------------------------------------ 6. overlap removal
def test_overlap_removal_2d_potential_bit_exact():
    """swarm_engine_remove_overlap with the potential set (k_global's
    steepest descent on a periodic 2-D box, block_env_run), 3 dense
    envs of two species, against sd_run_potential."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(207)
    E, n = 3, 300
    box = [40.0, 40.0, 40.0]
    shape = (57, 43, 1)
    sp = rng.integers(0, 2, n)
    h = Harness(box, 1e-4, 1.0239, 1.0239, 7, species_list(), sp, n_envs=E)
    states = []
    for _ in range(E):
        pos = np.zeros((n, 3))
        pos[:, :2] = rng.random((n, 2)) * 40.0
        th = 2 * np.pi * rng.random(n)
        states.append(oracle.state_from_positions(
            _pin_half_cells(pos, box, shape, 2),
            np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1), box))
    assert _half_cells_occupied(states, shape, 2)
    h.upload(states)
    phi, spacing, inv_h = _field(rng, shape, box, 2.0)  # gamma F on both sides of max_disp
    f_ext = _forces(rng, E, n, 0.4)
    h.set_external_force(f_ext)
    _set_potential(h, phi, spacing)
    f = rng.uniform(0.2, 1.0, E * n).astype(np.float32)
    t = rng.normal(size=E * n).astype(np.float32)
    h.set_actions(f, t)
    h.sd(120)
    got = h.download()
    trace = []
    for e in range(E):
        s = slice(e * n, (e + 1) * n)
        ref = pr.sd_run_potential(h.op, states[e], sp, 120, phi, inv_h, f_swim=f[s],
                                  torque=t[s], f_ext=_fe(f_ext, e),
                                  trace=trace if e == 0 else None)
        _eq(got[e], ref, KEYS2)
    assert pr.crossed_centre_planes(trace, states[0]["q"], shape, 2).mean() >= 0.1
    plain, _ = oracle.sd_run(h.op, states[0], sp, 120, f_swim=f[:n], torque_z=t[:n],
                             f_ext=_fe(f_ext, 0))
    assert not np.array_equal(plain["q"], got[0]["q"])
    assert np.array_equal(plain["q"][2], got[0]["q"][2])  # no stray z motion in 2-D


def test_overlap_removal_3d_potential_bit_exact():
    """The 3-D steepest descent (k_global3) with the potential set: z moves."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(208)
    E, n = 2, 120
    box = [30.0, 30.0, 30.0]
    shape = (35, 27, 44)
    sp = rng.integers(0, 2, n)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 4, species_list(), sp, n_envs=E, n_dims=3)
    states = [oracle.state3_from_positions(
        _pin_half_cells(rng.random((n, 3)) * 30.0, box, shape, 3), rng.normal(size=(n, 3)), box)
        for _ in range(E)]
    assert _half_cells_occupied(states, shape, 3)
    h.upload(states)
    phi, spacing, inv_h = _field(rng, shape, box, 2.0, dims=3)
    f_ext = _forces(rng, E, n, 0.4)
    h.set_external_force(f_ext)
    _set_potential(h, phi, spacing)
    f = rng.uniform(0.2, 1.0, E * n).astype(np.float32)
    tq = rng.normal(size=(3, E * n)).astype(np.float32)
    h.set_torque_xy(tq[:2])
    h.set_actions(f, tq[2])
    h.sd(80)
    got = h.download()
    trace = []
    for e in range(E):
        s = slice(e * n, (e + 1) * n)
        ref = pr.sd_run_potential(h.op, states[e], sp, 80, phi, inv_h, dims=3, f_swim=f[s],
                                  torque=tq[:, s], f_ext=_fe(f_ext, e),
                                  trace=trace if e == 0 else None)
        _eq(got[e], ref, KEYS3)
    assert pr.crossed_centre_planes(trace, states[0]["q"], shape, 3).mean() >= 0.1
    plain, _ = oracle.sd_run3(h.op, states[0], sp, 80, f_swim=f[:n], torque=tq[:, :n],
                              f_ext=_fe(f_ext, 0))
    assert not np.array_equal(plain["q"][2], got[0]["q"][2])


# ------------------------------------------------------------------ 7. 3-D
@pytest.mark.parametrize("path", ["global", "cluster", "nlist"])
def test_3d_potential_bit_exact(path, monkeypatch):
    """block_global_run3 (the cluster path switched off), run_wave3 (cluster
    window) and k_nl_step3 (neighbour-list window): 2 envs of 120 colloids of
    two species on a jittered cubic lattice in a 30 um box, a 35 x 27 x 44
    grid, torque about all three axes, chunks of 50, 1 and 30.  z feels the
    force."""
    from gpu_harness import Harness, species_list
    from test_gpu_3d_cluster import _lattice3

    if path == "global":
        monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "0")
    else:
        monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "1")
        monkeypatch.setenv("SWARMRL_AMD_NLIST", "1" if path == "nlist" else "0")
    rng = np.random.default_rng(209)
    E, n = 2, 120
    shape = (35, 27, 44)
    lat = [_lattice3(rng, n, a=6.0) for _ in range(E)]
    L = lat[0][2]
    assert L == 30.0
    box = [L, L, L]
    sp = rng.integers(0, 2, n)
    states = []
    for p, d, _ in lat:
        # (lattice sites sit 3 from the faces; 2.7 towards a face keeps 3.3 to
        # the periodic neighbour)
        states.append(oracle.state3_from_positions(_pin_half_cells(p, box, shape, 3), d, box))
    assert _half_cells_occupied(states, shape, 3)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 17, species_list(), sp, n_envs=E, n_dims=3)
    h.upload(states)
    phi, spacing, inv_h = _field(rng, shape, box, 4.0, dims=3)
    assert _max_force(phi, inv_h, states, 3) <= 4.0
    f_ext = _forces(rng, E, n, 0.5)
    h.set_external_force(f_ext)
    _set_potential(h, phi, spacing)
    plain = states[0]
    q_start = states[0]["q"].copy()
    trace = []
    step = 0
    for nsteps in (50, 1, 30):
        f = rng.uniform(1.0, 4.5, E * n).astype(np.float32)
        tq = rng.normal(scale=5.0, size=(3, E * n)).astype(np.float32)
        h.set_torque_xy(tq[:2])
        h.set_actions(f, tq[2])
        h.integrate(nsteps)
        vels, oms = [], []
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            states[e], v, w = pr.bd_run3_potential(
                h.op, states[e], sp, f[s], tq[:, s], nsteps, phi, inv_h, step0=step, env=e,
                f_ext=_fe(f_ext, e), trace=trace if e == 0 else None)
            vels.append(v)
            oms.append(w)
        plain, _, _ = oracle.bd_run3(h.op, plain, sp, f[:n], tq[:, :n], nsteps, step0=step,
                                     f_ext=_fe(f_ext, 0))
        step += nsteps
        _compare(h, states, vels, KEYS3)
        assert np.array_equal(h.omegas3(), np.concatenate(oms, axis=1))
        fb, waves = h.window_stats()
        print("3-D", path, "window", nsteps, "fallback", fb, "waves", waves)
        assert np.all(fb == 0), (fb, waves)
        assert np.all(waves > 0) if path == "cluster" else np.all(waves == 0), (path, waves)
    assert not np.array_equal(plain["q"][2], states[0]["q"][2])  # z felt the force
    assert pr.crossed_centre_planes(trace, q_start, shape, 3).mean() >= 0.1


# ------------------------------------------------- the C entry's refusals
def test_set_potential_field_refusals_and_removal():
    """swarm_engine_set_potential_field: SWARM_EINVAL (a ValueError through
    the binding) for a count that is not positive, a non-finite value, nz != 1
    on a 2-D engine, a grid that does not tile the box, a spacing that is not
    positive and a grid beyond 32-bit indexing; a refused call leaves the
    field as it was, and phi = NULL removes it (the run then equals the oracle
    without a potential)."""
    from gpu_harness import Harness, random_state, species_list

    rng = np.random.default_rng(210)
    n, L = 60, 30.0
    box = [L, L, L]
    sp = np.zeros(n, int)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 3, species_list()[:1], sp)
    st = oracle.sd_run(h.op, random_state(rng, n, box), sp, 200)[0]
    h.upload([st])
    shape = (7, 5, 1)
    phi, spacing, inv_h = _field(rng, shape, box, 3.0)
    _set_potential(h, phi, spacing)

    def refused(p, s, dims=None):
        p = np.ascontiguousarray(p, np.float32)
        d = p.shape if dims is None else dims
        s = np.ascontiguousarray(s, np.float64)
        with pytest.raises(ValueError):
            h.native.call("swarm_engine_set_potential_field", p.ctypes.data, d[0], d[1], d[2],
                          s.ctypes.data)

    refused(phi, spacing, (0, 5, 1))
    refused(phi, spacing, (7, -5, 1))
    bad = phi.copy()
    bad[3, 2, 0] = np.inf
    refused(bad, spacing)
    refused(np.zeros((7, 5, 2), np.float32), [L / 7, L / 5, L / 2])
    refused(phi, [L / 7, L / 5 * (1 + 1e-6), L])
    refused(phi, [L / 7, 0.0, L])
    refused(phi, [L / 70000, L / 70000, L], (70000, 70000, 1))  # 4.9e9 values: not read
    f = rng.uniform(1.0, 4.0, n).astype(np.float32)
    t = rng.normal(size=n).astype(np.float32)
    h.set_actions(f, t)
    h.integrate(20)
    ref, vel, _ = pr.bd_run_potential(h.op, st, sp, f, t, 20, phi, inv_h)
    _compare(h, [ref], [vel])  # the refused calls left the 7 x 5 field in place
    _set_potential(h, None, None)
    h.integrate(20)
    plain, vel, _ = oracle.bd_run(h.op, ref, sp, f, t, 20, step0=20)
    _compare(h, [plain], [vel])
    with_pot, _, _ = pr.bd_run_potential(h.op, ref, sp, f, t, 20, phi, inv_h, step0=20)
    assert not np.array_equal(with_pot["q"], plain["q"])


# ------------------------------------------------------------ 8. product API
def _product_engine(ureg, tmp_path, L, n_envs=1, seed=42, reuse_forces=True, **kw):
    from swarmrl_amd.engine import MDParams, SwarmEngine

    p = MDParams(ureg=ureg, box_length=ureg.Quantity([L, L, L], "micrometer"), **kw)
    return SwarmEngine(p, n_dims=2, seed=seed, out_folder=tmp_path, write_chunk_size=1,
                       n_envs=n_envs, reuse_forces=reuse_forces)


def test_product_linear_potential_drift_kat(tmp_path):
    """One passive colloid at kT = 0 in a potential linear in x between two
    cell centres: x = x0 - phi' / gamma t (rtol 2e-6, the bound of the
    reference's drift test, test_espresso.py:108-111); reuse_forces = False,
    so no first-step lag."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    L = 1000.0
    eng = _product_engine(ureg, tmp_path, L, reuse_forces=False,
                          fluid_dyn_viscosity=ureg.Quantity(8.9e-3, "pascal * second"),
                          WCA_epsilon=ureg.Quantity(1e-20, "joule"),
                          temperature=ureg.Quantity(0, "kelvin"),
                          time_step=ureg.Quantity(0.01, "second"),
                          time_slice=ureg.Quantity(0.1, "second"),
                          write_interval=ureg.Quantity(0.1, "second"))
    # 10 x 4 cells of 100 x 250 um, phi = slope * x_centre: linear between the
    # centres of cells 0 and 9 (x = 50 .. 950; the period closes across the
    # face).  The colloid starts at x = 700; the overlap removal, in which the
    # constraint acts too, takes it 100 um down the slope (0.1 um a step), so
    # the drift is measured from the state after the first slice
    slope = 250.0  # sim_energy / um = sim_force
    xc = (np.arange(10) + 0.5) * 100.0
    pot = np.repeat((slope * xc)[:, None], 4, axis=1)[:, :, None]
    eng.add_external_potential(ureg.Quantity(pot, "sim_energy"),
                               ureg.Quantity(np.array([100.0, 250.0, L]), "micrometer"))
    eng.add_colloid_on_point(ureg.Quantity(1.0, "micrometer"),
                             ureg.Quantity(np.array([700.0, 300.0, 0.0]), "micrometer"),
                             np.array([0.0, 1.0, 0.0]), type_colloid=1)
    ff = ForceFunction({"1": dummy_models.ConstForce(0.0)})
    eng.integrate(1, ff)
    old = eng.get_particle_data()
    t0 = eng.system.time
    assert 590.0 < old["Unwrapped_Positions"][0][0] < 600.0  # the overlap removal's 100 um
    eng.integrate(10, ff)
    new = eng.get_particle_data()
    gt, _ = eng.get_friction_coefficients(1)
    t = eng.system.time - t0
    assert t == pytest.approx(1.0)
    expect = old["Unwrapped_Positions"] + t * np.array([-slope / gt, 0.0, 0.0])
    print("linear potential: x", new["Unwrapped_Positions"][0], "expected", expect[0])
    assert 50.0 < new["Unwrapped_Positions"][0][0] < old["Unwrapped_Positions"][0][0] - 1.0
    np.testing.assert_allclose(new["Unwrapped_Positions"], expect, rtol=2e-6)
    eng.finalize()


def test_product_circular_arena_confines_swimmers(tmp_path):
    """The reference's use (test_flow.py:73-89): a circular arena from the
    step potential 2 F_swim h mask on a 100 x 100 x 1 grid in a 100 um box
    (a wall of gradient force 2 F_swim per cell step), ten ConstForce
    swimmers per env starting inside, E = 2.  The slice count is sized on the
    CPU so that without the potential at least one swimmer leaves the disc;
    with it every swimmer of every env ends inside."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.units import UnitRegistry

    L, R, f_swim = 100.0, 30.0, 10.0
    h = 1.0
    ij = (np.arange(100) + 0.5) * h
    mask = (np.hypot(ij[:, None] - 50.0, ij[None, :] - 50.0) > R).astype(float)
    pot = (2.0 * f_swim * h * mask)[:, :, None]

    def slices_until_one_leaves(eng, margin=5.0, cap=600):
        """The free run of env 0 restated on the CPU (the overlap removal,
        then slices with reuse_forces): the first slice count after which a
        swimmer is margin beyond the disc."""
        n = eng.n_particles
        p = oracle.make_params(eng._box, eng._time_step, eng._kT(),
                               eng.params.WCA_epsilon.m_as("sim_energy"), eng.seed,
                               [eng._species_keys[0]])
        sp = np.zeros(n, np.uint8)
        st = oracle.state_from_positions(np.stack(eng._pos[0]), np.stack(eng._dir[0]), eng._box)
        st, _ = oracle.sd_run(p, st, sp, 1000)
        track = oracle.ReuseForces(st)
        steps = eng.params.steps_per_slice
        for k in range(cap):
            st, _, _ = track.run(p, st, sp, np.full(n, f_swim, np.float32),
                                 np.zeros(n, np.float32), steps, step0=k * steps)
            pos = oracle.unwrapped(st, eng._box, dims=2)
            if np.any(np.hypot(pos[:, 0] - 50.0, pos[:, 1] - 50.0) > R + margin):
                return k + 1
        raise AssertionError("no swimmer left the disc on the CPU")

    def run(with_potential, folder, n_slices=None):
        ureg = UnitRegistry()
        eng = _product_engine(ureg, folder, L, n_envs=2, seed=5,
                              fluid_dyn_viscosity=ureg.Quantity(8.9e-4, "pascal * second"),
                              WCA_epsilon=ureg.Quantity(293, "kelvin") * ureg.boltzmann_constant,
                              temperature=ureg.Quantity(293, "kelvin"),
                              time_step=ureg.Quantity(0.005, "second"),
                              time_slice=ureg.Quantity(0.05, "second"),
                              write_interval=ureg.Quantity(5.0, "second"))
        if with_potential:
            eng.add_external_potential(ureg.Quantity(pot, "sim_energy"),
                                       ureg.Quantity(np.array([h, h, L]), "micrometer"))
        eng.add_colloids(10, ureg.Quantity(1.0, "micrometer"),
                         ureg.Quantity(np.array([50.0, 50.0, 0.0]), "micrometer"),
                         ureg.Quantity(10.0, "micrometer"), type_colloid=0)
        if n_slices is None:
            n_slices = slices_until_one_leaves(eng)
        eng.integrate(n_slices, ForceFunction({"0": dummy_models.ConstForce(f_swim)}))
        raw = eng.get_raw_state()
        pos = oracle.unwrapped({"q": raw["q"], "img": raw["img"]}, [L, L, L], dims=2)
        eng.finalize()
        return np.hypot(pos[:, 0] - 50.0, pos[:, 1] - 50.0), n_slices

    r_free, n_slices = run(False, tmp_path / "free")
    r_pot, _ = run(True, tmp_path / "arena", n_slices)
    print("arena: slices", n_slices, "max r free", r_free.max(), "max r confined", r_pot.max())
    assert 50 <= n_slices <= 600
    assert r_free.shape == (20,) and np.any(r_free > R)
    # the step's ramp ends at the centre of the first masked cell, at most one
    # cell diagonal beyond the disc's radius
    assert np.all(r_pot < R + np.sqrt(2.0) * h)
