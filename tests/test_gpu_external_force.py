"""
The constant external force (espresso.py:834-851, parts.ext_force; the
device array st.f_ext [3][E*N], swarm_engine_set_external_force) in every
integrator kernel that reads it, bit for bit against the CPU oracle run with
the same numbers:

  block_global_run      k_global, non-periodic boxes (BD and overlap removal)
  block_env_run         k_global, periodic 2-D (overlap removal; exact re-run)
  run_wave              k_cluster_run / k_cluster_run_wide
  run_big_clusters      the check workgroup's big-cluster run
  k_nl_step2            2-D neighbour-list window
  k_rod_run             rod engines (BD and overlap removal)
  block_global_run3     k_global3 (BD and overlap removal)
  run_wave3             k_cluster_run3
  k_nl_step3            3-D neighbour-list window

Every case hands the engine forces that differ per particle and per env, with
a non-zero z component, as float64 values that fp32 does not represent (the
host's cast and its [E*N][3] -> [3][E*N] transposition are part of what is
compared), runs several chunks (the step counter and the window parity
advance), shows from swarm_engine_window_stats that the path it is named
after ran, and checks that the oracle without the force gives other
positions.  Nothing is left out of any comparison: q, img, ang (dir in 3-D)
and the velocities of every particle of every env.
"""

import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _eq(got, ref, keys=("q", "img", "ang")):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), k


KEYS3 = ("q", "img", "dir")


def _forces(rng, E, n, scale, xy_max=None):
    """[E][N][3] float64, what swarm_engine_set_external_force takes.  xy_max:
    cap on the in-plane magnitude."""
    f = rng.normal(size=(E, n, 3)) * scale
    if xy_max is not None:
        norm = np.hypot(f[..., 0], f[..., 1])
        f[..., :2] *= np.minimum(1.0, xy_max / norm)[..., None]
    assert np.all(f != 0.0) and np.any(f.astype(np.float32) != f)
    return f


def _fe(f_ext, e):
    """Env e's forces as the oracle takes them: [3][N] fp32."""
    return np.ascontiguousarray(f_ext[e].T).astype(np.float32)


def _compare(h, states, vels, keys=("q", "img", "ang")):
    got = h.download()
    vel = h.velocities()
    n = h.n
    for e in range(h.E):
        _eq(got[e], states[e], keys)
        assert np.array_equal(vel[:, e * n:(e + 1) * n], vels[e]), e


def _lattice(rng, k, a, lo, jitter):
    """k x k colloids on a jittered square lattice of spacing a from lo."""
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2)
    pos = np.zeros((k * k, 3))
    pos[:, :2] = lo + (g + 0.5) * a + rng.uniform(-jitter, jitter, (k * k, 2))
    th = 2 * np.pi * rng.random(k * k)
    return pos, np.stack([np.cos(th), np.sin(th), np.zeros(k * k)], 1)


# ------------------------------------------------------------ 1. run_wave
@pytest.mark.parametrize("table", ["0", "1"])
@pytest.mark.parametrize("wide", ["0", "1"])
def test_run_wave_external_force_bit_exact(wide, table, monkeypatch):
    """k_cluster_run (wide = 0) and k_cluster_run_wide (1), normals drawn in
    the kernel (table = 0) or read from the k_noise table (1): 3 envs of 300
    dilute swimmers of two species (area fraction 0.1) after the overlap
    removal, chunks of 37, 1 and 100 sub-steps.  Every window ran on cluster
    waves and passed its check (|f_ext| + f_swim stays below the 10 force
    units that dilute windows of this kind run without fallback)."""
    from gpu_harness import Harness, random_state, species_list

    monkeypatch.setenv("SWARMRL_AMD_WIDE_RUN", wide)
    monkeypatch.setenv("SWARMRL_AMD_NOISE_TABLE", table)
    rng = np.random.default_rng(101)
    E, n = 3, 300
    L = float(np.sqrt(n * np.pi / 0.1))
    box = [L, L, L]
    sp = rng.integers(0, 2, n)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 42, species_list(), sp, n_envs=E)
    states = [random_state(rng, n, box) for _ in range(E)]
    h.upload(states)
    h.sd(300)
    states = [oracle.sd_run(h.op, s, sp, 300)[0] for s in states]
    f_ext = _forces(rng, E, n, 2.0, xy_max=5.0)
    h.set_external_force(f_ext)
    plain = states[0]
    step = 0
    for nsteps in (37, 1, 100):
        f = rng.uniform(1.0, 4.5, E * n).astype(np.float32)
        t = rng.normal(size=E * n).astype(np.float32) * 5
        h.set_actions(f, t)
        h.integrate(nsteps)
        vels = []
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            states[e], v, _ = oracle.bd_run(h.op, states[e], sp, f[s], t[s], nsteps, step0=step,
                                            env=e, f_ext=_fe(f_ext, e))
            vels.append(v)
        plain, _, _ = oracle.bd_run(h.op, plain, sp, f[:n], t[:n], nsteps, step0=step)
        step += nsteps
        _compare(h, states, vels)
        fb, waves = h.window_stats()
        print("run_wave wide", wide, "table", table, "window", nsteps, "fallback", fb, "waves",
              waves)
        assert np.all(fb == 0) and np.all(waves > 0), (fb, waves)
    assert not np.array_equal(plain["q"], states[0]["q"])


# ----------------------------------- 2. run_big_clusters, 3. the exact re-run
def _patch_box(rng, n_free):
    """One 10 x 10 patch at 2.5 um spacing (100 colloids within r_c + skin of
    their neighbours: a cluster wider than a wave) and n_free free colloids."""
    pts = [(40.0 + 2.5 * gx, 40.0 + 2.5 * gy) for gx in range(10) for gy in range(10)]
    while len(pts) < 100 + n_free:
        p = rng.random(2) * 200.0
        if min((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 for q in pts) > 16.0:
            pts.append((p[0], p[1]))
    n = len(pts)
    pos = np.zeros((n, 3))
    pos[:, :2] = pts
    a = 2 * np.pi * rng.random(n)
    return pos, np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)


def test_big_clusters_external_force_bit_exact():
    """run_big_clusters: the 100-colloid patch cannot run in a wave, so a
    window that reports no fallback ran it in the check's workgroup; two
    windows, the free colloids on cluster waves beside it."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(102)
    box = [200.0, 200.0, 200.0]
    pos, dirs = _patch_box(rng, 200)
    n = len(pos)
    sp = np.zeros(n, int)
    st = oracle.state_from_positions(pos, dirs, box)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 5, species_list()[:1], sp)
    h.upload([st])
    f_ext = _forces(rng, 1, n, 1.5, xy_max=4.0)
    h.set_external_force(f_ext)
    plain = st
    step = 0
    for nsteps in (100, 60):
        f = rng.uniform(1.0, 5.0, n).astype(np.float32)
        t = rng.choice([-5.0, 2.0, 5.0], n).astype(np.float32)
        h.set_actions(f, t)
        h.integrate(nsteps)
        st, vel, _ = oracle.bd_run(h.op, st, sp, f, t, nsteps, step0=step, f_ext=_fe(f_ext, 0))
        plain, _, _ = oracle.bd_run(h.op, plain, sp, f, t, nsteps, step0=step)
        step += nsteps
        _compare(h, [st], [vel])
        fb, waves = h.window_stats()
        print("big clusters window", nsteps, "fallback", fb, "waves", waves)
        assert fb[0] == 0 and waves[0] > 0, (fb, waves)
    assert not np.array_equal(plain["q"][:, :100], st["q"][:, :100])  # the patch felt the force


@pytest.mark.parametrize("reuse", [False, True])
def test_exact_rerun_external_force_bit_exact(reuse):
    """block_env_run as the exact re-run: in the same box one window's
    external force is +-300 force units along x on the two halves of the
    colloids (6 um in 100 sub-steps, past the skin), so the decomposition
    check fails and the window runs again from its snapshot on the global
    path -- with that window's forces, not the ones before or after.  Also
    with reuse_forces (sub-step 0 reuses the swim force and torque; the
    external force is the current one in every sub-step)."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(103)
    box = [200.0, 200.0, 200.0]
    pos, dirs = _patch_box(rng, 200)
    n = len(pos)
    sp = np.zeros(n, int)
    st = oracle.state_from_positions(pos, dirs, box)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 5, species_list()[:1], sp, reuse=reuse)
    h.upload([st])
    track = oracle.ReuseForces(st) if reuse else None
    plain = st
    step = 0
    seen = []
    for nsteps, big in ((100, False), (100, True), (60, False)):
        f_ext = _forces(rng, 1, n, 1.5, xy_max=4.0)
        if big:
            f_ext[0, :, 0] += np.where(np.arange(n) < n // 2, 300.0, -300.0)
        h.set_external_force(f_ext)
        f = rng.uniform(1.0, 5.0, n).astype(np.float32)
        t = rng.choice([-5.0, 2.0, 5.0], n).astype(np.float32)
        h.set_actions(f, t)
        h.integrate(nsteps)
        if reuse:
            st, vel, _ = track.run(h.op, st, sp, f, t, nsteps, step0=step, f_ext=_fe(f_ext, 0))
        else:
            st, vel, _ = oracle.bd_run(h.op, st, sp, f, t, nsteps, step0=step,
                                       f_ext=_fe(f_ext, 0))
        plain, _, _ = oracle.bd_run(h.op, plain, sp, f, t, nsteps, step0=step)
        step += nsteps
        _compare(h, [st], [vel])
        fb, waves = h.window_stats()
        seen.append(int(fb[0]))
        print("re-run reuse", reuse, "window", nsteps, "big", big, "fallback", fb, "waves", waves)
    assert seen[1] == 2, seen  # the +-300 window took the exact re-run
    assert not np.array_equal(plain["q"], st["q"])


# ------------------------------------------------------------ 4. k_nl_step2
def test_nlist2_external_force_bit_exact(monkeypatch):
    """One k_nl_step2 launch per sub-step: 2 envs of 1600 colloids of two
    species on a jittered lattice of spacing 3 (the links percolate), chunks
    of 100, 1 and 37; every window passed its check without cluster waves."""
    from gpu_harness import Harness, species_list

    monkeypatch.setenv("SWARMRL_AMD_NLIST", "1")
    rng = np.random.default_rng(104)
    E, k = 2, 40
    n = k * k
    L = 3.0 * k
    box = [L, L, L]
    sp = rng.integers(0, 2, n)
    states = [oracle.state_from_positions(*_lattice(rng, k, 3.0, 0.0, 0.3), box)
              for _ in range(E)]
    h = Harness(box, 1e-3, 1.0239, 1.0239, 21, species_list(), sp, n_envs=E)
    h.upload(states)
    f_ext = _forces(rng, E, n, 2.0, xy_max=5.0)
    h.set_external_force(f_ext)
    plain = states[0]
    step = 0
    for nsteps in (100, 1, 37):
        f = rng.uniform(1.0, 4.5, E * n).astype(np.float32)
        t = rng.normal(size=E * n).astype(np.float32) * 5
        h.set_actions(f, t)
        h.integrate(nsteps)
        vels = []
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            states[e], v, _ = oracle.bd_run(h.op, states[e], sp, f[s], t[s], nsteps, step0=step,
                                            env=e, f_ext=_fe(f_ext, e))
            vels.append(v)
        plain, _, _ = oracle.bd_run(h.op, plain, sp, f[:n], t[:n], nsteps, step0=step)
        step += nsteps
        _compare(h, states, vels)
        fb, waves = h.window_stats()
        print("nlist2 window", nsteps, "fallback", fb, "waves", waves)
        assert np.all(fb == 0) and np.all(waves == 0), (fb, waves)
    assert not np.array_equal(plain["q"], states[0]["q"])


# ------------------------------------------------------ 5. block_global_run
def test_global_path_nonperiodic_external_force_bit_exact(monkeypatch):
    """block_global_run (non-periodic boxes take it, not the LDS variant)
    with the cluster path switched off: 2 envs of 300 colloids, some outside
    the box and pairs close across its faces; the overlap removal with the
    force set, then chunks of 60, 1 and 40 sub-steps.  No window ran a wave."""
    from gpu_harness import Harness, species_list
    from test_gpu_nonperiodic import _straddling

    monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "0")
    rng = np.random.default_rng(105)
    E, n, L = 2, 300, 50.0
    box = [L, L, L]
    sp = rng.integers(0, 2, n)
    states = [oracle.state_from_positions(*_straddling(rng, n, L), box) for _ in range(E)]
    assert np.count_nonzero(states[0]["img"][:2]) > 20
    h = Harness(box, 1e-3, 1.0239, 1.0239, 8, species_list(), sp, n_envs=E, periodic=False)
    h.upload(states)
    f_ext = _forces(rng, E, n, 3.0)
    h.set_external_force(f_ext)
    h.sd(150)
    before = states
    states = [oracle.sd_run(h.op, s, sp, 150, f_ext=_fe(f_ext, e))[0]
              for e, s in enumerate(states)]
    got = h.download()
    for e in range(E):
        _eq(got[e], states[e])
    assert not np.array_equal(oracle.sd_run(h.op, before[0], sp, 150)[0]["q"], states[0]["q"])
    plain = states[0]
    step = 0
    for nsteps in (60, 1, 40):
        f = rng.normal(size=E * n).astype(np.float32) * 10
        t = rng.normal(size=E * n).astype(np.float32) * 5
        h.set_actions(f, t)
        h.integrate(nsteps)
        vels = []
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            states[e], v, _ = oracle.bd_run(h.op, states[e], sp, f[s], t[s], nsteps, step0=step,
                                            env=e, f_ext=_fe(f_ext, e))
            vels.append(v)
        plain, _, _ = oracle.bd_run(h.op, plain, sp, f[:n], t[:n], nsteps, step0=step)
        step += nsteps
        _compare(h, states, vels)
        fb, waves = h.window_stats()
        print("global non-periodic window", nsteps, "fallback", fb, "waves", waves)
        assert np.all(waves == 0) and np.all(fb == 0), (fb, waves)
    assert not np.array_equal(plain["q"], states[0]["q"])


def test_global_path_sedimentation_onto_a_wall_bit_exact(monkeypatch):
    """The same path with confining walls on the box faces and the external
    force pointing into the y = 0 wall (sedimentation, 6 +- 1.5 force units
    down): the colloids settle against the wall as the oracle's do, and the
    wall contacts counted by the engine equal the oracle's."""
    from gpu_harness import Harness, species_list

    monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "0")
    rng = np.random.default_rng(106)
    E, k, L = 2, 17, 60.0
    n = k * k
    box = [L, L, L]
    walls = [{"kind": 0, "normal": [1, 0, 0], "offset": 0.0},
             {"kind": 0, "normal": [-1, 0, 0], "offset": -L},
             {"kind": 0, "normal": [0, 1, 0], "offset": 0.0},
             {"kind": 0, "normal": [0, -1, 0], "offset": -L}]
    sp = rng.integers(0, 2, n)
    # the lowest row starts 1.6 um above the wall: within the wall's range for radius 1
    states = [oracle.state_from_positions(*_lattice(rng, k, 3.3, 0.0, 0.15), box)
              for _ in range(E)]
    h = Harness(box, 1e-3, 1.0239, 1.0239, 9, species_list(), sp, n_envs=E, periodic=False)
    h.upload(states)
    h.set_walls(walls)
    f_ext = _forces(rng, E, n, 1.5)
    f_ext[..., 1] -= 6.0
    h.set_external_force(f_ext)
    y0 = oracle.unwrapped(states[0], box)[:, 1]
    viol = np.zeros(1, np.uint64)
    plain = states[0]
    step = 0
    for nsteps in (100, 1, 99):
        f = rng.uniform(0.5, 3.0, E * n).astype(np.float32)
        t = rng.normal(size=E * n).astype(np.float32) * 5
        h.set_actions(f, t)
        h.integrate(nsteps)
        vels = []
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            states[e], v, _ = oracle.bd_run(h.op, states[e], sp, f[s], t[s], nsteps, step0=step,
                                            env=e, f_ext=_fe(f_ext, e), walls=walls,
                                            violations=viol)
            vels.append(v)
        plain, _, _ = oracle.bd_run(h.op, plain, sp, f[:n], t[:n], nsteps, step0=step,
                                    walls=walls)
        step += nsteps
        _compare(h, states, vels)
        fb, waves = h.window_stats()
        print("sedimentation window", nsteps, "fallback", fb, "waves", waves)
        assert np.all(waves == 0) and np.all(fb == 0), (fb, waves)
    print("sedimentation wall violations", h.wall_violations(), int(viol[0]))
    assert h.wall_violations() == int(viol[0])
    y1 = oracle.unwrapped(states[0], box)[:, 1]
    assert np.mean(y1 - y0) < -0.1 and np.all(y1 > 0.0)  # sank, and stayed above the wall
    assert not np.array_equal(plain["q"], states[0]["q"])


@pytest.mark.parametrize("case", ["two_cells", "two_per_thread"])
def test_lds_global_path_narrow_grid_and_two_particles_per_thread(case, monkeypatch):
    """k_global's LDS-resident sub-steps where the stencil and the particle
    loop take their other arms, 2 envs each, an external force set.
    two_cells: 12 colloids of radius 1 on a 3 x 4 lattice in a periodic
    6 x 40 um box, a grid of 2 x 16 cells: both cells of a row are one range
    and there is no wrap range; columns 2 um apart, also through the periodic
    boundary.  (A box this narrow has no cluster path.)
    two_per_thread: 1100 colloids of radius 0.5, 1.05 um apart, in a 100 um
    box with the cluster path switched off: a thread steps two of them.
    Pairs are inside the cutoff before and after the run."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(108)
    E = 2
    if case == "two_cells":
        n, box, radius, species = 12, [6.0, 40.0, 40.0], 1.0, species_list()[:1]
        g = np.stack(np.meshgrid(np.arange(3), np.arange(4), indexing="ij"), -1).reshape(-1, 2)
        lattice = np.array([1.0, 12.0]) + g * np.array([2.0, 2.05])
    else:
        monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "0")
        n, box, radius = 1100, [100.0, 100.0, 100.0], 0.5
        species = [(0.5, 4.0, 6.0, 1.0e-6, 4.0e-7)]
        g = np.stack(np.meshgrid(np.arange(34), np.arange(34), indexing="ij"), -1).reshape(-1, 2)
        lattice = 30.0 + g[:n] * 1.05
    sp = np.zeros(n, int)
    states = []
    for _ in range(E):
        pos = np.zeros((n, 3))
        pos[:, :2] = lattice + rng.uniform(-0.1, 0.1, (n, 2))
        th = 2 * np.pi * rng.random(n)
        states.append(oracle.state_from_positions(
            pos, np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1), box))
    h = Harness(box, 1e-3, 1.0239, 1.0239, 12, species, sp, n_envs=E)
    assert oracle.cell_grid(h.op, n, 2 * radius) == ((1, 4) if case == "two_cells" else (5, 5))
    h.upload(states)
    f_ext = _forces(rng, E, n, 1.0)
    h.set_external_force(f_ext)
    touching = [len(oracle.neighbor_pairs(h.op, s, 2 * radius)) for s in states]
    step = 0
    for nsteps in (12, 1):
        f = rng.uniform(1.0, 4.0, E * n).astype(np.float32)
        t = rng.normal(size=E * n).astype(np.float32) * 5
        h.set_actions(f, t)
        h.integrate(nsteps)
        vels = []
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            states[e], v, _ = oracle.bd_run(h.op, states[e], sp, f[s], t[s], nsteps, step0=step,
                                            env=e, f_ext=_fe(f_ext, e))
            vels.append(v)
        step += nsteps
        _compare(h, states, vels)
        fb, waves = h.window_stats()
        assert np.all(waves == 0) and np.all(fb == 0), (fb, waves)
    touching += [len(oracle.neighbor_pairs(h.op, s, 2 * radius)) for s in states]
    print("lds global path", case, "pairs inside the cutoff", touching)
    assert min(touching) >= n // 4, touching


# ------------------------------------------------------ 6. overlap removal
def test_overlap_removal_2d_external_force_bit_exact():
    """swarm_engine_remove_overlap with the force set (SwarmEngine uploads it
    before its overlap removal): k_global's steepest descent on a periodic
    2-D box (block_env_run), 3 dense envs of two species."""
    from gpu_harness import Harness, random_state, species_list

    rng = np.random.default_rng(107)
    E, n = 3, 300
    box = [40.0, 40.0, 40.0]
    sp = rng.integers(0, 2, n)
    h = Harness(box, 1e-4, 1.0239, 1.0239, 7, species_list(), sp, n_envs=E)
    states = [random_state(rng, n, box) for _ in range(E)]
    h.upload(states)
    f_ext = _forces(rng, E, n, 0.6)  # gamma F on both sides of max_disp = 0.1
    assert np.any(np.abs(f_ext) > 1.0) and np.any(np.abs(f_ext) < 1.0)
    h.set_external_force(f_ext)
    f = rng.uniform(0.2, 1.0, E * n).astype(np.float32)
    t = rng.normal(size=E * n).astype(np.float32)
    h.set_actions(f, t)
    h.sd(120)
    got = h.download()
    for e in range(E):
        s = slice(e * n, (e + 1) * n)
        ref, steps = oracle.sd_run(h.op, states[e], sp, 120, f_swim=f[s], torque_z=t[s],
                                   f_ext=_fe(f_ext, e))
        assert steps == 120
        _eq(got[e], ref)
    plain, _ = oracle.sd_run(h.op, states[0], sp, 120, f_swim=f[:n], torque_z=t[:n])
    assert not np.array_equal(plain["q"], got[0]["q"])
    assert np.array_equal(plain["q"][2], got[0]["q"][2])  # no stray z motion in 2-D


def test_overlap_removal_3d_external_force_bit_exact():
    """The 3-D steepest descent (k_global3) with the force set: z moves."""
    from gpu_harness import Harness, random_state3, species_list

    rng = np.random.default_rng(108)
    E, n = 2, 120
    box = [30.0, 30.0, 30.0]
    sp = rng.integers(0, 2, n)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 4, species_list(), sp, n_envs=E, n_dims=3)
    states = [random_state3(rng, n, box) for _ in range(E)]
    h.upload(states)
    f_ext = _forces(rng, E, n, 0.6)
    h.set_external_force(f_ext)
    f = rng.uniform(0.2, 1.0, E * n).astype(np.float32)
    tq = rng.normal(size=(3, E * n)).astype(np.float32)
    h.set_torque_xy(tq[:2])
    h.set_actions(f, tq[2])
    h.sd(80)
    got = h.download()
    for e in range(E):
        s = slice(e * n, (e + 1) * n)
        ref, steps = oracle.sd_run3(h.op, states[e], sp, 80, f_swim=f[s], torque=tq[:, s],
                                    f_ext=_fe(f_ext, e))
        assert steps == 80
        _eq(got[e], ref, KEYS3)
    plain, _ = oracle.sd_run3(h.op, states[0], sp, 80, f_swim=f[:n], torque=tq[:, :n])
    assert not np.array_equal(plain["q"][2], got[0]["q"][2])


# ------------------------------------------------------------------ 7. 3-D
@pytest.mark.parametrize("path", ["global", "cluster", "nlist"])
def test_3d_external_force_bit_exact(path, monkeypatch):
    """block_global_run3 (the cluster path switched off), run_wave3 (cluster
    window) and k_nl_step3 (neighbour-list window): 2 envs of 120 colloids of
    two species on a jittered cubic lattice in a 30 um box, torque about all
    three axes, chunks of 50, 1 and 30; all three equal bd_run3 with f_ext.
    global: no waves; cluster: waves and no fallback; nlist: a windowed
    engine without waves and without fallback."""
    from gpu_harness import Harness, species_list
    from test_gpu_3d_cluster import _lattice3

    if path == "global":
        monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "0")
    else:
        monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "1")
        monkeypatch.setenv("SWARMRL_AMD_NLIST", "1" if path == "nlist" else "0")
    rng = np.random.default_rng(109)
    E, n = 2, 120
    lat = [_lattice3(rng, n, a=6.0) for _ in range(E)]
    L = lat[0][2]
    assert L == 30.0
    box = [L, L, L]
    sp = rng.integers(0, 2, n)
    states = [oracle.state3_from_positions(p, d, box) for p, d, _ in lat]
    h = Harness(box, 1e-3, 1.0239, 1.0239, 17, species_list(), sp, n_envs=E, n_dims=3)
    h.upload(states)
    f_ext = _forces(rng, E, n, 2.0)
    h.set_external_force(f_ext)
    plain = states[0]
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
            states[e], v, w = oracle.bd_run3(h.op, states[e], sp, f[s], tq[:, s], nsteps,
                                             step0=step, env=e, f_ext=_fe(f_ext, e))
            vels.append(v)
            oms.append(w)
        plain, _, _ = oracle.bd_run3(h.op, plain, sp, f[:n], tq[:, :n], nsteps, step0=step)
        step += nsteps
        _compare(h, states, vels, KEYS3)
        assert np.array_equal(h.omegas3(), np.concatenate(oms, axis=1))
        fb, waves = h.window_stats()
        print("3-D", path, "window", nsteps, "fallback", fb, "waves", waves)
        assert np.all(fb == 0), (fb, waves)
        assert np.all(waves > 0) if path == "cluster" else np.all(waves == 0), (path, waves)
    assert not np.array_equal(plain["q"][2], states[0]["q"][2])  # z felt the force


# ------------------------------------------------------------- 8. k_rod_run
@pytest.mark.parametrize("forces", ["type", "per_particle"])
def test_rod_run_external_force_bit_exact(tmp_path, forces):
    """k_rod_run (every run and the overlap removal of a rod engine): the
    smallest engine of test_gpu_rod.py, E = 2, 24 swimmers around a free
    11-particle rod, three slices of 20 sub-steps with reuse_forces.
    type: add_const_force_to_colloids on the swimmers' type through the
    product API.  per_particle: forces that differ per particle and env,
    non-zero on the rod's own particles too -- the kernel and the
    restatement both leave those out."""
    import rod_oracle
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction
    from test_gpu_rod import _add_points, _add_rod, _engine, _restatement, _ring

    rng = np.random.default_rng(110)
    ureg, eng = _engine(tmp_path, n_envs=2)
    pos, dirs = _ring((25.0, 25.0), 8.0, 24)
    _add_points(ureg, eng, pos, dirs, 1.0)
    _add_rod(ureg, eng, (25.0, 25.0), 20.0, 3.0, 0.3, 11, False)
    E, n = eng.n_envs, eng.n_particles
    eng.add_const_force_to_colloids(ureg.Quantity(np.array([0.31, -0.23, 0.17]), "sim_force"), 0)
    if forces == "per_particle":
        f_ext = _forces(rng, E, n, 0.3)
        eng._compose_ext_force = lambda: f_ext  # what the engine uploads at its set-up
    else:
        f_ext = eng._compose_ext_force()
        assert f_ext.shape == (E, n, 3) and np.all(f_ext[:, 24:] == 0.0)
    p, sp, rod, states = _restatement(eng)
    f_swim = np.where(np.asarray(eng._types_list) == 0, 5.0, 0.0).astype(np.float32)
    steps = eng.params.steps_per_slice
    start = states
    states = [rod_oracle.sd_run(p, st, sp, 1000, rod, f_ext=_fe(f_ext, e))[0]
              for e, st in enumerate(states)]
    reuse = [rod_oracle.ReuseForces(st) for st in states]
    plain_st = rod_oracle.sd_run(p, start[0], sp, 1000, rod)[0]
    plain = rod_oracle.ReuseForces(plain_st)
    contacts = np.zeros(E, np.int64)
    ff = ForceFunction({"0": dummy_models.ConstForce(5.0)})
    for k in range(3):
        eng.integrate(1, ff)
        got = eng.get_raw_state()
        vel = eng._host()["vel"]
        for e in range(E):
            states[e], info = reuse[e].run(p, states[e], sp, f_swim, np.zeros(n), steps, rod,
                                           step0=k * steps, env=e, f_ext=_fe(f_ext, e))
            contacts[e] += info["contacts"]
            for key in ("q", "img", "ang"):
                assert np.array_equal(got[key][..., e * n:(e + 1) * n], states[e][key]), (key, e)
            assert np.array_equal(vel[e].T.astype(np.float32), info["vel"]), e
        plain_st, _ = plain.run(p, plain_st, sp, f_swim, np.zeros(n), steps, rod,
                                step0=k * steps)
    print("rod", forces, "contacts", contacts, "steps", eng.step_count())
    assert eng._rod is not None and eng.step_count() == 60  # a rod engine: k_rod_run ran them
    assert not np.array_equal(plain_st["q"][:, :24], states[0]["q"][:, :24])
