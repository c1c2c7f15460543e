"""
3-D at scale: the two windowed 3-D paths against the CPU oracle, bit for
bit (swarm_integrator3.cuh):
  cluster  k_build_sort3 -> k_build_pairs3 -> k_cluster_build ->
           k_cluster_run3 -> k_check3 (dilute boxes)
  nlist    k_build_sort3 -> k_build_nlist3 -> one k_nl_step3 per sub-step
           -> k_check3 (boxes whose rc + skin
           graph percolates)
SWARMRL_AMD_NLIST=0|1 picks the path (by default the engine picks it from
the density).

The reference engine's default dimension is 3 (EspressoMD(n_dims=3),
espresso.py:143-152; free rotation about all axes, espresso.py:415-426);
the BD update is or_bd_run3's sequence (oracle/swarm_oracle.c).  Covered:
bench-size envs (4096 colloids) that pass the decomposition check, several
envs, two species, reuse_forces with a one-sub-step window, walls, and
windows that fail the check or are flagged by the build (a cluster wider
than a wave) and re-run on the 3-D global path.
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


def _eq3(got, ref):
    for k in ("q", "img", "dir"):
        assert np.array_equal(got[k], ref[k]), k


def _lattice3(rng, n, a=4.6, jitter=0.3):
    """n colloids on a jittered cubic lattice of spacing a (no overlaps; few
    links within r_i + r_j + skin = 4, so small clusters); the box is k a."""
    k = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1)
    pos = (g.reshape(-1, 3)[:n] + 0.5) * a + rng.uniform(-jitter, jitter, (n, 3))
    d = rng.normal(size=(n, 3))
    return pos, d, k * a


@pytest.fixture(params=["cluster", "nlist"])
def path3(request, monkeypatch):
    """cluster: the cluster window; nlist: one k_nl_step3 launch per
    sub-step over per-colloid Verlet lists."""
    monkeypatch.setenv("SWARMRL_AMD_NLIST", "0" if request.param == "cluster" else "1")
    return request.param


def _stats(h):
    fb = np.zeros(h.E, np.int32)
    w = np.zeros(h.E, np.int32)
    h.native.call("swarm_engine_window_stats", fb.ctypes.data, w.ctypes.data)
    return fb, w


@pytest.mark.parametrize("E,n_species", [(1, 1), (3, 2)])
def test_cluster3_4096_bit_exact(E, n_species, path3):
    """4096 colloids at volume fraction ~0.04: every window passes the check (no re-run), three slices with new
    actions, positions / images / directors / velocities bit-exact."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(41)
    n = 4096
    lat = [_lattice3(rng, n) for _ in range(E)]
    L = lat[0][2]
    box = [L, L, L]
    sp = rng.integers(0, n_species, n)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 17, species_list()[:n_species], sp, n_envs=E,
                n_dims=3)
    states = [oracle.state3_from_positions(p, d, box) for p, d, _ in lat]
    h.upload(states)
    check = sorted({0, E - 1})
    step = 0
    for nsteps in (100, 100, 37):
        f = rng.choice([0.0, 10.0], E * n).astype(np.float32)
        tq = rng.normal(scale=5.0, size=(3, E * n)).astype(np.float32)
        h.set_actions(f, tq[2])
        h.set_torque_xy(tq[:2])
        h.integrate(nsteps)
        fb, waves = _stats(h)
        assert (fb == 0).all()  # check passed, no re-run
        assert (waves > 0).all() == (path3 == "cluster")
        got = h.download()
        vel = h.velocities()
        om = h.omegas3()
        for e in check:
            s = slice(e * n, (e + 1) * n)
            states[e], v, w = oracle.bd_run3(h.op, states[e], sp, f[s], tq[:, s], nsteps,
                                             step0=step, env=e)
            _eq3(got[e], states[e])
            assert np.array_equal(vel[:, s], v) and np.array_equal(om[:, s], w)
        step += nsteps


def test_cluster3_above_4096_colloids_bit_exact(monkeypatch):
    """One env of 4913 colloids (17^3): above 4096 the 3-D build sort takes 16
    colloids per thread (k_build_sort3<16>).  Two cluster windows of 5
    sub-steps, no re-run, bit-exact."""
    from gpu_harness import Harness, species_list

    monkeypatch.setenv("SWARMRL_AMD_NLIST", "0")
    rng = np.random.default_rng(43)
    n = 17 ** 3
    pos, d, L = _lattice3(rng, n)
    box = [L, L, L]
    sp = np.zeros(n, int)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 19, species_list()[:1], sp, n_dims=3)
    st = oracle.state3_from_positions(pos, d, box)
    h.upload([st])
    for w in range(2):
        f = rng.choice([0.0, 10.0], n).astype(np.float32)
        tq = rng.normal(scale=5.0, size=(3, n)).astype(np.float32)
        h.set_actions(f, tq[2])
        h.set_torque_xy(tq[:2])
        h.integrate(5)
        fb, waves = _stats(h)
        assert fb[0] == 0 and waves[0] > 0, (w, fb, waves)
        st, v, om = oracle.bd_run3(h.op, st, sp, f, tq, 5, step0=5 * w)
        _eq3(h.download()[0], st)
        assert np.array_equal(h.velocities(), v) and np.array_equal(h.omegas3(), om)


def test_cluster3_matches_global_path(monkeypatch):
    """The same engine run on the three 3-D paths (SWARMRL_AMD_CLUSTER_PATH=0
    forces the global one) gives the same bits."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(42)
    n = 2000
    pos, d, L = _lattice3(rng, n)
    box = [L, L, L]
    st = oracle.state3_from_positions(pos, d, box)
    f = rng.choice([0.0, 20.0], n).astype(np.float32)
    tq = rng.normal(scale=5.0, size=(3, n)).astype(np.float32)
    out = {}
    for path in ("1", "0", "nl"):
        monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "0" if path == "0" else "1")
        monkeypatch.setenv("SWARMRL_AMD_NLIST", "1" if path == "nl" else "0")
        h = Harness(box, 1e-3, 1.0239, 1.0239, 5, species_list()[:1], np.zeros(n, int),
                    n_dims=3)
        h.upload([st])
        h.set_actions(f, tq[2])
        h.set_torque_xy(tq[:2])
        h.integrate(150)
        out[path] = (h.download()[0], h.velocities(), h.omegas3(), _stats(h))
    for p in ("1", "nl"):
        _eq3(out[p][0], out["0"][0])
        assert np.array_equal(out[p][1], out["0"][1]) and np.array_equal(out[p][2], out["0"][2])
        assert out[p][3][0][0] == 0  # windowed path, check passed
    assert out["1"][3][1][0] > 0 and out["0"][3][1][0] == 0  # waves: cluster vs global


@pytest.mark.parametrize("kT", [0.0, 1.0239])
def test_global3_grid_of_two_cells(kT, monkeypatch):
    """k_global3 (the cluster path switched off) on a grid with two cells on an
    axis, where block_global_run3's stencil runs over both cells and has no
    wrap: 2 envs of 24 colloids of radius 1 on a 3 x 4 x 2 lattice in a periodic
    6 x 40 x 40 um box, columns 2 um apart, also through the periodic boundary;
    reuse_forces on, chunks of 12 and 1 sub-steps, against oracle.bd_run3, with
    noise and without (kT = 0: the update's noise-free arms).
    (More colloids than threads: test_nonperiodic_3d_bit_exact[global-2500].)
    The oracle runs first: WCA acted (the result differs from free swimming)."""
    from gpu_harness import Harness, species_list

    monkeypatch.setenv("SWARMRL_AMD_CLUSTER_PATH", "0")
    rng = np.random.default_rng(46)
    E, n, box, radius, species = 2, 24, [6.0, 40.0, 40.0], 1.0, species_list()[:1]
    g = np.stack(np.meshgrid(np.arange(3), np.arange(4), np.arange(2), indexing="ij"), -1)
    lattice = np.array([1.0, 12.0, 15.0]) + g.reshape(-1, 3) * np.array([2.0, 2.05, 2.05])
    sp = np.zeros(n, int)
    start = [oracle.state3_from_positions(lattice + rng.uniform(-0.1, 0.1, (n, 3)),
                                          rng.normal(size=(n, 3)), box) for _ in range(E)]
    op = oracle.make_params(box, 1e-3, kT, 1.0239, 13, species, n_dims=3)
    free_op = oracle.make_params(box, 1e-3, kT, 0.0, 13, species, n_dims=3)
    # on the CPU: two cells on x.  The 3-D grid (cell_grid3) takes or_cell_grid's
    # per-axis rule, floor(log2(6 / 2)) = 1 on x and 4 on y and z, and its cap of
    # max(n, 64) cells lowers only the largest axis, so it stops at 2 x 4 x 8 = 64
    # cells with x untouched.
    assert oracle.cell_grid(op, n, 2 * radius)[0] == 1
    assert 2 * 4 * 8 <= max(n, 64) < 2 * 8 * 8
    chunks = []
    refs = []
    tracks = [oracle.ReuseForces(s, dims=3) for s in start]
    free = start[0]
    free_track = oracle.ReuseForces(free, dims=3)
    states = list(start)
    step = 0
    for nsteps in (12, 1):
        f = rng.uniform(1.0, 4.0, E * n).astype(np.float32)
        tq = rng.normal(scale=5.0, size=(3, E * n)).astype(np.float32)
        chunks.append((nsteps, f, tq))
        out = []
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            states[e], v, w = tracks[e].run(op, states[e], sp, f[s], tq[:, s], nsteps, step0=step,
                                            env=e)
            out.append((states[e], v, w))
        free, _, _ = free_track.run(free_op, free, sp, f[:n], tq[:, :n], nsteps, step0=step)
        refs.append(out)
        step += nsteps
    assert not np.array_equal(free["q"], states[0]["q"])  # WCA acted
    h = Harness(box, 1e-3, kT, 1.0239, 13, species, sp, n_envs=E, n_dims=3, reuse=True)
    h.upload(start)
    for (nsteps, f, tq), out in zip(chunks, refs):
        h.set_actions(f, tq[2])
        h.set_torque_xy(tq[:2])
        h.integrate(nsteps)
        got, vel, om = h.download(), h.velocities(), h.omegas3()
        for e in range(E):
            s = slice(e * n, (e + 1) * n)
            _eq3(got[e], out[e][0])
            assert np.array_equal(vel[:, s], out[e][1]) and np.array_equal(om[:, s], out[e][2])
        fb, waves = _stats(h)
        assert (fb == 0).all() and (waves == 0).all(), (fb, waves)


def test_cluster3_reuse_one_substep_window(path3):
    """reuse_forces on the 3-D cluster path, including a window of one
    sub-step (its saved actions are this run's, not the reused ones)."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(43)
    n = 1500
    pos, d, L = _lattice3(rng, n)
    box = [L, L, L]
    st = oracle.state3_from_positions(pos, d, box)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 6, species_list()[:1], np.zeros(n, int), n_dims=3,
                reuse=True)
    h.upload([st])
    track = oracle.ReuseForces(st, dims=3)
    step = 0
    for nsteps in (100, 1, 1, 60):
        f = rng.normal(size=n).astype(np.float32) * 10
        tq = rng.normal(size=(3, n)).astype(np.float32) * 10
        h.set_actions(f, tq[2])
        h.set_torque_xy(tq[:2])
        h.integrate(nsteps)
        st, v, w = track.run(h.op, st, np.zeros(n), f, tq, nsteps, step0=step)
        step += nsteps
        _eq3(h.download()[0], st)
        assert np.array_equal(h.velocities(), v) and np.array_equal(h.omegas3(), w)
        fb, waves = _stats(h)
        assert fb[0] == 0 and (waves[0] > 0) == (path3 == "cluster")


def test_cluster3_rerun_and_big_cluster_bit_exact(path3):
    """A dense block of touching colloids (one cluster wider than a wave: the
    build flags the env) and fast swimmers (movers that fail the check) both
    re-run on the 3-D global path from the window-start snapshot."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(44)
    rest, _, L = _lattice3(rng, 1000, a=6.0, jitter=0.2)
    box = [L, L, L]
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1)
    block = 10.0 + 2.3 * g.reshape(-1, 3)  # 125 colloids within rc + skin of their neighbours
    rest = rest[np.min(np.linalg.norm(rest[:, None] - block[None], axis=2), axis=1) > 5.0]
    pos = np.concatenate([block, rest])
    n = len(pos)
    st = oracle.state3_from_positions(pos, rng.normal(size=(n, 3)), box)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 8, species_list()[:1], np.zeros(n, int), n_dims=3)
    h.upload([st])
    step = 0
    seen = set()
    for nsteps, fmax in ((100, 5.0), (100, 400.0)):
        f = rng.choice([0.0, fmax], n).astype(np.float32)
        tq = rng.normal(scale=5.0, size=(3, n)).astype(np.float32)
        h.set_actions(f, tq[2])
        h.set_torque_xy(tq[:2])
        h.integrate(nsteps)
        st, v, w = oracle.bd_run3(h.op, st, np.zeros(n), f, tq, nsteps, step0=step)
        step += nsteps
        _eq3(h.download()[0], st)
        assert np.array_equal(h.velocities(), v) and np.array_equal(h.omegas3(), w)
        seen.add(int(_stats(h)[0][0]))
    assert 2 in seen  # re-run on the global path


def test_cluster3_kt0_window_and_rerun_bit_exact(path3):
    """kT = 0 (the update's noise-free arms) on the windowed 3-D paths with
    WCA acting: 256 dimers, partners 1.6 um apart (inside the cutoff r_i + r_j
    of every species pair but 0.7 + 0.7), on a lattice 8 um apart, so clusters
    of two.
    Two windows of 40 sub-steps: with slow swimmers (f = 3) the check passes and
    the result is k_cluster_run3's or k_nl_step3's alone; with swimmers at
    f = 400 it fails and the window re-runs inside k_check3.
    The oracle runs first: in each window the result differs from the
    free-swimming one (WCA epsilon 0), so a pair force acted."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(47)
    k, a = 7, 8.0
    L = k * a
    box = [L, L, L]
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1)
    centre = (g.reshape(-1, 3)[:256] + 0.5) * a + rng.uniform(-0.3, 0.3, (256, 3))
    axis = rng.normal(size=(256, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    pos = np.concatenate([centre - 0.8 * axis, centre + 0.8 * axis])
    n = len(pos)
    sp = rng.integers(0, 2, n)
    start = oracle.state3_from_positions(pos, rng.normal(size=(n, 3)), box)
    op = oracle.make_params(box, 1e-3, 0.0, 1.0239, 10, species_list(), n_dims=3)
    free_op = oracle.make_params(box, 1e-3, 0.0, 0.0, 10, species_list(), n_dims=3)
    chunks, refs = [], []
    st, free = start, start
    for w, fmax in enumerate((3.0, 400.0)):
        f = rng.choice([0.0, fmax], n).astype(np.float32)
        tq = rng.normal(scale=5.0, size=(3, n)).astype(np.float32)
        before = st
        st, v, om = oracle.bd_run3(op, st, sp, f, tq, 40, step0=40 * w)
        free, _, _ = oracle.bd_run3(free_op, before, sp, f, tq, 40, step0=40 * w)
        assert not np.array_equal(free["q"], st["q"]), w  # WCA acted in this window
        chunks.append((f, tq))
        refs.append((st, v, om))
    h = Harness(box, 1e-3, 0.0, 1.0239, 10, species_list(), sp, n_dims=3)
    h.upload([start])
    codes = []
    for (f, tq), (ref, v, om) in zip(chunks, refs):
        h.set_actions(f, tq[2])
        h.set_torque_xy(tq[:2])
        h.integrate(40)
        _eq3(h.download()[0], ref)
        assert np.array_equal(h.velocities(), v) and np.array_equal(h.omegas3(), om)
        fb, waves = _stats(h)
        codes.append(int(fb[0]))
        assert (waves[0] > 0) == (path3 == "cluster")
    assert codes == [0, 2], codes  # the first window stood, the second re-ran


def test_cluster3_walls_bit_exact(path3):
    """Plane walls (espresso.py:667-711) on the 3-D cluster path."""
    from gpu_harness import Harness, species_list

    rng = np.random.default_rng(45)
    n = 1000
    pos, d, L = _lattice3(rng, n)
    box = [L, L, L]
    pos[:, 2] = 2.0 + (pos[:, 2] / L) * (L - 4.0)  # keep clear of the z walls at start
    st = oracle.state3_from_positions(pos, d, box)
    walls = [{"kind": 0, "normal": (0.0, 0.0, 1.0), "offset": 0.5},
             {"kind": 0, "normal": (0.0, 0.0, -1.0), "offset": -(L - 0.5)}]
    h = Harness(box, 1e-3, 1.0239, 1.0239, 9, species_list()[:1], np.zeros(n, int), n_dims=3)
    h.set_walls(walls)
    h.upload([st])
    f = np.full(n, 10.0, np.float32)
    tq = rng.normal(scale=5.0, size=(3, n)).astype(np.float32)
    h.set_actions(f, tq[2])
    h.set_torque_xy(tq[:2])
    h.integrate(200)
    ref, v, w = oracle.bd_run3(h.op, st, np.zeros(n), f, tq, 200, walls=walls)
    _eq3(h.download()[0], ref)
    assert np.array_equal(h.velocities(), v)
    fb, waves = _stats(h)
    assert (waves[0] > 0) == (path3 == "cluster")
