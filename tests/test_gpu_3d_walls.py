"""
3-D dynamics and walls on the GPU against the CPU oracle.

3-D is the reference engine's default dimension (EspressoMD(n_dims=3),
espresso.py:143-152; free rotation about all axes, espresso.py:415-426).
Walls are espresso.py:667-800 (ShapeBasedConstraint + WCA with the
particle's radius as cutoff).  Deterministic parts are compared bit for bit
(positions, image counters, directors, velocities); the 3-D thermostat is
pinned statistically: MSD = 6 D_t t, <d(t).d(0)> = exp(-2 D_r t).
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


@pytest.mark.parametrize("kT", [0.0, 1.0239])
def test_bd3_wca_bit_exact(kT):
    from gpu_harness import Harness, random_state3, species_list

    rng = np.random.default_rng(31)
    n, E = 600, 2
    box = [22.0, 22.0, 22.0]
    sp = rng.integers(0, 2, n)
    h = Harness(box, 1e-3, kT, 1.0239, 9, species_list(), sp, n_envs=E, n_dims=3)
    states = [random_state3(rng, n, box) for _ in range(E)]
    h.upload(states)
    f = rng.choice([0.0, 10.0], E * n).astype(np.float32)
    tq = rng.normal(scale=5.0, size=(3, E * n)).astype(np.float32)
    h.set_actions(f, tq[2])
    h.set_torque_xy(tq[:2])
    h.integrate(150)
    got = h.download()
    vel = h.velocities()
    om = h.omegas3()
    for e in range(E):
        s = slice(e * n, (e + 1) * n)
        ref, v, w = oracle.bd_run3(h.op, states[e], sp, f[s], tq[:, s], 150, env=e)
        _eq3(got[e], ref)
        assert np.array_equal(vel[:, s], v) and np.array_equal(om[:, s], w)
        assert np.allclose(np.linalg.norm(ref["dir"], axis=0), 1.0, atol=1e-6)
    # overlaps existed, so WCA acted (positions differ from free swimming)
    free, _, _ = oracle.bd_run3(oracle.make_params(box, 1e-3, kT, 0.0, 9, species_list(),
                                                    n_dims=3),
                                states[0], sp, f[:n], tq[:, :n], 150, env=0)
    assert not np.array_equal(free["q"], got[0]["q"])


def test_sd3_bit_exact_and_counter():
    from gpu_harness import Harness, random_state3, species_list

    rng = np.random.default_rng(32)
    n = 400
    box = [14.0, 14.0, 14.0]
    h = Harness(box, 1e-3, 1.0239, 1.0239, 3, species_list()[:1], np.zeros(n, int), n_dims=3)
    st = random_state3(rng, n, box)
    h.upload([st])
    h.sd(200)
    ref, steps = oracle.sd_run3(h.op, st, np.zeros(n), 200)
    _eq3(h.download()[0], ref)
    assert steps > 10
    # SD does not consume noise: a following BD run starts at step 0
    h.set_actions(np.zeros(n), np.zeros(n))
    h.integrate(20)
    ref2, _, _ = oracle.bd_run3(h.op, ref, np.zeros(n), np.zeros(n), np.zeros((3, n)), 20)
    _eq3(h.download()[0], ref2)


def test_bd3_statistics():
    """Free 3-D diffusion (no WCA): MSD = 6 D_t t and <d(t).d(0)> =
    exp(-2 D_r t) within 4 standard errors."""
    from gpu_harness import Harness, random_state3

    rng = np.random.default_rng(33)
    n = 8000
    box = [400.0, 400.0, 400.0]
    gt, gr = 4.6595, 6.2126
    kT = 1.0239
    h = Harness(box, 1e-3, kT, 0.0, 4, [(1.0, gt, gr, 1.0, 1.0)], np.zeros(n, int), n_dims=3)
    st = random_state3(rng, n, box, lo=100.0, hi=300.0)
    h.upload([st])
    h.set_actions(np.zeros(n), np.zeros(n))
    steps = 500
    h.integrate(steps)
    got = h.download()[0]
    t = steps * 1e-3
    dx = oracle.unwrapped(got, box) - oracle.unwrapped(st, box)
    msd = np.mean(np.sum(dx ** 2, axis=1))
    exp_msd = 6 * kT / gt * t
    assert abs(msd - exp_msd) < 4 * exp_msd * np.sqrt(2 / 3 / n) * 1.5, (msd, exp_msd)
    corr = np.mean(np.sum(got["dir"] * st["dir"], axis=0))
    exp_corr = np.exp(-2 * kT / gr * t)
    assert abs(corr - exp_corr) < 0.02, (corr, exp_corr)


@pytest.mark.parametrize("dims", [2, 3])
def test_confining_walls_bit_exact(dims):
    """Box-face walls (add_confining_walls): swimmers pushed against x = L
    stay inside, bit-identical to the oracle; no wall contact is violated."""
    from gpu_harness import Harness, random_state, random_state3, species_list

    rng = np.random.default_rng(40 + dims)
    n = 300 if dims == 3 else 60  # dilute in either dimension
    box = [30.0, 30.0, 30.0]
    walls = [{"kind": 0, "normal": [1, 0, 0], "offset": 0.0},
             {"kind": 0, "normal": [-1, 0, 0], "offset": -30.0},
             {"kind": 0, "normal": [0, 1, 0], "offset": 0.0},
             {"kind": 0, "normal": [0, -1, 0], "offset": -30.0}]
    if dims == 3:
        walls += [{"kind": 0, "normal": [0, 0, 1], "offset": 0.0},
                  {"kind": 0, "normal": [0, 0, -1], "offset": -30.0}]
    h = Harness(box, 1e-3, 1.0239, 1.0239, 6, species_list()[:1], np.zeros(n, int),
                n_dims=dims)
    if dims == 3:
        st = random_state3(rng, n, box, lo=3.0, hi=27.0)
        st["dir"][:] = np.array([[1.0], [0.0], [0.0]], np.float32)
    else:
        st = random_state(rng, n, box, lo=3.0, hi=27.0)
        st["ang"][:] = 0
    h.upload([st])
    h.set_walls(walls)
    h.sd(100)
    f = np.full(n, 60.0, np.float32)
    h.set_actions(f, np.zeros(n, np.float32))
    h.integrate(400)
    got = h.download()[0]
    if dims == 3:
        ref, _ = oracle.sd_run3(h.op, st, np.zeros(n), 100, walls=walls)
        ref, _, _ = oracle.bd_run3(h.op, ref, np.zeros(n), f, np.zeros((3, n)), 400, walls=walls)
        _eq3(got, ref)
    else:
        ref, _ = oracle.sd_run(h.op, st, np.zeros(n), 100, walls=walls)
        ref, _, _ = oracle.bd_run(h.op, ref, np.zeros(n), f, np.zeros(n), 400, walls=walls)
        for k in ("q", "img", "ang"):
            assert np.array_equal(got[k], ref[k]), k
    pos = oracle.unwrapped(got, box, dims)
    assert np.all(pos[:, :dims] > 0.0) and np.all(pos[:, :dims] < 30.0)
    assert pos[:, 0].max() > 28.0  # pressed against the x = L wall
    assert h.wall_violations() == 0


def test_slab_walls_cluster_path_bit_exact():
    """add_walls slabs (vertical Rhomboids) around a square, 2-D, with enough
    colloids for the cluster path: wall forces inside the fused run kernel
    are bit-identical to the oracle, and the colloids stay inside."""
    from gpu_harness import Harness, random_state, species_list

    rng = np.random.default_rng(44)
    n = 2048
    box = [400.0, 400.0, 400.0]
    lo, hi, th = 100.0, 300.0, 2.0
    segs = [((lo, lo), (lo, hi)), ((lo, lo), (hi, lo)), ((hi, hi), (lo, hi)), ((hi, hi), (hi, lo))]
    walls = []
    for (x0, y0), (x1, y1) in segs:
        a = np.array([x1 - x0, y1 - y0, 0.0])
        b = np.cross(a / np.linalg.norm(a), [0, 0, 1.0]) * th
        walls.append({"kind": 1, "corner": [x0 - b[0] / 2, y0 - b[1] / 2, 0.0], "a": a, "b": b})
    h = Harness(box, 1e-3, 1.0239, 1.0239, 8, species_list()[:1], np.zeros(n, int))
    st = random_state(rng, n, box, lo=lo + 2.2, hi=hi - 2.2)
    h.upload([st])
    h.set_walls(walls)
    h.sd(200)
    ref, _ = oracle.sd_run(h.op, st, np.zeros(n), 200, walls=walls)
    f = rng.choice([0.0, 40.0], n).astype(np.float32)
    t = rng.choice([-10.0, 0.0, 10.0], n).astype(np.float32)
    h.set_actions(f, t)
    for w in range(3):
        h.integrate(100)
        ref, _, _ = oracle.bd_run(h.op, ref, np.zeros(n), f, t, 100, step0=100 * w, walls=walls)
        got = h.download()[0]
        for k in ("q", "img", "ang"):
            assert np.array_equal(got[k], ref[k]), k
    pos = oracle.unwrapped(got, box)
    assert np.all((pos[:, :2] > lo) & (pos[:, :2] < hi))
    assert h.wall_violations() == 0


def test_confining_walls_throughput_run_bit_exact(monkeypatch):
    """k_cluster_run<false, false, true, false>: the walls as its only variant
    flag (one species, no potential; SWARMRL_AMD_WIDE_RUN=0 for the
    throughput kernel and SWARMRL_AMD_NOISE_TABLE=0 for normals drawn in the
    kernel, which so small an engine would otherwise read from the table):
    two envs of 64 swimmers heading for x = L inside box-face walls, some of
    them in reach of it from the start, three windows on cluster waves
    without a re-run (0.21 um of drift a window, well below half the skin),
    bit-identical to the oracle, whose run without the walls differs."""
    from gpu_harness import Harness, species_list

    monkeypatch.setenv("SWARMRL_AMD_WIDE_RUN", "0")
    monkeypatch.setenv("SWARMRL_AMD_NOISE_TABLE", "0")
    rng = np.random.default_rng(47)
    E, k, a = 2, 8, 6.0
    n, L = k * k, k * a
    box = [L, L, L]
    walls = [{"kind": 0, "normal": [1, 0, 0], "offset": 0.0},
             {"kind": 0, "normal": [-1, 0, 0], "offset": -L},
             {"kind": 0, "normal": [0, 1, 0], "offset": 0.0},
             {"kind": 0, "normal": [0, -1, 0], "offset": -L}]
    h = Harness(box, 1e-3, 1.0239, 1.0239, 6, species_list()[:1], np.zeros(n, int), n_envs=E)
    # a jittered lattice shifted towards x = L and y = L: its last column and
    # row start within reach of those walls
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2)
    states = []
    for _ in range(E):
        pos = np.zeros((n, 3))
        pos[:, :2] = 1.2 + (g + 0.5) * a + rng.uniform(-1.0, 1.0, (n, 2))
        dirs = np.tile([1.0, 0.0, 0.0], (n, 1))
        states.append(oracle.state_from_positions(pos, dirs, box))
    h.upload(states)
    h.set_walls(walls)
    h.sd(100)
    refs = [oracle.sd_run(h.op, st, np.zeros(n), 100, walls=walls)[0] for st in states]
    free = refs[0]
    f = np.full(E * n, 10.0, np.float32)
    h.set_actions(f, np.zeros(E * n, np.float32))
    for w in range(3):
        h.integrate(100)
        got = h.download()
        for e in range(E):
            refs[e], _, _ = oracle.bd_run(h.op, refs[e], np.zeros(n), f[:n], np.zeros(n), 100,
                                          step0=100 * w, env=e, walls=walls)
            for k in ("q", "img", "ang"):
                assert np.array_equal(got[e][k], refs[e][k]), (w, e, k)
        free, _, _ = oracle.bd_run(h.op, free, np.zeros(n), f[:n], np.zeros(n), 100, step0=100 * w)
        fb, waves = h.window_stats()
        assert np.all(fb == 0) and np.all(waves > 0), (w, fb, waves)
    assert not np.array_equal(free["q"], refs[0]["q"])  # the walls were felt
    pos = oracle.unwrapped(got[0], box, 2)
    assert np.all(pos[:, :2] > 0.0) and np.all(pos[:, :2] < L)
    assert h.wall_violations() == 0


def test_wall_violation_is_counted():
    from gpu_harness import Harness, species_list

    n = 49  # a 7 x 7 lattice, spacing 3 (no overlaps, no motion at kT = 0)
    box = [50.0, 50.0, 50.0]
    h = Harness(box, 1e-3, 0.0, 1.0239, 1, species_list()[:1], np.zeros(n, int))
    gx, gy = np.meshgrid(16.0 + 3.0 * np.arange(7), 16.0 + 3.0 * np.arange(7))
    pos = np.stack([gx.ravel(), gy.ravel(), np.zeros(n)], 1)
    st = oracle.state_from_positions(pos, np.tile([1.0, 0.0, 0.0], (n, 1)), box)
    h.upload([st])
    # a slab covering the whole particle region: every particle is inside
    walls = [{"kind": 1, "corner": [10.0, 10.0, 0.0], "a": [30.0, 0.0, 0.0],
              "b": [0.0, 30.0, 0.0]}]
    h.set_walls(walls)
    h.set_actions(np.zeros(n), np.zeros(n))
    h.integrate(3)
    viol = np.zeros(1, np.uint64)
    oracle.bd_run(h.op, st, np.zeros(n), np.zeros(n), np.zeros(n), 3, walls=walls,
                  violations=viol)
    assert h.wall_violations() == int(viol[0]) == 3 * n
