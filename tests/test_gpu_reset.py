"""
In-place reset of chosen envs (swarm_engine_set_reset_plan,
swarm_engine_reset_envs; swarm_reset.cuh): the placement kernel bit for bit
against its numpy restatement (tests/reset_ref.py), the masked overlap removal
against the oracle's steepest descent per env, unlisted envs untouched to the
bit, the run that follows a reset against the oracle, the distribution of the
draws, the refusals, and SwarmEngine.reset_envs / EpisodicTrainer(...,
reset_in_place=True) through the product API.
"""

import ctypes

import numpy as np
import pytest
import torch

import potential_ref as pr
import reset_ref
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 42
WALLS = lambda L: [{"kind": 0, "normal": [1, 0, 0], "offset": 0.0},  # noqa: E731
                   {"kind": 0, "normal": [-1, 0, 0], "offset": -L},
                   {"kind": 0, "normal": [0, 1, 0], "offset": 0.0},
                   {"kind": 0, "normal": [0, -1, 0], "offset": -L}]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


# ------------------------------------------------------------------ helpers
def _harness(box, sp, E, dims=2, reuse=True, periodic=True, dt=1e-3):
    from gpu_harness import Harness, species_list

    return Harness(box, dt, 1.0239, 1.0239, SEED, species_list(), sp, n_envs=E, n_dims=dims,
                   reuse=reuse, periodic=periodic)


def _start(rng, E, n, box, dims, lo, hi):
    """Per env: fp64 positions and directors [n, 3] and their oracle state."""
    pos = np.zeros((E, n, 3))
    pos[:, :, :dims] = lo + rng.random((E, n, dims)) * (hi - lo)
    dirs = rng.normal(size=(E, n, 3))
    if dims == 2:
        dirs[:, :, 2] = 0.0
    fn = oracle.state3_from_positions if dims == 3 else oracle.state_from_positions
    return pos, dirs, [fn(pos[e], dirs[e], box) for e in range(E)]


def _set_plan(h, pos, dirs, groups):
    from swarmrl_amd import _capi

    arr = (_capi.SwarmResetGroup * max(1, len(groups)))()
    for k, (first, count, centre, radius) in enumerate(groups):
        arr[k].first, arr[k].count, arr[k].radius = first, count, radius
        for a in range(3):
            arr[k].centre[a] = centre[a]
    p = np.ascontiguousarray(pos, np.float64)
    d = np.ascontiguousarray(dirs, np.float64)
    h.native.bind_stream()
    h.native.call("swarm_engine_set_reset_plan", p.ctypes.data, d.ctypes.data,
                  ctypes.cast(arr, ctypes.c_void_p), len(groups))


def _reset(h, envs, sd_steps):
    h.native.bind_stream()
    if envs is None:
        h.native.call("swarm_engine_reset_envs", None, int(sd_steps), 0.1, 0.1)
        return
    mask = np.zeros(h.E, np.uint8)
    mask[list(envs)] = 1
    h.native.call("swarm_engine_reset_envs", mask.ctypes.data, int(sd_steps), 0.1, 0.1)


def _everything(h):
    """Every per-particle array a reset may write, as host copies."""
    from swarmrl_amd import _capi
    from swarmrl_amd.engine.swarm_view import wrap_device_pointer

    M = h.E * h.n
    st = h.download()
    out = {"q": np.concatenate([s["q"] for s in st], 1),
           "img": np.concatenate([s["img"] for s in st], 1),
           "ang": np.concatenate([s["ang"] for s in st])}
    if h.dims == 3:
        out["dir"] = np.concatenate([s["dir"] for s in st], 1)
    v = _capi.SwarmDeviceViews()
    _capi.check(h.native._lib.swarm_engine_device_views(h.native.ptr, ctypes.byref(v)))
    torch.cuda.synchronize()
    dev = torch.device("cuda", 0)
    views = {"vel": (v.vel, (3, M)), "omega": (v.omega_z, (M,)), "f_swim": (v.f_swim, (M,)),
             "torque_z": (v.torque_z, (M,))}
    if h.dims == 3:
        views.update({"omega_xy": (v.omega_xy, (2, M)), "torque_xy": (v.torque_xy, (2, M))})
    for k, (ptr, shape) in views.items():
        out[k] = wrap_device_pointer(ptr, shape, torch.float32, dev).cpu().numpy().copy()
    out["f_prev"] = np.zeros((2, M), np.float32)
    out["tz_prev"] = np.zeros((2, M), np.float32)
    out["ang_prev"] = np.zeros((2, M), np.uint32)
    d3 = t2 = None
    if h.dims == 3:
        out["dir3_prev"] = np.zeros((2, 3, M), np.float32)
        out["txy_prev"] = np.zeros((2, 2, M), np.float32)
        d3, t2 = out["dir3_prev"].ctypes.data, out["txy_prev"].ctypes.data
    h.native.call("swarm_engine_download_reuse_slots", out["f_prev"].ctypes.data,
                  out["tz_prev"].ctypes.data, out["ang_prev"].ctypes.data, d3, t2)
    return out


def _env(a, e, n):
    return a[..., e * n:(e + 1) * n]


def _assert_env_untouched(before, after, e, n):
    for k in before:
        assert np.array_equal(_env(before[k], e, n), _env(after[k], e, n)), (k, e)


def _assert_env_fresh(after, e, n, want, dims):
    """Env e holds `want` and what a fresh engine has beside it."""
    for k in ("q", "img") + (("dir",) if dims == 3 else ("ang",)):
        assert np.array_equal(_env(after[k], e, n), want[k]), (k, e)
    zero = ["vel", "omega", "f_swim", "torque_z", "f_prev", "tz_prev"]
    zero += ["omega_xy", "torque_xy", "txy_prev"] if dims == 3 else []
    for k in zero:
        assert not _env(after[k], e, n).any(), (k, e)
    for p in range(2):
        if dims == 3:
            assert np.array_equal(_env(after["dir3_prev"][p], e, n), want["dir"]), (p, e)
        else:
            assert np.array_equal(_env(after["ang_prev"][p], e, n), want["ang"]), (p, e)


def _stir(h, rng, dims):
    """A few slices with actions, so that velocities, actions and both
    reuse_forces slots (one window each) are non-zero."""
    M = h.E * h.n
    for _ in range(2):
        if dims == 3:
            h.set_torque_xy(rng.normal(size=(2, M)).astype(np.float32) * 5)
        h.set_actions(rng.uniform(1.0, 10.0, M).astype(np.float32),
                      rng.choice([-5.0, 5.0], M).astype(np.float32))
        h.integrate(10)
    got = _everything(h)
    for k in ("vel", "omega", "f_swim", "torque_z"):
        assert got[k].any(), k
    assert got["f_prev"][0].any() and got["f_prev"][1].any()
    return got


# --------------------------------------------------------- placement, 2-D
def test_place_2d_bit_exact_and_unlisted_env_untouched():
    """E = 3, N = 70, two species; a centred disc, a disc over the box corner
    (folded q, image counters of both signs), one particle in no group.
    Reset {0, 2}: env 1 identical to the bit in every array, envs 0 and 2 the
    restatement; a second reset draws with the next ordinal."""
    rng = np.random.default_rng(101)
    E, n, box = 3, 70, [40.0, 40.0, 40.0]
    sp = rng.integers(0, 2, n)
    h = _harness(box, sp, E)
    pos, dirs, states = _start(rng, E, n, box, 2, 2.0, 38.0)
    h.upload(states)
    h.sd(100)
    before = _stir(h, rng, 2)
    groups = [(0, 40, [20.0, 20.0, 0.0], 6.0), (40, 29, [37.0, 3.0, 0.0], 8.0)]
    _set_plan(h, pos, dirs, groups)
    assert np.array_equal(_everything(h)["q"], before["q"])  # the plan moves nothing

    for ordinal, envs in enumerate([(0, 2), (0, 2), (1,)]):
        _reset(h, envs, 0)
        after = _everything(h)
        for e in range(E):
            if e not in envs:
                _assert_env_untouched(before, after, e, n)
                continue
            want = reset_ref.place_env(box, 2, SEED, e, ordinal, states[e], groups)
            _assert_env_fresh(after, e, n, want, 2)
            # the particle in no group is home
            assert want["q"][0, 69] == states[e]["q"][0, 69]
            assert not np.array_equal(_env(after["q"], e, n)[:, :69],
                                      _env(before["q"], e, n)[:, :69])
        if ordinal == 0:
            img = _env(after["img"], 0, n)[:2, 40:69]
            assert (img > 0).any() and (img < 0).any() and (img == 0).any()
        before = after
    assert int(h.native._lib.swarm_engine_step_count(h.native.ptr)) == 20  # the noise goes on


# --------------------------------------------------------- placement, 3-D
@pytest.mark.parametrize("periodic", [True, False])
def test_place_3d_bit_exact(periodic):
    """E = 2, N = 70, a ball that reaches over the box face: folded with an
    image count in the periodic box, the same unwrapped position (image
    counter and all, as swarm_engine_upload_state keeps it) in the
    non-periodic one."""
    rng = np.random.default_rng(102)
    E, n, box = 2, 70, [40.0, 36.0, 44.0]
    sp = rng.integers(0, 2, n)
    h = _harness(box, sp, E, dims=3, periodic=periodic)
    pos, dirs, states = _start(rng, E, n, box, 3, 6.0, 30.0)
    h.upload(states)
    before = _stir(h, rng, 3)
    groups = [(1, 69, [36.0, 18.0, 22.0], 7.0)]
    _set_plan(h, pos, dirs, groups)
    for ordinal in range(2):
        _reset(h, (1,), 0)
        after = _everything(h)
        _assert_env_untouched(before, after, 0, n)
        want = reset_ref.place_env(box, 3, SEED, 1, ordinal, states[1], groups)
        _assert_env_fresh(after, 1, n, want, 3)
        assert np.array_equal(want["dir"][:, 0], states[1]["dir"][:, 0])  # particle 0: home
        assert (want["img"][0, 1:] == 1).any() and (want["img"][0, 1:] == 0).any()
        norm = np.linalg.norm(_env(after["dir"], 1, n).astype(np.float64), axis=0)
        assert np.all(np.abs(norm - 1.0) < 3e-7)  # three fp32 roundings
        before = after


# ------------------------------------------------- masked overlap removal
def _field(rng, shape, box, fmax, dims):
    h = np.asarray(box, float) / np.asarray(shape)
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    phi = (np.sin(2 * np.pi * (i + 0.5) / shape[0]) * np.cos(4 * np.pi * (j + 0.5) / shape[1])
           + 0.5 * np.cos(2 * np.pi * (k + 0.5) / shape[2]) + 0.02 * rng.normal(size=shape))
    g = [np.max(np.abs(np.roll(phi, -1, axis=a) - phi)) / h[a] for a in range(dims)]
    phi = (phi * (fmax / float(np.sqrt(np.sum(np.square(g)))))).astype(np.float32)
    return phi, h, pr.inv_spacing(h)


@pytest.mark.parametrize("dims,periodic", [(2, True), (2, False), (3, True)])
def test_masked_overlap_removal_matches_the_oracle_per_env(dims, periodic):
    """Dense groups, so the placement overlaps; reset {0, 2} with 200 steps:
    those envs equal the oracle's steepest descent from the restated
    placement (the gridded potential acting), env 1 -- uploaded with
    overlaps, under the same potential -- does not move.  2-D periodic: the
    LDS body; 2-D non-periodic: the global body; 3-D: k_global3_envs."""
    rng = np.random.default_rng(103 + dims + periodic)
    E, n = 3, 70
    box = [40.0, 40.0, 40.0] if dims == 2 else [30.0, 30.0, 30.0]
    sp = rng.integers(0, 2, n)
    h = _harness(box, sp, E, dims=dims, periodic=periodic)
    c = box[0] / 2
    pos, dirs, states = _start(rng, E, n, box, dims, c - 3.0, c + 3.0)  # overlapping
    h.upload(states)
    shape = (23, 19, 1) if dims == 2 else (13, 11, 9)
    phi, spacing, inv_h = _field(rng, shape, box, 2.0, dims)
    p = np.ascontiguousarray(phi, np.float32)
    s = np.ascontiguousarray(spacing, np.float64)
    h.native.bind_stream()
    h.native.call("swarm_engine_set_potential_field", p.ctypes.data, p.shape[0], p.shape[1],
                  p.shape[2], s.ctypes.data)
    groups = [(0, 45, [c - 2.0, c, c if dims == 3 else 0.0], 5.0),
              (45, 24, [c + 6.0, c + 1.0, c if dims == 3 else 0.0], 3.0)]
    _set_plan(h, pos, dirs, groups)
    before = _everything(h)
    _reset(h, (0, 2), 200)
    after = _everything(h)
    _assert_env_untouched(before, after, 1, n)
    moved = 0
    for e in (0, 2):
        placed = reset_ref.place_env(box, dims, SEED, e, 0, states[e], groups)
        want = pr.sd_run_potential(h.op, placed, sp, 200, phi, inv_h, dims=dims)
        _assert_env_fresh(after, e, n, want, dims)
        moved += int((want["q"] != placed["q"]).sum())
    assert moved > n  # the placement did overlap
    # and env 1 would have moved: the existing overlap removal moves it
    h.sd(5)
    assert not np.array_equal(_env(_everything(h)["q"], 1, n), _env(before["q"], 1, n))


@pytest.mark.parametrize("dims", [2, 3])
def test_reset_of_all_envs_equals_placement_then_remove_overlap(dims):
    """reset_envs(NULL, S) == reset_envs(NULL, 0) + swarm_engine_remove_overlap(S)
    bit for bit: k_global_envs / k_global3_envs against k_global / k_global3."""
    n, E = 70, 3
    box = [40.0, 40.0, 40.0] if dims == 2 else [30.0, 30.0, 30.0]
    c = box[0] / 2
    out = []
    for split in (False, True):
        rng = np.random.default_rng(104)
        sp = rng.integers(0, 2, n)
        h = _harness(box, sp, E, dims=dims)
        pos, dirs, states = _start(rng, E, n, box, dims, 4.0, box[0] - 4.0)
        h.upload(states)
        _stir(h, rng, dims)
        _set_plan(h, pos, dirs, [(0, n, [c, c, c if dims == 3 else 0.0], 5.0)])
        if split:
            _reset(h, None, 0)
            h.sd(150)
        else:
            _reset(h, None, 150)
        out.append(_everything(h))
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    placed = reset_ref.place_env(box, dims, SEED, 0, 0, states[0],
                                 [(0, n, [c, c, c if dims == 3 else 0.0], 5.0)])
    assert not np.array_equal(_env(out[0]["q"], 0, n), placed["q"])  # the descent ran


# ---------------------------------------------------------------- going on
def test_run_after_reset_matches_the_oracle_on_the_cluster_path():
    """reuse_forces, confining walls, the cluster windows: after a reset of
    {1} with its overlap removal, two runs of 25 sub-steps equal the oracle in
    every env -- env 1 from its post-reset state with no previous forces, the
    noise at the engine's step count; envs 0 and 2 go on as if nothing
    happened."""
    rng = np.random.default_rng(105)
    E, n, L = 3, 70, 60.0
    box = [L, L, L]
    sp = rng.integers(0, 2, n)
    h = _harness(box, sp, E)
    walls = WALLS(L)
    h.set_walls(walls)
    pos, dirs, states = _start(rng, E, n, box, 2, 6.0, 54.0)
    h.upload(states)
    h.sd(100)
    cur = [oracle.sd_run(h.op, s, sp, 100, walls=walls)[0] for s in states]
    track = [oracle.ReuseForces(s) for s in cur]
    step = 0

    def run(k):
        nonlocal step
        f = rng.uniform(1.0, 10.0, E * n).astype(np.float32)
        t = rng.choice([-5.0, 0.0, 5.0], E * n).astype(np.float32)
        h.set_actions(f, t)
        h.integrate(k)
        got = h.download()
        for e in range(E):
            sl = slice(e * n, (e + 1) * n)
            cur[e], _, _ = track[e].run(h.op, cur[e], sp, f[sl], t[sl], k, step0=step, env=e,
                                        walls=walls)
            for key in ("q", "img", "ang"):
                assert np.array_equal(got[e][key], cur[e][key]), (key, e, step)
        step += k

    run(25)
    run(25)
    groups = [(0, n, [30.0, 30.0, 0.0], 12.0)]
    _set_plan(h, pos, dirs, groups)
    _reset(h, (1,), 100)
    placed = reset_ref.place_env(box, 2, SEED, 1, 0, states[1], groups)
    cur[1] = oracle.sd_run(h.op, placed, sp, 100, walls=walls)[0]
    track[1] = oracle.ReuseForces(cur[1])
    assert int(h.native._lib.swarm_engine_step_count(h.native.ptr)) == step == 50
    run(25)
    run(25)
    fb, waves = h.window_stats()
    # the cluster windows ran (env 1's dense disc may be one cluster wider
    # than a wave, which the check runs: its waves are not asserted)
    assert waves[0] > 0 and waves[2] > 0 and fb[0] == 0 and fb[2] == 0


# ------------------------------------------------------------ distribution
def _distribution_ok(st, dims, box, centre, R):
    """The issue's bounds, five standard deviations of each estimator over
    16 384 samples: inside the radius up to one fixed-point step; the share
    within the half-measure radius 0.5 +- 0.02 (sigma = 0.5 / 128); the means
    of the director's components and of the polar direction 0 +- 0.03
    (sigma <= sqrt(1/2) / 128)."""
    d = oracle.unwrapped(st, box, dims)[:, :dims] - np.asarray(centre)[:dims]
    r = np.linalg.norm(d, axis=1)
    assert np.all(r <= R + max(box) / 2.0 ** 32)
    inner = R / np.sqrt(2.0) if dims == 2 else R * 2.0 ** (-1.0 / 3.0)
    assert abs(np.mean(r <= inner) - 0.5) <= 0.02
    if dims == 2:
        sn, cs = reset_ref.sincos_turn(st["ang"])
        u = np.stack([cs, sn], 1).astype(np.float64)
    else:
        u = st["dir"].T.astype(np.float64)
    assert np.all(np.abs(u.mean(axis=0)) <= 0.03)
    assert np.all(np.abs((d / r[:, None]).mean(axis=0)) <= 0.03)


@pytest.mark.parametrize("dims", [2, 3])
def test_distribution_of_one_placement(dims):
    """4 x 4096 particles, one placement: the restatement passes the bounds
    alone, and the device holds the restatement."""
    rng = np.random.default_rng(106)
    E, n = 4, 4096
    box = [300.0, 300.0, 300.0] if dims == 2 else [120.0, 120.0, 120.0]
    centre, R = ([140.0, 160.0, 0.0], 110.0) if dims == 2 else ([60.0, 55.0, 65.0], 50.0)
    h = _harness(box, np.zeros(n, int), E, dims=dims)
    pos, dirs, states = _start(rng, E, n, box, dims, 10.0, 100.0)
    h.upload(states)
    groups = [(0, n, centre, R)]
    _set_plan(h, pos, dirs, groups)
    _reset(h, None, 0)
    got = h.download()
    ref = [reset_ref.place_env(box, dims, SEED, e, 0, states[e], groups) for e in range(E)]
    keys = ("q", "img") + (("dir",) if dims == 3 else ("ang",))
    allref = {k: np.concatenate([r[k] for r in ref], axis=-1) for k in keys}
    _distribution_ok(allref, dims, box, centre, R)
    for e in range(E):
        for k in keys:
            assert np.array_equal(got[e][k], ref[e][k]), (k, e)


# ---------------------------------------------------------------- refusals
def test_refusals():
    from swarmrl_amd import _capi

    rng = np.random.default_rng(107)
    E, n, box = 2, 20, [40.0, 40.0, 40.0]
    sp = np.zeros(n, int)
    pos, dirs, states = _start(rng, E, n, box, 2, 2.0, 38.0)

    h = _harness(box, sp, E)
    h.upload(states)
    with pytest.raises(RuntimeError, match="reset plan"):  # SWARM_ESTATE
        _reset(h, None, 0)
    c = [20.0, 20.0, 0.0]
    for bad in ([(0, 12, c, 5.0), (10, 5, c, 5.0)],       # overlapping
                [(15, 6, c, 5.0)], [(-1, 3, c, 5.0)],      # out of range
                [(0, 5, c, -1.0)], [(0, 5, c, float("nan"))], [(0, 5, c, float("inf"))],
                [(0, 5, c, 20.5)]):                         # wider than the box
        with pytest.raises(ValueError):                     # SWARM_EINVAL
            _set_plan(h, pos, dirs, bad)
    with pytest.raises(RuntimeError, match="reset plan"):   # a refused plan is no plan
        _reset(h, None, 0)
    _set_plan(h, pos, dirs, [(0, 5, c, 5.0)])
    before = _everything(h)
    h.native.call("swarm_engine_reset_envs", np.zeros(E, np.uint8).ctypes.data, 10, 0.1, 0.1)
    after = _everything(h)
    for k in before:                                        # an empty mask: a no-op
        assert np.array_equal(before[k], after[k]), k
    with pytest.raises(ValueError):
        _reset(h, None, -1)

    def refused(prepare, dt=1e-3):
        hh = _harness(box, sp, E, reuse=False, dt=dt)
        hh.upload(states)
        prepare(hh)
        _set_plan(hh, pos, dirs, [(0, 5, c, 5.0)])
        with pytest.raises(ValueError, match="rod, ellipsoids or the Langevin"):
            _reset(hh, None, 0)

    rod = _capi.SwarmRod()
    rod.first, rod.n, rod.delta, rod.fixed = 0, 5, 1.0, 1
    refused(lambda hh: hh.native.call("swarm_engine_set_rod", ctypes.byref(rod)))
    ell = _capi.SwarmEllipsoids()
    ell.aspect_ratio = 1.0
    for s in range(2):
        ell.gamma_par[s], ell.gamma_perp[s] = 4.0, 6.0
    refused(lambda hh: hh.native.call("swarm_engine_set_ellipsoids", ctypes.byref(ell)))
    # (a step the explicit friction integrates: dt gamma / m < 2)
    refused(lambda hh: hh.native.call("swarm_engine_set_langevin"), dt=5e-8)


# ----------------------------------------------------------------- product
def _md_params(ureg, L, **kw):
    from swarmrl_amd.engine import MDParams

    return MDParams(ureg=ureg, box_length=ureg.Quantity([L, L, L], "micrometer"),
                    time_step=ureg.Quantity(1e-3, "second"), **kw)


def test_engine_reset_envs(tmp_path):
    """A 2-env SwarmEngine with add_colloids and one add_colloid_on_point:
    reset_envs([1]) leaves env 0 as it is; env 1 lies in its disc, free of
    overlaps, with its point colloid home."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.engine import SwarmEngine
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    um = lambda v: ureg.Quantity(v, "micrometer")  # noqa: E731
    L, n = 60.0, 40
    eng = SwarmEngine(_md_params(ureg, L, time_slice=ureg.Quantity(1e-2, "second"),
                                 write_interval=ureg.Quantity(1e-2, "second")),
                      n_dims=2, seed=9, out_folder=tmp_path, n_envs=2)
    with pytest.raises(RuntimeError):
        eng.reset_envs()
    eng.add_colloids(n, um(1.0), um(np.array([25.0, 30.0, 0.0])), um(14.0), type_colloid=0)
    eng.add_colloid_on_point(um(1.0), um(np.array([50.0, 50.0, 0.0])), np.array([0.0, 1.0, 0.0]),
                             type_colloid=1)
    ff = ForceFunction({"0": dummy_models.ConstForce(5.0), "1": dummy_models.ConstForce(5.0)})
    eng.integrate(3, ff)
    N = n + 1
    before = eng.get_raw_state(velocities=True)
    t0, steps0 = eng.system.time, eng.step_count()
    eng.reset_envs([1])
    after = eng.get_raw_state(velocities=True)
    for k in before:
        assert np.array_equal(before[k][..., :N], after[k][..., :N]), k
    assert not np.array_equal(before["q"][:, N:], after["q"][:, N:])
    assert not after["vel"][:, N:].any()
    assert eng.system.time == t0 and eng.step_count() == steps0  # the clocks go on
    pos = eng.get_particle_data()["Unwrapped_Positions"][1]
    np.testing.assert_allclose(pos[n], [50.0, 50.0, 0.0], atol=1e-6)
    d = pos[:n, :2] - [25.0, 30.0]
    # placed inside 14; the overlap removal moves a colloid 0.1 a step at most
    assert np.all(np.hypot(d[:, 0], d[:, 1]) <= 14.0 + 3.0)
    gap = np.linalg.norm(pos[:, None, :2] - pos[None, :, :2], axis=2) + 10.0 * np.eye(N)
    assert gap.min() > 1.9  # no overlap left (contact at 2)
    eng.integrate(2, ff)  # and the engine goes on
    assert eng.step_count() == steps0 + 2 * eng.params.steps_per_slice
    eng.finalize()


class _Recorder:
    """Mixin: keeps every reward tensor the task hands out."""

    def __call__(self, colloids):
        r = super().__call__(colloids)
        self.seen.append(torch.as_tensor(r).detach().cpu().numpy().copy())
        return r


def test_episodic_trainer_reset_in_place(tmp_path):
    """3 episodes at reset_frequency = 1 on one engine: get_engine is called
    once, rewards are finite, the first slice after a reset pays no more than
    one slice's motion can (a task history left at the old episode's
    positions would pay for the jump to the new start), and the trajectory
    holds one group per cycle."""
    from swarmrl_amd.actions import Action
    from swarmrl_amd.agents import ActorCriticAgent
    from swarmrl_amd.engine import SwarmEngine, trajectory_writer
    from swarmrl_amd.networks import ActorCriticMLP, TorchModel
    from swarmrl_amd.observables import SubdividedVisionCones
    from swarmrl_amd.tasks.searching import GradientSensing
    from swarmrl_amd.trainers import EpisodicTrainer
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    n, L, slices = 200, 100.0, 4
    made = []

    def get_engine(system, tag):
        eng = SwarmEngine(_md_params(ureg, L, time_slice=ureg.Quantity(0.1, "second"),
                                     write_interval=ureg.Quantity(0.2, "second")),
                          n_dims=2, seed=42, out_folder=tmp_path, write_chunk_size=1, n_envs=2,
                          h5_group_tag=tag)
        eng.add_colloids(n, ureg.Quantity(1.0, "micrometer"),
                         ureg.Quantity(np.array([L / 2, L / 2, 0.0]), "micrometer"),
                         ureg.Quantity(L / 2 - 2, "micrometer"), type_colloid=1)
        made.append(eng)
        return eng

    class Task(_Recorder, GradientSensing):
        seen = []

    scale = 10
    task = Task(np.array([L / 2, L / 2, 0]), lambda d: 1 - d, np.array([L, L, L]), scale,
                particle_type=1)
    net = TorchModel(ActorCriticMLP(3, 4, 32), input_shape=(3,), rng_key=3)
    force = 10.0
    actions = {"a": Action(torque=np.array([0, 0, 10.0])), "b": Action(force=force),
               "c": Action(torque=np.array([0, 0, -10.0])), "d": Action()}
    agent = ActorCriticAgent(1, net, task,
                             SubdividedVisionCones(10.0, np.pi / 2, 3, [1.0] * n, particle_type=1),
                             actions)
    agent.loss.n_epochs = 2
    trainer = EpisodicTrainer([agent])
    rewards = trainer.perform_rl_training(get_engine, None, n_episodes=3, episode_length=slices,
                                          reset_frequency=1, load_bar=False,
                                          reset_in_place=True)
    assert len(made) == 1 and trainer.engine is made[0]
    assert rewards.shape == (4,) and np.all(np.isfinite(rewards))
    eng = made[0]
    # one slice's motion: the swim speed F / gamma_t for the slice, eight
    # standard deviations of its diffusion, twice over for contacts; the
    # reward is scale * (distance moved towards the source) / L at most
    gamma_t, _ = eng.get_friction_coefficients(1)
    T = eng.params.steps_per_slice * eng._time_step
    move = 2.0 * (force / gamma_t * T + 8.0 * np.sqrt(2.0 * eng._kT() / gamma_t * T))
    assert scale * move / L < 1.0  # (a jump across the disc pays ~ scale * 48 / L)
    assert len(task.seen) == 3 * slices
    for r in task.seen:
        assert np.all(np.isfinite(r)) and r.max() <= scale * move / L
    assert trajectory_writer.read_groups(eng.h5_filename) == ["0", "1", "2"]


def test_headline_schedule_across_a_reset_matches_the_oracle():
    """The headline's slice schedule (bench.build_workload at 1024 colloids:
    vision cone, fused policy, the next window's build riding in the
    observable launches, the pair search filtering the candidate lists of the
    last run) through a reset_envs(): the lists of the old positions must not
    be used for the new ones.  Rewards of every slice and the final state
    against the oracle's replay of the recorded actions, the reset restated
    as placement + 1000 steps of steepest descent."""
    import argparse
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    dev = torch.device("cuda", 0)
    N = 1024
    ns = argparse.Namespace(colloids=N, envs_per_gpu=1, write_interval=1.0)
    eng, ff, agent = bench.build_workload(ns, SEED, dev)
    pos0, dir0 = np.stack(eng._pos[0]), np.stack(eng._dir[0])

    def block():
        t = agent.trajectory
        return {k: [torch.as_tensor(x).detach().cpu().numpy().copy() for x in getattr(t, k)]
                for k in ("actions", "rewards")}

    def build_stats():
        stats = (ctypes.c_uint64 * 4)()
        eng._native.call("swarm_engine_build_stats", stats, 0)
        return list(stats)  # windows that filtered lists, that waited, re-runs, windows

    eng.integrate(3, ff)
    first = block()
    before = build_stats()
    agent.reset_trajectory()
    eng.reset_envs()
    agent.reset_agent(eng.colloids)
    eng.integrate(3, ff)
    second = block()
    got = eng.get_raw_state()
    after = build_stats()

    L = float(eng._box[0])
    box, src = np.array([L, L, L]), np.array([L / 2, L / 2, 0.0])
    p = oracle.make_params(eng._box, eng._time_step, eng._kT(),
                           eng.params.WCA_epsilon.m_as("sim_energy"), SEED, [eng._species_keys[0]])
    agents, sp = np.arange(N), np.zeros(N, np.uint8)
    ftab = np.array([0.0, 10.0, 0.0, 0.0], np.float32)
    ttab = np.array([10.0, 0.0, -10.0, 0.0], np.float32)
    f32 = np.float32
    home = oracle.state_from_positions(pos0, dir0, eng._box)
    step = 0
    for k, blk in enumerate((first, second)):
        if k == 0:
            hist = oracle.history_from_state(home, agents)  # the task saw the start
            st = home
        else:
            st = reset_ref.place_env(list(eng._box), 2, SEED, 0, 0, home, eng._reset_groups)
        st, _ = oracle.sd_run(p, st, sp, 1000)
        if k == 1:
            hist = oracle.history_from_state(st, agents)  # reset_agent after the reset
        prev = {"f": np.zeros(N, f32), "t": np.zeros(N, f32), "ang": st["ang"].copy()}
        assert len(blk["actions"]) == 3
        for s in range(3):
            idx = blk["actions"][s].reshape(-1)
            f, t = ftab[idx], ttab[idx]
            st, _, _ = oracle.bd_run(p, st, sp, f, t, 100, step0=100 * step, prev=prev)
            prev = {"f": f, "t": t, "ang": st["ang"].copy()}
            dc, dp = oracle.field_distance(p, st, agents, src, box, hist, update=True)
            v = (f32(10.0) * ((f32(1.0) - dc) - (f32(1.0) - dp))).astype(f32)
            rew = np.where(v < 0, f32(0), v).astype(f32)
            assert np.array_equal(blk["rewards"][s].reshape(-1), rew), (k, s, "reward")
            step += 1
    for key in ("q", "img", "ang"):
        assert np.array_equal(got[key], st[key]), key
    # every window's pair search ran as a filter of lists or behind the fresh
    # sort; the lists were in use before the reset, and the first window
    # after it cannot have used them
    assert before[3] == 3 and before[0] >= 1 and before[0] + before[1] == 3, before
    assert after[3] == 6 and after[0] + after[1] == 6 and after[1] > before[1], (before, after)
    eng.finalize()
