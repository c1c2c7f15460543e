"""
Ellipsoids on the GPU: k_ellipsoid_run (BD sub-steps and the overlap removal)
bit for bit against the CPU restatement tests/csrc/ellipsoid_oracle.c, the
reference's test_anisotropic through the product API, the displacement
statistics of the body-frame noise, a deep overlap, and the untouched sphere
path after an ellipsoid engine.
"""

import ctypes

import numpy as np
import pytest
import torch

import ellipsoid_oracle
from oracle import oracle

pytestmark = pytest.mark.gpu

TWO32 = 4294967296.0
KT = EPS = 1.0239
DT = 0.005
# (radius, gamma_par, gamma_r, mass, rinertia) and gamma_perp per species
SPECIES = [(0.5, 4.0, 6.0, 1.0e-6, 4.0e-7), (0.8, 6.0, 9.0, 2.0e-6, 9.0e-7)]
GAMMA_PERP = [7.0, 10.0]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _harness(box, species_of, n_envs, kappa, reuse=False, kT=KT, seed=17, n_species=1):
    """An engine through the C ABI with ellipsoids set, and the restatement's
    parameters."""
    from gpu_harness import Harness
    from swarmrl_amd import _capi

    h = Harness(list(box) if np.ndim(box) else [box, box, box], DT, kT, EPS, seed,
                SPECIES[:n_species], species_of,
                n_envs=n_envs, reuse=reuse)
    cell = _capi.SwarmEllipsoids()
    cell.aspect_ratio = kappa
    for s in range(n_species):
        cell.gamma_par[s], cell.gamma_perp[s] = SPECIES[s][1], GAMMA_PERP[s]
    h.native.call("swarm_engine_set_ellipsoids", ctypes.byref(cell))
    ell = ellipsoid_oracle.make_ellipsoids(kappa, [s[1] for s in SPECIES[:n_species]],
                                           GAMMA_PERP[:n_species])
    return h, ell


def _lattice(rng, n, box, jitter, lo=0.0):
    """n particles on a jittered square lattice over [lo, lo + box)^2 (folded
    into the box by the fixed-point conversion), random directors."""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    pos = np.stack([(k % side + 0.5), (k // side + 0.5)], 1) * (box / side)
    pos = lo + pos + rng.uniform(-jitter, jitter, (n, 2))
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    return (np.concatenate([pos, np.zeros((n, 1))], 1),
            np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1))


def _run_bit_exact(h, ell, states, species_of, reuse, slices=2, steps=10, sd_steps=0,
                   min_pairs=True):
    """(overlap removal,) then `slices` runs of `steps` sub-steps with a swim
    force and a torque; q, img, ang of every particle equal the restatement
    after every run.  Returns the restatement's statistics per env."""
    n = h.n
    sp = np.asarray(species_of, np.uint8)
    rng = np.random.default_rng(3)
    f_swim = rng.uniform(2.0, 6.0, n).astype(np.float32)
    torque = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    h.upload(states)
    if sd_steps:
        h.sd(sd_steps)
        done = [ellipsoid_oracle.sd_run(h.op, ell, st, sp, sd_steps) for st in states]
        states = [st for st, _ in done]
        _assert_equal(h, states)
    h.set_actions(np.tile(f_swim, h.E), np.tile(torque, h.E))
    prev = [ellipsoid_oracle.ReuseForces(st) for st in states]
    pairs, contacts, deep = np.zeros(h.E), np.zeros(h.E), 0
    for k in range(slices):
        h.integrate(steps)
        for e in range(h.E):
            if reuse:
                states[e], info = prev[e].run(h.op, ell, states[e], sp, f_swim, torque, steps,
                                              step0=k * steps, env=e)
            else:
                states[e], info = ellipsoid_oracle.bd_run(h.op, ell, states[e], sp, f_swim, torque,
                                                          steps, step0=k * steps, env=e)
            pairs[e] += info["torque_pairs"] / 2.0  # (counted from both sides)
            contacts[e] += info["pairs"] / 2.0
            deep += info["deep"]
        _assert_equal(h, states)
    # deep overlaps land in the engine's violation counter, one per visit
    assert h.wall_violations() == deep
    # the condition of the case: on average over the sub-steps at least N / 2
    # pairs inside the cutoff with a non-zero torque, in every env
    if min_pairs:
        assert np.all(pairs / (slices * steps) >= n / 2), (pairs / (slices * steps), n)
    return states, contacts / (slices * steps)


def _assert_equal(h, states):
    got = h.download()
    for e, st in enumerate(states):
        for k in ("q", "img", "ang"):
            assert np.array_equal(got[e][k], st[k]), (k, e)


def _states(rng, n, box, jitter, n_envs, lo=0.0):
    return [oracle.state_from_positions(*_lattice(rng, n, box, jitter, lo), [box] * 3)
            for _ in range(n_envs)]


@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("kappa", [3.0, 1.0 / 3.0])
def test_ellipsoid_run_bit_exact(kappa, reuse):
    """E = 2 x 96 spheroids of equatorial radius 0.5 (cutoff 6) in a 32 um
    box, noise on, 2 runs of 10 sub-steps: about a dozen partners inside the
    cutoff of each."""
    rng = np.random.default_rng(101)
    h, ell = _harness(32.0, np.zeros(96, int), 2, kappa, reuse=reuse)
    _run_bit_exact(h, ell, _states(rng, 96, 32.0, 0.9, 2), np.zeros(96, int), reuse)


def test_two_species_of_different_radii():
    """Radii 0.5 and 0.8: three different sigma0 and cutoffs (6, 7.8, 9.6),
    the grid that of the widest."""
    rng = np.random.default_rng(102)
    sp = (np.arange(96) % 3 == 0).astype(int)
    h, ell = _harness(40.0, sp, 2, 3.0, n_species=2)
    _run_bit_exact(h, ell, _states(rng, 96, 40.0, 0.8, 2), sp, False)


def test_more_particles_than_threads():
    """1100 particles in one env: a thread steps two of them."""
    rng = np.random.default_rng(103)
    h, ell = _harness(100.0, np.zeros(1100, int), 1, 3.0, reuse=True)
    _run_bit_exact(h, ell, _states(rng, 1100, 100.0, 0.7, 1), np.zeros(1100, int), True)


def test_pairs_across_the_periodic_boundary():
    """The lattice shifted by half a box: particles within one cutoff of both
    periodic boundaries, image counters on both sides."""
    rng = np.random.default_rng(104)
    h, ell = _harness(32.0, np.zeros(96, int), 2, 3.0)
    states = _states(rng, 96, 32.0, 0.9, 2, lo=16.0)
    assert states[0]["img"][:2].min() == 0 and states[0]["img"][:2].max() == 1
    cut = 6.0 / 32.0 * TWO32
    assert np.any(states[0]["q"][0] < cut) and np.any(states[0]["q"][0] > TWO32 - cut)
    _run_bit_exact(h, ell, states, np.zeros(96, int), False)


def test_grid_of_two_cells():
    """A 20 x 50 um box with the cutoff of 6: 2 x 8 cells, so both cells of a
    stencil row are one range and there is no wrap range.  16 prolate
    spheroids on a 4 x 4 lattice 5 um apart (also through the periodic
    boundary in x), jittered by 0.9."""
    rng = np.random.default_rng(107)
    n, box = 16, [20.0, 50.0, 50.0]
    h, ell = _harness(box, np.zeros(n, int), 2, 3.0, reuse=True)
    assert oracle.cell_grid(h.op, n, 6.0) == (1, 3)
    states = []
    for _ in range(2):
        k = np.arange(n)
        pos = np.stack([2.5 + 5.0 * (k % 4), 17.5 + 5.0 * (k // 4), np.zeros(n)], 1)
        pos[:, :2] += rng.uniform(-0.9, 0.9, (n, 2))
        th = rng.uniform(0.0, 2.0 * np.pi, n)
        states.append(oracle.state_from_positions(
            pos, np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1), box))
    _run_bit_exact(h, ell, states, np.zeros(n, int), True)


def test_spheres_with_per_axis_friction():
    """kGB = false: aspect ratio 1, gamma_par != gamma_perp, radius 0.5 on a
    1.2 um lattice jittered by 0.15: a few pairs overlap at the start (the
    overlap removal parts them) and swimmers collide in the run.  WCA has no
    torque, so the condition here is N / 10 pairs in contact per sub-step."""
    rng = np.random.default_rng(105)
    n, box = 100, 12.0
    h, ell = _harness(box, np.zeros(n, int), 2, 1.0)
    states = _states(rng, n, box, 0.15, 2)
    _, contacts = _run_bit_exact(h, ell, states, np.zeros(n, int), False, sd_steps=50,
                                 min_pairs=False)
    assert np.all(contacts >= n / 10), contacts


def test_overlap_removal_from_an_overlapping_start():
    """96 prolate spheroids dropped at random into a 28 um box: deep overlaps
    at the start; 100 steepest-descent steps with the Gay-Berne force and
    torque, then the sub-steps, equal the restatement."""
    rng = np.random.default_rng(106)
    n, box = 96, 28.0
    h, ell = _harness(box, np.zeros(n, int), 2, 3.0)
    states = []
    for _ in range(2):
        pos = np.concatenate([rng.uniform(0.0, box, (n, 2)), np.zeros((n, 1))], 1)
        th = rng.uniform(0.0, 2.0 * np.pi, n)
        states.append(oracle.state_from_positions(
            pos, np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1), [box] * 3))
    sp = np.zeros(n, np.uint8)
    _, info = ellipsoid_oracle.bd_run(h.op, ell, states[0], sp, np.zeros(n), np.zeros(n), 1)
    assert info["deep"] > 0  # (the start does overlap deeply)
    _run_bit_exact(h, ell, states, np.zeros(n, int), False, sd_steps=100)


def _product_engine(tmp_path, box, temperature, eps_scale=1.0, n_envs=1, dt=0.01):
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    params = MDParams(
        ureg=ureg,
        fluid_dyn_viscosity=ureg.Quantity(8.9e-4, "pascal * second"),
        WCA_epsilon=eps_scale * ureg.Quantity(300, "kelvin") * ureg.boltzmann_constant,
        temperature=ureg.Quantity(temperature, "kelvin"),
        box_length=ureg.Quantity(3 * [box], "micrometer"),
        time_step=ureg.Quantity(dt, "second"),
        time_slice=ureg.Quantity(10 * dt, "second"),
        write_interval=ureg.Quantity(10 * dt, "second"),
    )
    return ureg, params, SwarmEngine(params, n_dims=2, out_folder=tmp_path, write_chunk_size=1,
                                     n_envs=n_envs)


def _omega(eng):
    from swarmrl_amd.engine.swarm_view import wrap_device_pointer

    v = eng._device_views()
    torch.cuda.synchronize()
    return wrap_device_pointer(v.omega_z, (eng.n_envs * eng.n_particles,), torch.float32,
                               torch.device("cuda", 0)).cpu().numpy()


def test_reference_anisotropic_test_through_the_product_api(tmp_path):
    """CI/espresso_tests/unit_tests/test_espresso_2d.py:93-183: T = 0, one
    aspect-3 spheroid pointing along y, a constant force (1, 1): v = (1 /
    gamma_eq, 1 / gamma_ax); under ConstTorque omega = 1 / gamma_rot_eq.
    rtol 1e-6: two fp32 roundings and the constants' conversion, ~3 2^-24."""
    from swarmrl_amd import utils
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.units import ensure_quantity_array

    ureg, params, runner = _product_engine(tmp_path, 10000.0, 0.0, eps_scale=0.01)
    radius = ureg.Quantity(1, "micrometer")
    aspect_ratio = 3
    equatorial = radius / np.cbrt(aspect_ratio)
    axial = equatorial * aspect_ratio
    g_t_ax, g_t_eq = utils.calc_ellipsoid_friction_factors_translation(
        axial, equatorial, params.fluid_dyn_viscosity)
    g_r_ax, g_r_eq = utils.calc_ellipsoid_friction_factors_rotation(
        axial, equatorial, params.fluid_dyn_viscosity)
    partcl = runner.add_colloid_on_point(
        equatorial, ureg.Quantity(np.array([500, 500, 0]), "micrometer"),
        init_direction=np.array([0, 1, 0]),
        gamma_translation=ensure_quantity_array([g_t_eq, g_t_eq, g_t_ax], ureg),
        gamma_rotation=ensure_quantity_array([g_r_eq, g_r_eq, g_r_ax], ureg),
        aspect_ratio=aspect_ratio)
    runner.add_const_force_to_colloids(ureg.Quantity(np.array([1.0, 1.0, 0.0]), "sim_force"), 0)
    runner.integrate(10, ForceFunction({"0": dummy_models.ConstForce(force=0)}))
    np.testing.assert_allclose(
        partcl.v, [1 / g_t_eq.m_as("sim_force/sim_velocity"),
                   1 / g_t_ax.m_as("sim_force/sim_velocity"), 0], rtol=1e-6)
    runner.add_const_force_to_colloids(ureg.Quantity(np.zeros(3), "sim_force"), 0)
    runner.integrate(10, ForceFunction(
        {"0": dummy_models.ConstTorque(torque=np.array([0, 0, 1]))}))
    np.testing.assert_allclose(_omega(runner)[0],
                               1 / g_r_eq.m_as("sim_torque/sim_angular_velocity"), rtol=1e-6)
    runner.finalize()


def test_product_api_run_equals_the_restatement(tmp_path):
    """add_colloids / integrate end to end: 2 envs of 64 spheroids placed at
    random (overlapping), the engine's own overlap removal of 1000 steps and 2
    slices of 10 sub-steps with a ConstForce on the device path, equal the
    restatement built from the test's own numbers."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction

    ureg, params, eng = _product_engine(tmp_path, 40.0, 300.0, n_envs=2, dt=DT)
    g_par, g_perp, g_rot = 4.0, 7.0, 6.0
    eng.add_colloids(
        64, ureg.Quantity(0.5, "micrometer"), ureg.Quantity(np.array([20.0, 20.0, 0]), "micrometer"),
        ureg.Quantity(12.0, "micrometer"),
        gamma_translation=ureg.Quantity(np.array([1.0, g_perp, g_par]), "sim_force/sim_velocity"),
        gamma_rotation=ureg.Quantity(np.array([g_rot, 2.0, 3.0]),
                                     "sim_torque/sim_angular_velocity"),
        aspect_ratio=3.0)
    n = eng.n_particles
    (key,) = eng._species_keys
    p = oracle.make_params(eng._box, DT, eng._kT(), params.WCA_epsilon.m_as("sim_energy"),
                           eng.seed, [(0.5, g_par, g_rot, key[3], key[4])])
    ell = ellipsoid_oracle.make_ellipsoids(3.0, [g_par], [g_perp])
    sp = np.zeros(n, np.uint8)
    states = [oracle.state_from_positions(np.stack(eng._pos[e]), np.stack(eng._dir[e]), eng._box)
              for e in range(2)]
    states = [ellipsoid_oracle.sd_run(p, ell, st, sp, 1000)[0] for st in states]
    reuse = [ellipsoid_oracle.ReuseForces(st) for st in states]
    ff = ForceFunction({"0": dummy_models.ConstForce(5.0)})
    assert ff.supports_device()
    for k in range(2):
        eng.integrate(1, ff)
        got = eng.get_raw_state()
        for e in range(2):
            states[e], _ = reuse[e].run(p, ell, states[e], sp, np.full(n, 5.0), np.zeros(n), 10,
                                        step0=10 * k, env=e)
            for name in ("q", "img", "ang"):
                assert np.array_equal(got[name][..., e * n:(e + 1) * n], states[e][name]), (name, e)
    assert eng.step_count() == 20
    eng.finalize()


def test_displacement_variances_follow_the_frictions():
    """64 x 1024 ellipsoids on a 7 um lattice (cutoff 6: no pair interacts),
    one sub-step: var(along) / var(across) = gamma_perp / gamma_par within 3 %
    (five standard errors of sqrt(2 / 65536) on each variance)."""
    n, side = 1024, 32
    box = 7.0 * side
    h, ell = _harness(box, np.zeros(n, int), 64, 3.0)
    rng = np.random.default_rng(9)
    states = _states(rng, n, box, 0.2, 64)
    h.upload(states)
    h.set_actions(np.zeros(64 * n), np.zeros(64 * n))
    h.integrate(1)
    got = h.download()
    par, perp = [], []
    for st0, st1 in zip(states, got):
        d = (st1["q"][:2] - st0["q"][:2]).astype(np.int32).astype(np.float64) * (box / TWO32)
        th = st0["ang"].astype(np.float64) * (2.0 * np.pi / TWO32)
        par.append(d[0] * np.cos(th) + d[1] * np.sin(th))
        perp.append(-d[0] * np.sin(th) + d[1] * np.cos(th))
    par, perp = np.concatenate(par), np.concatenate(perp)
    np.testing.assert_allclose(par.var(), 2.0 * KT * DT / SPECIES[0][1], rtol=0.03)
    np.testing.assert_allclose(perp.var(), 2.0 * KT * DT / GAMMA_PERP[0], rtol=0.03)
    np.testing.assert_allclose(par.var() / perp.var(), GAMMA_PERP[0] / SPECIES[0][1], rtol=0.03)


def test_deep_overlap_is_finite_and_counted():
    """One side-by-side pair 0.3 sigma0 apart (X = 1 / 0.3 > 1.25): finite
    state after 5 sub-steps, a non-zero violation count, the restatement's."""
    box = 40.0
    h, ell = _harness(box, np.zeros(2, int), 1, 3.0, kT=0.0)
    sig0 = 2.0 ** (-1.0 / 6.0)
    pos = np.array([[20.0, 20.0, 0.0], [20.0 + 0.3 * sig0, 20.0, 0.0]])
    dirs = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    st = oracle.state_from_positions(pos, dirs, [box] * 3)
    h.upload([st])
    h.set_actions(np.zeros(2), np.zeros(2))
    h.integrate(5)
    want, info = ellipsoid_oracle.bd_run(h.op, ell, st, np.zeros(2, np.uint8), np.zeros(2),
                                         np.zeros(2), 5)
    _assert_equal(h, [want])
    assert info["deep"] > 0 and h.wall_violations() == info["deep"]
    assert np.all(np.isfinite(h.velocities()))
    sep = (want["q"][0, 1] - want["q"][0, 0]).astype(np.int32) * (box / TWO32)
    assert sep > 0.3 * sig0  # pushed apart


def test_setter_refuses_what_the_kernel_cannot_run():
    from gpu_harness import Harness
    from swarmrl_amd import _capi

    def ell(kappa=3.0, g=4.0):
        c = _capi.SwarmEllipsoids()
        c.aspect_ratio = kappa
        c.gamma_par[0], c.gamma_perp[0] = g, 7.0
        return c

    def make(**kw):
        return Harness([40.0] * 3, DT, KT, EPS, 1, SPECIES[:1], np.zeros(8, int), **kw)

    for bad in (ell(0.0), ell(-1.0), ell(g=0.0)):
        with pytest.raises(ValueError):
            make().native.call("swarm_engine_set_ellipsoids", ctypes.byref(bad))
    with pytest.raises(ValueError):
        make(n_dims=3).native.call("swarm_engine_set_ellipsoids", ctypes.byref(ell()))
    with pytest.raises(ValueError):
        make(periodic=False).native.call("swarm_engine_set_ellipsoids", ctypes.byref(ell()))
    h = make()
    h.integrate(1)
    with pytest.raises(RuntimeError):  # legal only before the first step
        h.native.call("swarm_engine_set_ellipsoids", ctypes.byref(ell()))
    big = Harness([400.0] * 3, DT, KT, EPS, 1, SPECIES[:1], np.zeros(4000, int))
    with pytest.raises(ValueError, match=r"at most 3\d\d\d particles"):
        big.native.call("swarm_engine_set_ellipsoids", ctypes.byref(ell()))
    ok = make()
    ok.native.call("swarm_engine_set_ellipsoids", ctypes.byref(ell()))
    with pytest.raises(ValueError):
        ok.set_walls([{"kind": 0, "normal": [1.0, 0.0, 0.0], "offset": 1.0}])
    deferred = ctypes.c_int32(7)
    ok.native.call("swarm_engine_defer_build", ctypes.byref(deferred))
    assert deferred.value == 0


def test_spheres_after_an_ellipsoid_engine_reproduce_the_golden_vectors():
    """An engine of plain spheres created after an ellipsoid engine in the
    same process runs the kernels it always ran: tests/golden/bd2d_wca.npz."""
    import pathlib

    from gpu_harness import Harness

    rng = np.random.default_rng(1)
    h, ell = _harness(32.0, np.zeros(96, int), 1, 3.0)
    h.upload(_states(rng, 96, 32.0, 0.9, 1))
    h.integrate(3)
    golden = pathlib.Path(__file__).resolve().parent / "golden" / "bd2d_wca.npz"
    with np.load(golden, allow_pickle=False) as f:
        z = {k: f[k] for k in f.files}
    species = [(1.0, 4.6595, 6.2126, 1.0358e-6, 4.143e-7), (0.7, 3.2617, 2.1309, 3.55e-7, 7.0e-8)]
    g = Harness(list(z["box"]), 1e-3, 1.0239, 1.0239, int(z["seed"]), species,
                z["species"].astype(int))
    g.upload([{"q": z["q0"], "img": z["img0"], "ang": z["ang0"]}])
    g.sd(int(z["sd_steps"]))
    g.set_actions(z["f_swim"], z["torque_z"])
    g.integrate(int(z["bd_steps"]))
    got = g.download()[0]
    for k in ("q", "img", "ang"):
        assert np.array_equal(got[k], z[k]), k
    assert np.array_equal(g.velocities(), z["vel"])
