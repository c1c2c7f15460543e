"""
Ellipsoids without a GPU: the Python surface and its errors, the friction
helpers against the reference functions' recorded outputs, the fp64 statement
of the Gay-Berne pair (tests/ellipsoid_ref.py) against itself, the fp32
restatement (tests/csrc/ellipsoid_oracle.c) against the fp64 statement, and
known answers of the restatement's body-frame step.
"""

import numpy as np
import pytest

import ellipsoid_oracle
import ellipsoid_ref
from conftest import ROOT
from oracle import oracle

TWO32 = 4294967296.0
EPS0, RADIUS = 0.1, 1.0
SIGMA0 = 2.0 * RADIUS * 2.0 ** (-1.0 / 6.0)


def _engine(tmp_path, n_dims=2, temperature=300.0):
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    params = MDParams(
        ureg=ureg,
        box_length=ureg.Quantity(3 * [100.0], "micrometer"),
        temperature=ureg.Quantity(temperature, "kelvin"),
        time_step=ureg.Quantity(0.01, "second"),
        time_slice=ureg.Quantity(0.1, "second"),
        write_interval=ureg.Quantity(0.1, "second"),
    )
    return ureg, SwarmEngine(params, n_dims=n_dims, out_folder=tmp_path, write_chunk_size=1)


def _add(ureg, eng, aspect_ratio=3.0, type_colloid=0, x=50.0, gt=(2.0, 3.0, 1.5),
         gr=(4.0, 5.0, 6.0)):
    return eng.add_colloid_on_point(
        ureg.Quantity(1.0, "micrometer"), ureg.Quantity(np.array([x, 50.0, 0.0]), "micrometer"),
        np.array([0.0, 1.0, 0.0]), type_colloid=type_colloid,
        gamma_translation=ureg.Quantity(np.array(gt), "sim_force / sim_velocity"),
        gamma_rotation=ureg.Quantity(np.array(gr), "sim_torque / sim_angular_velocity"),
        aspect_ratio=aspect_ratio)


# ------------------------------------------------------------ Python surface
def test_aspect_ratio_and_per_axis_friction_are_accepted(tmp_path):
    """aspect_ratio = 3 with 3-vector frictions: registered as the reference
    does, the species carries gamma_translation[2] along the director,
    gamma_translation[1] across it and gamma_rotation[0] about lab z."""
    ureg, eng = _engine(tmp_path)
    _add(ureg, eng)
    assert eng.colloid_radius_register == {0: {"radius": 1.0, "aspect_ratio": 3.0}}
    (key,) = eng._species_keys
    assert key[1] == 1.5 and key.gamma_perp == 3.0 and key[2] == 4.0
    assert eng._has_ellipsoids()
    eng.add_colloids(3, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(np.array([50.0, 50.0, 0.0]), "micrometer"),
                     ureg.Quantity(20.0, "micrometer"),
                     gamma_translation=ureg.Quantity(np.array([2.0, 3.0, 1.5]),
                                                     "sim_force / sim_velocity"),
                     gamma_rotation=ureg.Quantity(np.array([4.0, 5.0, 6.0]),
                                                  "sim_torque / sim_angular_velocity"),
                     aspect_ratio=3.0)
    assert len(eng._species_keys) == 1 and eng.n_particles == 4


def test_isotropic_spheres_keep_their_species(tmp_path):
    """A sphere with scalar or equal-component frictions stays on the sphere
    path, and a species that differs only across the director is its own."""
    ureg, eng = _engine(tmp_path)
    _add(ureg, eng, aspect_ratio=1.0, gt=(2.0, 2.0, 2.0), gr=(4.0, 4.0, 4.0))
    assert not eng._has_ellipsoids()
    assert tuple(eng._species_keys[0])[:3] == (1.0, 2.0, 4.0)
    _add(ureg, eng, aspect_ratio=1.0, type_colloid=1, gt=(2.0, 7.0, 2.0), gr=(4.0, 4.0, 4.0))
    assert len(eng._species_keys) == 2 and eng._has_ellipsoids()


def test_mixed_aspect_ratios_raise_at_the_first_integrate(tmp_path):
    ureg, eng = _engine(tmp_path)
    _add(ureg, eng, aspect_ratio=3.0, type_colloid=0)
    _add(ureg, eng, aspect_ratio=2.0, type_colloid=1, x=20.0)
    with pytest.raises(ValueError, match="All particles in the system must have the same aspect"):
        eng.integrate(1)


def test_three_dimensions_and_a_potential_are_not_implemented(tmp_path):
    ureg, eng3 = _engine(tmp_path, n_dims=3)
    with pytest.raises(NotImplementedError):
        _add(ureg, eng3, aspect_ratio=3.0, gt=(2.0, 2.0, 2.0), gr=(4.0, 4.0, 4.0))
    with pytest.raises(NotImplementedError):
        _add(ureg, eng3, aspect_ratio=1.0)
    pot = ureg.Quantity(np.zeros((4, 4, 1)), "sim_energy")
    h = ureg.Quantity(np.array([25.0, 25.0, 100.0]), "micrometer")
    ureg, eng = _engine(tmp_path)
    _add(ureg, eng)
    with pytest.raises(NotImplementedError):
        eng.add_external_potential(pot, h)
    ureg, eng = _engine(tmp_path)
    eng.add_external_potential(ureg.Quantity(np.zeros((4, 4, 1)), "sim_energy"),
                               ureg.Quantity(np.array([25.0, 25.0, 100.0]), "micrometer"))
    with pytest.raises(NotImplementedError):
        _add(ureg, eng)


# ---------------------------------------------------------- friction helpers
def test_friction_helpers_match_the_reference_functions():
    """tests/golden/ellipsoid_friction.npz holds the outputs of the reference's
    calc_ellipsoid_friction_factors_translation / _rotation (swarmrl/utils/
    utils.py:380-457) for eight (axial, equatorial, viscosity) triples, prolate
    and oblate.  The reference's module does not import where the fixture was
    made (it needs jax), so the two functions were run on their own.  The same
    formulas in fp64: only the order of operations may differ."""
    from swarmrl_amd import utils

    gold = np.load(ROOT / "tests" / "golden" / "ellipsoid_friction.npz")
    assert len(gold["triples"]) == 8
    assert (gold["triples"][:, 0] > gold["triples"][:, 1]).sum() == 4  # prolate
    for (ax, eq, eta), tr, ro in zip(gold["triples"], gold["translation"], gold["rotation"]):
        np.testing.assert_allclose(
            utils.calc_ellipsoid_friction_factors_translation(ax, eq, eta), tr, rtol=1e-12)
        np.testing.assert_allclose(
            utils.calc_ellipsoid_friction_factors_rotation(ax, eq, eta), ro, rtol=1e-12)
        assert utils.utils.calc_ellipsoid_friction_factors_rotation is \
            utils.calc_ellipsoid_friction_factors_rotation


def test_friction_helpers_take_quantities():
    from swarmrl_amd import utils
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    eq = ureg.Quantity(1.0, "micrometer") / np.cbrt(3)
    eta = ureg.Quantity(8.9e-4, "pascal * second")
    g_ax, g_eq = utils.calc_ellipsoid_friction_factors_translation(eq * 3, eq, eta)
    want = utils.calc_ellipsoid_friction_factors_translation(3e-6 / np.cbrt(3), 1e-6 / np.cbrt(3),
                                                             8.9e-4)
    np.testing.assert_allclose([g_ax.m_as("newton * second / meter"),
                                g_eq.m_as("newton * second / meter")], want, rtol=1e-12)
    r_ax, r_eq = utils.calc_ellipsoid_friction_factors_rotation(eq * 3, eq, eta)
    assert 0.0 < r_ax.m_as("newton * meter * second") < r_eq.m_as("newton * meter * second")


# ------------------------------------------------------- the pair geometries
def _sample(kappa, lo, hi, n, seed):
    """n pair geometries (r, u_i, u_j: fp32 values held in fp64) inside the
    cutoff with lo < X < hi."""
    rng = np.random.default_rng(seed)
    r_cut = 4.0 * RADIUS * max(kappa, 1.0 / kappa)
    got = [np.zeros((0, 2))] * 3
    while len(got[0]) < n:
        m = 8 * n
        th, d = rng.uniform(0.0, 2.0 * np.pi, m), rng.uniform(0.2, r_cut, m)
        ti, tj = rng.uniform(0.0, 2.0 * np.pi, (2, m))
        new = [np.stack([d * np.cos(th), d * np.sin(th)], -1),
               np.stack([np.cos(ti), np.sin(ti)], -1), np.stack([np.cos(tj), np.sin(tj)], -1)]
        new = [v.astype(np.float32).astype(np.float64) for v in new]
        x = ellipsoid_ref.overlap_x(*new, kappa, SIGMA0)
        dist = np.linalg.norm(new[0], axis=1)
        ok = (x > lo) & (x < hi) & (dist < 0.999 * r_cut)
        got = [np.concatenate([g, v[ok]]) for g, v in zip(got, new)]
    return [g[:n] for g in got] + [r_cut]


def _rot(u, t):
    c, s = np.cos(t), np.sin(t)
    return np.stack([u[:, 0] * c - u[:, 1] * s, u[:, 0] * s + u[:, 1] * c], -1)


@pytest.mark.parametrize("kappa", [3.0, 1.0 / 3.0])
def test_fp64_statement_against_itself(kappa):
    """Central differences of U with h = 1e-5 sigma0 against the analytic
    force and torque, to 1e-6 of |F| and of |T| + |r||F| (truncation h^2 U'''
    / 6 ~ 4e-8 at contact); F_i = -F_j and T_i + T_j + (r x F_j)_z = 0 to
    1e-12.  The sample lies at contact and inside it, 1 <= X < 1.25: a bound
    relative to |F| means nothing around the force's zero at X = 2^(-1/6)."""
    r, ui, uj, r_cut = _sample(kappa, 1.0, 1.25, 4000, 21)
    args = (kappa, SIGMA0, EPS0, r_cut)
    f, t = ellipsoid_ref.force_torque(r, ui, uj, *args)
    fm, dist = np.linalg.norm(f, axis=1), np.linalg.norm(r, axis=1)
    h = 1e-5 * SIGMA0
    fn = np.zeros_like(f)
    for a in range(2):
        e = np.zeros(2)
        e[a] = h
        fn[:, a] = (ellipsoid_ref.energy(r + e, ui, uj, *args)
                    - ellipsoid_ref.energy(r - e, ui, uj, *args)) / (2.0 * h)
    dev_f = np.max(np.linalg.norm(fn - f, axis=1) / fm)
    dth = 1e-5
    tn = -(ellipsoid_ref.energy(r, _rot(ui, dth), uj, *args)
           - ellipsoid_ref.energy(r, _rot(ui, -dth), uj, *args)) / (2.0 * dth)
    dev_t = np.max(np.abs(tn - t) / (np.abs(t) + dist * fm))
    print(f"kappa {kappa:.3f}: central differences force {dev_f:.3g} torque {dev_t:.3g}")
    assert dev_f < 1e-6 and dev_t < 1e-6
    fj, tj = ellipsoid_ref.force_torque(-r, uj, ui, *args)
    assert np.max(np.linalg.norm(f + fj, axis=1) / fm) < 1e-12
    balance = t + tj + (r[:, 0] * fj[:, 1] - r[:, 1] * fj[:, 0])
    assert np.max(np.abs(balance) / (np.abs(t) + np.abs(tj) + dist * fm)) < 1e-12


# measured on this sample: kappa = 3: 2.68e-4 (force), 1.43e-4 (torque);
# kappa = 1/3: 1.58e-5, 4.16e-6.  Four times the worst (1.07e-3), rounded up
# to a power of ten
FP32_TOLERANCE = 1e-2


@pytest.mark.parametrize("kappa", [3.0, 1.0 / 3.0])
def test_fp32_restatement_against_the_fp64_statement(kappa):
    """10^4 pair geometries with 0.8 < X < 1.25 inside the cutoff: the worst
    deviation of the fp32 force from the fp64 one relative to |F| + eps0 /
    sigma0 (the torque: to |T| + |r||F| + eps0).  The worst cases are
    end-to-end pairs (g ~ 0.1 from 1 - 0.9) near the force's zero crossing.
    Above 1e-3 the sequence would be wrong, whatever the tolerance."""
    r, ui, uj, r_cut = _sample(kappa, 0.8, 1.25, 10000, 5)
    f, t = ellipsoid_ref.force_torque(r, ui, uj, kappa, SIGMA0, EPS0, r_cut)
    p = oracle.make_params([100.0] * 3, 0.01, 1.0, EPS0, 1, [(RADIUS, 1.0, 1.0, 1.0, 1.0)])
    ell = ellipsoid_oracle.make_ellipsoids(kappa, [1.0], [2.0])
    got = np.zeros((len(r), 3))
    for k in range(len(r)):
        got[k], in_range, deep = ellipsoid_oracle.pair(p, ell, r[k, 0], r[k, 1], ui[k], uj[k])
        assert in_range and not deep
    fm, dist = np.linalg.norm(f, axis=1), np.linalg.norm(r, axis=1)
    dev_f = np.max(np.linalg.norm(got[:, :2] - f, axis=1) / (fm + EPS0 / SIGMA0))
    dev_t = np.max(np.abs(got[:, 2] - t) / (np.abs(t) + dist * fm + EPS0))
    print(f"kappa {kappa:.3f}: fp32 against fp64 force {dev_f:.3g} torque {dev_t:.3g}")
    assert max(dev_f, dev_t) < 1e-3  # (a wrong sequence)
    assert max(dev_f, dev_t) < FP32_TOLERANCE


def test_deep_overlap_is_finite_and_flagged():
    """X >= 1.25 and |r| - sigma + sigma0 <= 0: the values at X = 1.25, finite."""
    p = oracle.make_params([100.0] * 3, 0.01, 1.0, EPS0, 1, [(RADIUS, 1.0, 1.0, 1.0, 1.0)])
    ell = ellipsoid_oracle.make_ellipsoids(3.0, [1.0], [2.0])
    ux = np.array([1.0, 0.0], np.float32)
    edge, _, deep_e = ellipsoid_oracle.pair(p, ell, 3.0 * SIGMA0 - 0.2 * SIGMA0 + 1e-4, 0.0, ux, ux)
    assert not deep_e
    for d in (4.0, 3.0, 1.0, 1e-3):  # end to end: sigma = 3 sigma0 = 5.35
        out, in_range, deep = ellipsoid_oracle.pair(p, ell, d, 0.0, ux, ux)
        assert in_range and deep and np.all(np.isfinite(out))
        np.testing.assert_allclose(out[0], edge[0], rtol=2e-3)
        assert out[0] < 0.0  # pushed away from j


# ------------------------------------------------ the restatement's own step
@pytest.mark.parametrize("degrees", [0.0, 90.0, 37.0])
def test_anisotropic_step_known_answers(degrees):
    """T = 0, one particle, a constant force (1, 0.5): one sub-step displaces
    it by R diag(dt / g_par, dt / g_perp) R^T f, the last velocities are R
    diag(1 / g_par, 1 / g_perp) R^T f, the torque turns it by t dt / g_r."""
    g_par, g_perp, g_rot, dt, box = 2.0, 5.0, 4.0, 0.01, 100.0
    p = oracle.make_params([box] * 3, dt, 0.0, EPS0, 1, [(RADIUS, g_par, g_rot, 1.0, 1.0)])
    ell = ellipsoid_oracle.make_ellipsoids(3.0, [g_par], [g_perp])
    th = np.deg2rad(degrees)
    u = np.array([np.cos(th), np.sin(th)])
    st0 = oracle.state_from_positions(np.array([[50.0, 50.0, 0.0]]),
                                      np.array([[u[0], u[1], 0.0]]), [box] * 3)
    f = np.array([1.0, 0.5])
    f_ext = np.array([[f[0]], [f[1]], [0.0]], np.float32)
    st, info = ellipsoid_oracle.bd_run(p, ell, st0, [0], [0.0], [0.3], 1, f_ext=f_ext)
    rot = np.array([[u[0], -u[1]], [u[1], u[0]]])
    mob = rot @ np.diag([1.0 / g_par, 1.0 / g_perp]) @ rot.T
    grid = box / TWO32
    dq = (st["q"][:2, 0].astype(np.int64) - st0["q"][:2, 0].astype(np.int64)) * grid
    np.testing.assert_allclose(dq, dt * mob @ f, rtol=1e-6, atol=grid)
    np.testing.assert_allclose(info["vel"][:2, 0], mob @ f, rtol=1e-6)
    assert info["vel"][2, 0] == 0.0
    np.testing.assert_allclose(info["omega"][0], 0.3 / g_rot, rtol=1e-6)
    dang = (int(st["ang"][0]) - int(st0["ang"][0])) * (2.0 * np.pi / TWO32)
    np.testing.assert_allclose(dang, 0.3 * dt / g_rot, rtol=1e-6)
    if degrees == 90.0:  # the reference's case: x across the director, y along it
        np.testing.assert_allclose(info["vel"][:2, 0], [f[0] / g_perp, f[1] / g_par], rtol=1e-6)


def test_swim_force_moves_along_the_director_with_the_parallel_friction():
    g_par, g_perp, dt, box = 2.0, 5.0, 0.01, 100.0
    p = oracle.make_params([box] * 3, dt, 0.0, EPS0, 1, [(RADIUS, g_par, 4.0, 1.0, 1.0)])
    ell = ellipsoid_oracle.make_ellipsoids(1.0, [g_par], [g_perp])  # WCA pairs, new step
    th = np.deg2rad(37.0)
    st0 = oracle.state_from_positions(np.array([[50.0, 50.0, 0.0]]),
                                      np.array([[np.cos(th), np.sin(th), 0.0]]), [box] * 3)
    _, info = ellipsoid_oracle.bd_run(p, ell, st0, [0], [3.0], [0.0], 1)
    np.testing.assert_allclose(info["vel"][:2, 0], 3.0 / g_par * np.array([np.cos(th), np.sin(th)]),
                               rtol=1e-6)
