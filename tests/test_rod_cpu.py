"""
The rod without a GPU: SwarmEngine.add_rod on the host (placement, types,
radius register, refusals), RotateRod on the list path against the
reference's known answers (CI/unit_tests/tasks/test_rod_rotation.py), and
known answers of the CPU restatement of the rod sub-step
(tests/csrc/rod_oracle.c) that the GPU tests compare the kernels with.
"""

import logging

import numpy as np
import pytest

import rod_oracle
from oracle import oracle


# ------------------------------------------------------------ add_rod (host)
def _md_params(ureg, **kw):
    from swarmrl_amd.engine import MDParams

    args = dict(
        ureg=ureg,
        fluid_dyn_viscosity=ureg.Quantity(8.9e-4, "pascal * second"),
        WCA_epsilon=0.1 * ureg.Quantity(300, "kelvin") * ureg.boltzmann_constant,
        temperature=ureg.Quantity(300, "kelvin"),
        box_length=ureg.Quantity(3 * [50], "micrometer"),
        time_step=ureg.Quantity(0.0001, "second"),
        time_slice=ureg.Quantity(0.1, "second"),
        write_interval=ureg.Quantity(0.1, "second"),
    )
    args.update(kw)
    return MDParams(**args)


def _runner(tmp_path, n_dims=2, n_colloids=50, **kw):
    from swarmrl_amd.engine import SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    runner = SwarmEngine(_md_params(ureg, **kw), n_dims=n_dims, out_folder=tmp_path,
                         write_chunk_size=1)
    if n_colloids:
        runner.add_colloids(n_colloids, ureg.Quantity(1.0, "micrometer"),
                            ureg.Quantity(np.array([25, 25, 0]), "micrometer"),
                            ureg.Quantity(25, "micrometer"), type_colloid=0)
    return ureg, runner


def _rod_args(ureg, **kw):
    """The rod of the reference's test_rod.py."""
    args = dict(
        rod_center=ureg.Quantity(np.array([25, 25, 0]), "micrometer"),
        rod_length=ureg.Quantity(40, "micrometer"),
        rod_thickness=ureg.Quantity(3, "micrometer"),
        rod_start_angle=np.pi / 2.0,
        n_particles=31,
        friction_trans=ureg.Quantity(10, "newton/ (meter / second)"),
        friction_rot=ureg.Quantity(1e-17, "newton * meter * second"),
        rod_particle_type=2,
        fixed=True,
    )
    args.update(kw)
    return args


def test_add_rod_places_centre_and_beads(tmp_path):
    ureg, runner = _runner(tmp_path)
    centre = runner.add_rod(**_rod_args(ureg))
    assert len(runner.colloids) == 81
    assert centre.id == 50 and centre is runner.colloids[50]
    delta = (40.0 - 3.0) / 30
    u = np.array([np.cos(np.pi / 2), np.sin(np.pi / 2), 0.0])
    np.testing.assert_allclose(centre.pos, [25.0, 25.0, 0.0])
    for k in range(30):
        expect = np.array([25.0, 25.0, 0.0]) + (-1) ** k * (k // 2 + 1) * delta * u
        np.testing.assert_allclose(runner.colloids[51 + k].pos, expect, atol=1e-12)
        np.testing.assert_allclose(runner.colloids[51 + k].director, u, atol=1e-12)
    assert [c.type for c in runner.colloids] == 50 * [0] + 31 * [2]
    assert runner.colloid_radius_register[2] == {"radius": 1.5, "aspect_ratio": 1.0}
    assert runner._rod == {"first": 50, "n": 31, "delta": pytest.approx(delta), "fixed": True,
                           "type": 2}
    # a species of its own: the frictions given, no mass or rotational inertia
    key = runner._species_keys[runner._species_of[50]]
    assert key[0] == 1.5 and key[3] == 0.0 and key[4] == 0.0
    assert len(set(runner._species_of[50:])) == 1
    assert runner._species_of[50] != runner._species_of[0]


def test_add_rod_warns_about_holes(tmp_path, caplog):
    ureg, runner = _runner(tmp_path, n_colloids=0)
    with caplog.at_level(logging.WARNING):
        runner.add_rod(**_rod_args(ureg, n_particles=5))  # spacing 9.25 > thickness 3
    assert "your rod has holes" in caplog.text


def test_add_rod_refusals_as_the_reference(tmp_path):
    ureg, runner = _runner(tmp_path / "a", n_dims=3, n_colloids=0)
    with pytest.raises(ValueError, match="2d"):
        runner.add_rod(**_rod_args(ureg))
    ureg, runner = _runner(tmp_path / "b", n_colloids=0)
    with pytest.raises(ValueError, match="uneven"):
        runner.add_rod(**_rod_args(ureg, n_particles=30))
    with pytest.raises(ValueError, match="rotational friction"):
        runner.add_rod(**_rod_args(ureg, friction_rot=None))
    with pytest.raises(ValueError, match="friction coefficient"):
        runner.add_rod(**_rod_args(ureg, friction_trans=None, fixed=False))
    with pytest.raises(ValueError, match="particle type"):
        runner.add_rod(**_rod_args(ureg, rod_particle_type=None))
    # none of the refused calls left anything behind
    assert runner.colloids == [] and runner._rod is None
    runner.add_rod(**_rod_args(ureg))
    assert len(runner.colloids) == 31


def test_add_rod_refuses_a_second_rod(tmp_path):
    ureg, runner = _runner(tmp_path, n_colloids=0)
    runner.add_rod(**_rod_args(ureg))
    with pytest.raises(ValueError, match="already has a rod"):
        runner.add_rod(**_rod_args(ureg, rod_particle_type=3))


def test_add_rod_refuses_walls(tmp_path):
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction

    ureg, runner = _runner(tmp_path / "a")
    runner.add_confining_walls(5)
    with pytest.raises(NotImplementedError, match="walls"):
        runner.add_rod(**_rod_args(ureg))
    # walls added after the rod: refused at the first integrate, before any device work
    ureg, runner = _runner(tmp_path / "b")
    runner.add_rod(**_rod_args(ureg))
    runner.add_confining_walls(5)
    with pytest.raises(NotImplementedError, match="walls"):
        runner.integrate(1, ForceFunction({"0": dummy_models.ConstForce(0)}))


def test_rod_refuses_a_constant_force_on_its_type(tmp_path):
    """k_rod_run applies f_ext to the free colloids only, so a force on the
    rod's type would be dropped without a word: the host refuses it, whether
    the rod or the colloids' force came first.  A force on the colloids' type
    is fine, and its rows for the rod's particles are zero."""
    ureg, runner = _runner(tmp_path / "a")
    force = ureg.Quantity(np.array([1.0, 2.0, 0.0]), "sim_force")
    runner.add_rod(**_rod_args(ureg))
    with pytest.raises(NotImplementedError, match="rod's type"):
        runner.add_const_force_to_colloids(force, 2)
    assert runner._ext_force == {}
    runner.add_const_force_to_colloids(force, 0)

    ureg, runner = _runner(tmp_path / "b")
    force = ureg.Quantity(np.array([1.0, 2.0, 0.0]), "sim_force")
    runner.add_const_force_to_colloids(force, 0)
    with pytest.raises(ValueError, match="Particles of type 2 not added"):
        runner.add_const_force_to_colloids(force, 2)  # (no rod yet: the reference's error)
    runner.add_rod(**_rod_args(ureg))
    with pytest.raises(NotImplementedError, match="rod's type"):
        runner.add_const_force_to_colloids(force, 2)
    ext = runner._compose_ext_force()
    assert ext.shape == (1, 81, 3)
    assert np.all(ext[0, :50] == [1.0, 2.0, 0.0]) and np.all(ext[0, 50:] == 0.0)
    # the check of the first integrate: a force that got onto the rod's type some other way
    runner._ext_force[2] = np.zeros(3)
    with pytest.raises(NotImplementedError, match="rod's type"):
        runner._validate_rod()


def test_add_rod_refuses_a_non_periodic_box(tmp_path):
    ureg, runner = _runner(tmp_path, periodic=False)
    with pytest.raises(NotImplementedError, match="non-periodic"):
        runner.add_rod(**_rod_args(ureg))


def test_add_rod_refuses_more_than_255_rod_particles(tmp_path):
    ureg, runner = _runner(tmp_path, n_colloids=0)
    with pytest.raises(ValueError, match="255"):
        runner.add_rod(**_rod_args(ureg, n_particles=257))
    runner.add_rod(**_rod_args(ureg, n_particles=255))


def test_add_rod_refuses_more_than_4096_particles_per_env(tmp_path):
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction

    ureg, runner = _runner(tmp_path / "a", n_colloids=4066)
    with pytest.raises(ValueError, match="4096"):
        runner.add_rod(**_rod_args(ureg))  # 4066 + 31 = 4097
    ureg, runner = _runner(tmp_path / "b", n_colloids=4065)
    runner.add_rod(**_rod_args(ureg))  # 4096: allowed
    runner.add_colloids(1, ureg.Quantity(1.0, "micrometer"),
                        ureg.Quantity(np.array([25, 25, 0]), "micrometer"),
                        ureg.Quantity(25, "micrometer"), type_colloid=0)
    with pytest.raises(ValueError, match="4096"):
        runner.integrate(1, ForceFunction({"0": dummy_models.ConstForce(0)}))


# -------------------------------------------------- RotateRod on the list path
def _trajectory(direction_scale=1):
    from swarmrl_amd.components import Colloid

    colloids, angle = [], 0.0
    for _ in range(100):
        angle += np.deg2rad(direction_scale * 45)
        director = np.array([np.cos(angle), np.sin(angle), 0])
        colloids.append(Colloid(pos=np.array([0, 0, 0]), id=0, director=director, type=1))
    return np.array([1, 0, 0]), colloids


@pytest.mark.parametrize("direction,sign", [("CCW", 1.0), ("CW", -1.0)])
def test_rotate_rod_angular_velocity_kat(direction, sign):
    """test_rod_rotation.py:42-94: steps of +-45 degrees give +-45.0 for CCW
    and the negated values for CW, at every length of the history."""
    from swarmrl_amd.tasks import RotateRod

    for scale in (1, -1):
        task = RotateRod(direction=direction, angular_velocity_scale=1.0)
        start, colloids = _trajectory(direction_scale=scale)
        task._historic_rod_director = start
        for colloid in colloids:
            velocity = task._compute_angular_velocity(colloid.director)
            assert velocity == pytest.approx(sign * scale * 45.0)


def _rod_colloids(angle=0.0, n=5, delta=1.0, rod_type=1):
    from swarmrl_amd.components import Colloid

    u = np.array([np.cos(angle), np.sin(angle), 0.0])
    return [Colloid(pos=rod_oracle.slot(b) * delta * u, director=u, id=100 + b, type=rod_type)
            for b in range(n)]


def test_rotate_rod_partition_kat():
    """One colloid takes the whole reward, two mirror-image colloids half
    each, partition=False shares it uniformly; initialize takes the rod's
    director as the historic one."""
    from swarmrl_amd.components import Colloid
    from swarmrl_amd.tasks.object_movement import RotateRod
    from swarmrl_amd.utils.colloid_utils import compute_torque_partition_on_rod

    x = np.array([1.0, 0.0, 0.0])

    def swimmer(pos, i):
        return Colloid(pos=np.array(pos, dtype=float), director=x, id=i, type=0)

    rod0, rod1 = _rod_colloids(0.0), _rod_colloids(np.deg2rad(30.0))
    one = [swimmer([1.3, 2.0, 0.0], 0)]
    task = RotateRod(velocity_history=4)
    task.initialize(one + rod0)
    np.testing.assert_array_equal(task._historic_rod_director, rod0[0].director)
    r = task(one + rod1)
    assert r.shape == (1,) and r.dtype == np.float32
    assert r[0] == pytest.approx(30.0, rel=1e-6)  # partition 1, mean over one entry

    two = [swimmer([1.3, 2.0, 0.0], 0), swimmer([-1.3, -2.0, 0.0], 1)]
    rp = np.array([c.pos for c in rod0])
    rd = np.array([c.director for c in rod0])
    part = compute_torque_partition_on_rod(np.array([c.pos for c in two]), rp, rd)
    np.testing.assert_allclose(part, [0.5, 0.5], rtol=1e-12)
    task = RotateRod(velocity_history=4, direction="CW")
    task.initialize(two + rod0)
    np.testing.assert_allclose(task(two + rod1), [-15.0, -15.0], rtol=1e-6)
    # second call: the mean of (30, 0)
    np.testing.assert_allclose(task(two + rod1), [-7.5, -7.5], rtol=1e-6)

    three = two + [swimmer([7.0, 9.0, 0.0], 2)]
    part = compute_torque_partition_on_rod(np.array([c.pos for c in three]), rp, rd)
    assert part[2] < 1e-3 * part[0] and part.sum() == pytest.approx(1.0)
    task = RotateRod(partition=False, angular_velocity_scale=2)
    task.initialize(three + rod0)
    np.testing.assert_allclose(task(three + rod1), 3 * [2 * 30.0 / 3], rtol=1e-6)


def test_torque_partition_is_the_references_formula():
    """w_i = |sum_b cross(u_b, grad(1 / |r_b - r_i|^12))| + 1e-8, written out
    per pair (colloid_utils.py:29-117)."""
    from swarmrl_amd.utils.colloid_utils import compute_torque_partition_on_rod

    rng = np.random.default_rng(3)
    cp = np.concatenate([rng.uniform(-6, 6, (7, 2)), np.zeros((7, 1))], axis=1)
    cp[:, 1] += 3.0
    th = 0.4
    u = np.array([np.cos(th), np.sin(th), 0.0])
    rp = np.array([rod_oracle.slot(b) * 0.9 * u for b in range(9)])
    w = np.zeros(7)
    for i in range(7):
        tq = np.zeros(3)
        for b in range(9):
            r = (rp[b] - cp[i])[:2]
            f = -12.0 * r / np.linalg.norm(r) ** 14
            tq += np.cross(u, np.array([f[0], f[1], 0.0]))
        w[i] = np.linalg.norm(tq) + 1e-8
    got = compute_torque_partition_on_rod(cp, rp, np.tile(u, (9, 1)))
    np.testing.assert_allclose(got, w / w.sum(), rtol=1e-12)


# --------------------------------------------------- the restatement's KATs
BOX = np.array([50.0, 50.0, 50.0])
DT = 0.005
COLLOID = (1.0, 4.0, 3.0, 1.0, 0.4)  # radius, gamma_t, gamma_r, mass, rinertia
ROD = (1.5, 20.0, 200.0, 0.0, 0.0)


def _system(colloid_pos, colloid_dir, centre=(25.0, 25.0), angle=0.0, n_rod=11, length=20.0,
            kT=0.0, fixed=True, seed=5):
    """colloids first, then the rod (centre, beads) snapped onto its line"""
    nc = len(colloid_pos)
    delta = (length - 2 * ROD[0]) / (n_rod - 1)
    pos = np.zeros((nc + n_rod, 3))
    dirs = np.zeros((nc + n_rod, 3))
    pos[:nc, :2] = colloid_pos
    dirs[:nc, :2] = colloid_dir
    u = np.array([np.cos(angle), np.sin(angle)])
    for b in range(n_rod):
        pos[nc + b, :2] = np.asarray(centre) + rod_oracle.slot(b) * delta * u
        dirs[nc + b, :2] = u
    params = oracle.make_params(BOX, DT, kT, 1.0, seed, [COLLOID, ROD])
    rod = rod_oracle.make_rod(nc, n_rod, delta, fixed)
    species = np.array(nc * [0] + n_rod * [1], np.uint8)
    state = rod_oracle.snap(params, oracle.state_from_positions(pos, dirs, BOX), rod)
    return params, state, species, rod


def _placed(params, state, rod, b):
    """The placement rule applied to the centre of `state`, for bead b."""
    c = rod.first
    sn, cs = oracle.sincos_turn(int(state["ang"][c]))
    lever = np.float32(rod_oracle.slot(b)) * np.float32(rod.delta)
    out = []
    for a, t in ((0, cs), (1, sn)):
        inv_sx = np.float32(oracle.TWO32 / params.box[a])
        dq = int(np.rint(np.float32(np.float32(lever * np.float32(t)) * inv_sx)))
        total = int(state["img"][a, c]) * 2**32 + int(state["q"][a, c]) + dq
        out.append((total % 2**32, total // 2**32))
    return out


def test_restatement_fixed_rod_only_turns():
    """No colloids, kT > 0, fixed rod: the centre's q/img keep their bits,
    its angle changes, and every bead is the placement rule applied to the
    centre."""
    params, st0, species, rod = _system(np.zeros((0, 2)), np.zeros((0, 2)), angle=0.3, kT=1.0)
    n = len(species)
    st, info = rod_oracle.bd_run(params, st0, species, np.zeros(n), np.zeros(n), 25, rod)
    c = rod.first
    assert np.array_equal(st["q"][:, c], st0["q"][:, c])
    assert np.array_equal(st["img"][:, c], st0["img"][:, c])
    assert st["ang"][c] != st0["ang"][c]
    assert info["contacts"] == 0 and not info["F"].any() and not info["S"].any()
    for b in range(1, rod.n):
        (qx, ix), (qy, iy) = _placed(params, st, rod, b)
        assert (st["q"][0, c + b], st["img"][0, c + b]) == (qx, ix)
        assert (st["q"][1, c + b], st["img"][1, c + b]) == (qy, iy)
        assert st["ang"][c + b] == st["ang"][c]
    np.testing.assert_array_equal(info["vel"][:, c], 0.0)


def _push(side):
    """kT = 0: one colloid swimming perpendicularly (+y) into a fixed rod
    along x, at lever side * 3.4 (bead slot 2 * side), starting just outside
    the cutoff."""
    gap = COLLOID[0] + ROD[0] + 0.004
    return _system(np.array([[25.0 + side * 3.4, 25.0 - gap]]), np.array([[0.0, 1.0]]))


def _first_contact(side):
    params, st, species, rod = _push(side)
    n = len(species)
    f_swim = np.array([8.0] + (n - 1) * [0.0], np.float32)
    for step in range(40):
        new, info = rod_oracle.bd_run(params, st, species, f_swim, np.zeros(n), 1, rod,
                                      step0=step)
        if info["contacts"]:
            d = (int(new["ang"][rod.first]) - int(st["ang"][rod.first])) % 2**32
            return (d - 2**32 if d >= 2**31 else d), info
        st = new
    raise AssertionError("the colloid never reached the rod")


def test_restatement_torque_sign_and_mirror():
    """The angle increment of the first contact sub-step has the sign of
    s x F (lever +s along x, force along +y: counter-clockwise), and the
    mirrored set-up gives exactly the negated increment."""
    d_plus, info = _first_contact(+1)
    assert info["F"][1] > 0 and info["S"][1] > 0 and info["tau"] > 0
    assert d_plus > 0
    d_minus, info = _first_contact(-1)
    assert info["F"][1] > 0 and info["S"][1] < 0 and info["tau"] < 0
    assert d_minus == -d_plus


def test_restatement_rod_force_is_minus_the_colloids():
    """Every sub-step of a contact run: F = -Sigma, Sigma the sum of the
    bead-contact forces on the colloids -- exact in fixed point."""
    rng = np.random.default_rng(1)
    th = np.linspace(0.0, 2 * np.pi, 12, endpoint=False)
    ring = 25.0 + np.stack([9.0 * np.cos(th), 2.6 * np.sin(th)], axis=1)
    facing = np.stack([-np.cos(th), -np.sin(th)], axis=1)
    params, st, species, rod = _system(ring + rng.uniform(-0.05, 0.05, ring.shape), facing,
                                       angle=0.1, kT=1.0, fixed=False)
    n = len(species)
    f_swim = np.array(12 * [6.0] + rod.n * [0.0], np.float32)
    seen = 0
    for step in range(30):
        st, info = rod_oracle.bd_run(params, st, species, f_swim, np.zeros(n), 1, rod,
                                     step0=step)
        assert np.array_equal(info["F"], -info["sigma"])
        seen += info["contacts"]
    assert seen >= 10


def test_restatement_central_push_translates_without_turning():
    """A free rod pushed at its centre along its normal translates and turns
    by exactly 0 (kT = 0: S_y = 0 and u_y = 0)."""
    gap = COLLOID[0] + ROD[0] + 0.004
    params, st0, species, rod = _system(np.array([[25.0, 25.0 - gap]]), np.array([[0.0, 1.0]]),
                                        fixed=False)
    n = len(species)
    f_swim = np.array([8.0] + (n - 1) * [0.0], np.float32)
    st, info = rod_oracle.bd_run(params, st0, species, f_swim, np.zeros(n), 60, rod)
    c = rod.first
    assert info["contacts"] > 0
    assert st["ang"][c] == st0["ang"][c]
    assert np.array_equal(st["ang"][c:], st0["ang"][c:])
    dy = int(st["q"][1, c]) - int(st0["q"][1, c])
    assert dy > 0 and st["q"][0, c] == st0["q"][0, c]
    # every bead moved with the centre
    assert np.array_equal(st["q"][1, c:].astype(np.int64) - st0["q"][1, c:], np.full(rod.n, dy))


def test_restatement_external_force_moves_the_colloids_only():
    """f_ext in the rod restatement.  Free colloids far from the rod at kT = 0
    drift by n dt (f_ext + f_swim d) / gamma_t (the bound of
    test_oracle_kat.py's drift case: n sx / 2 + 4 2^-24 |expected|), the z
    component moves nothing, and the rod keeps its bits.  In a contact run
    at kT > 0 a force on the rod's own particles has no effect: the same bits
    as zeros there -- what k_rod_run does, which skips f_ext for the rod."""
    rng = np.random.default_rng(8)
    cpos = np.array([[8.0, 9.0], [41.0, 10.0], [9.0, 40.0], [42.0, 41.0]])
    ang = np.array([0.4, 2.0, 3.7, 5.5])
    params, st0, species, rod = _system(cpos, np.stack([np.cos(ang), np.sin(ang)], 1), angle=0.3)
    n, nc, n_steps = len(species), len(cpos), 100
    f_swim = np.array([2.0, 3.0, 1.5, 4.0] + rod.n * [0.0], np.float32)
    f_ext = (rng.uniform(1.0, 6.0, (3, n)) * rng.choice([-1.0, 1.0], (3, n))).astype(np.float32)
    st, info = rod_oracle.bd_run(params, st0, species, f_swim, np.zeros(n), n_steps, rod,
                                 f_ext=f_ext)
    assert info["contacts"] == 0
    th = st0["ang"][:nc].astype(np.float64) * (2 * np.pi / 2.0**32)
    force = f_ext[:2, :nc].astype(np.float64) + f_swim[:nc] * np.stack([np.cos(th), np.sin(th)])
    expect = (n_steps * DT * force / COLLOID[1]).T
    dx = (oracle.unwrapped(st, BOX) - oracle.unwrapped(st0, BOX))[:nc]
    bound = n_steps * (BOX[0] / 2.0**32) / 2 + 4 * 2.0**-24 * np.abs(expect)
    assert np.all(np.abs(dx[:, :2] - expect) <= bound), np.max(np.abs(dx[:, :2] - expect) / bound)
    assert np.all(dx[:, 2] == 0.0) and np.all(info["vel"][2] == 0.0)
    v_bound = (4 * 2.0**-24 * (np.abs(f_ext[:2, :nc]) + f_swim[:nc]) + 2e-7 * f_swim[:nc])
    assert np.all(np.abs(info["vel"][:2, :nc] - force / COLLOID[1]) <= v_bound / COLLOID[1])
    c = rod.first
    for k in ("q", "img", "ang"):  # kT = 0, no contact: the forced rod does not move
        assert np.array_equal(st[k][..., c:], st0[k][..., c:])

    # contacts, noise, a free rod: the rod's rows of f_ext are never read
    th = np.linspace(0.0, 2 * np.pi, 12, endpoint=False)
    ring = 25.0 + np.stack([9.0 * np.cos(th), 2.6 * np.sin(th)], axis=1)
    facing = np.stack([-np.cos(th), -np.sin(th)], axis=1)
    params, st0, species, rod = _system(ring + rng.uniform(-0.05, 0.05, ring.shape), facing,
                                        angle=0.1, kT=1.0, fixed=False)
    n = len(species)
    f_swim = np.array(12 * [6.0] + rod.n * [0.0], np.float32)
    f_ext = (rng.normal(size=(3, n)) * 3).astype(np.float32)
    zeroed = f_ext.copy()
    zeroed[:, rod.first:] = 0.0
    a, ia = rod_oracle.bd_run(params, st0, species, f_swim, np.zeros(n), 30, rod, f_ext=f_ext)
    b, ib = rod_oracle.bd_run(params, st0, species, f_swim, np.zeros(n), 30, rod, f_ext=zeroed)
    none, _ = rod_oracle.bd_run(params, st0, species, f_swim, np.zeros(n), 30, rod)
    assert ia["contacts"] >= 10
    for k in ("q", "img", "ang"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(ia["vel"], ib["vel"]) and np.array_equal(ia["omega"], ib["omega"])
    assert np.array_equal(ia["F"], ib["F"]) and ia["tau"] == ib["tau"]
    assert not np.array_equal(a["q"], none["q"])
    # the overlap removal: the same holds
    sa, _ = rod_oracle.sd_run(params, st0, species, 50, rod, f_ext=f_ext)
    sb, _ = rod_oracle.sd_run(params, st0, species, 50, rod, f_ext=zeroed)
    s0, _ = rod_oracle.sd_run(params, st0, species, 50, rod)
    for k in ("q", "img", "ang"):
        assert np.array_equal(sa[k], sb[k]), k
        assert np.array_equal(sa[k][..., rod.first:], st0[k][..., rod.first:])
    assert not np.array_equal(sa["q"], s0["q"])


def test_restatement_overlap_removal_keeps_the_rod():
    params, st0, species, rod = _system(np.array([[24.0, 26.0], [30.0, 24.2]]),
                                        np.array([[1.0, 0.0], [1.0, 0.0]]), angle=0.2)
    st, steps = rod_oracle.sd_run(params, st0, species, 1000, rod)
    c = rod.first
    for k in ("q", "img", "ang"):
        assert np.array_equal(st[k][..., c:], st0[k][..., c:])
    assert not np.array_equal(st["q"][:, :c], st0["q"][:, :c])
    assert 0 < steps < 1000
    # nothing overlaps any more: one more step moves nothing
    again, more = rod_oracle.sd_run(params, st, species, 5, rod)
    assert more == 0 and np.array_equal(again["q"], st["q"])
