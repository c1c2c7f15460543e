"""
The rod on the GPU: k_rod_run (BD sub-steps and the overlap removal) bit for
bit against the CPU restatement tests/csrc/rod_oracle.c, the reference's
test_rod.py through the product API, RotateRod's device reward against its
list path, the vision cone on a rod engine and a short training run.
"""

import numpy as np
import pytest
import torch

import rod_oracle
from oracle import oracle

pytestmark = pytest.mark.gpu

TWO32 = 4294967296.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _engine(tmp_path, box=50.0, n_envs=1, seed=11, reuse_forces=True, steps_per_slice=20,
            time_step=0.005, temperature=300.0):
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    params = MDParams(
        ureg=ureg,
        box_length=ureg.Quantity(list(box) if np.ndim(box) else 3 * [box], "micrometer"),
        temperature=ureg.Quantity(temperature, "kelvin"),
        time_step=ureg.Quantity(time_step, "second"),
        time_slice=ureg.Quantity(time_step * steps_per_slice, "second"),
        write_interval=ureg.Quantity(time_step * steps_per_slice, "second"),
    )
    eng = SwarmEngine(params, n_dims=2, seed=seed, out_folder=tmp_path, write_chunk_size=1,
                      n_envs=n_envs, reuse_forces=reuse_forces)
    return ureg, eng


def _add_points(ureg, eng, pos, dirs, radius):
    for p, d in zip(pos, dirs):
        eng.add_colloid_on_point(ureg.Quantity(radius, "micrometer"),
                                 ureg.Quantity(np.array([p[0], p[1], 0.0]), "micrometer"),
                                 np.array([d[0], d[1], 0.0]), type_colloid=0)


def _add_rod(ureg, eng, centre, length, thickness, angle, n, fixed, rod_type=2):
    return eng.add_rod(ureg.Quantity(np.array([centre[0], centre[1], 0.0]), "micrometer"),
                       ureg.Quantity(length, "micrometer"),
                       ureg.Quantity(thickness, "micrometer"), angle, n,
                       ureg.Quantity(20.0, "sim_force / sim_velocity"),
                       ureg.Quantity(200.0, "sim_force * sim_length * sim_time"),
                       rod_type, fixed=fixed)


def _ring(centre, radius, n):
    """n swimmers on a ring around the rod's centre, facing it."""
    th = np.linspace(0.0, 2 * np.pi, n, endpoint=False) + 0.05
    unit = np.stack([np.cos(th), np.sin(th)], axis=1)
    return np.asarray(centre) + radius * unit, -unit


def _restatement(eng):
    """The CPU side of an engine that has not integrated yet: parameters,
    species, rod and per env the uploaded state with the beads snapped."""
    p = oracle.make_params(eng._box, eng._time_step, eng._kT(),
                           eng.params.WCA_epsilon.m_as("sim_energy"), eng.seed,
                           eng._species_keys)
    rod = rod_oracle.make_rod(eng._rod["first"], eng._rod["n"], eng._rod["delta"],
                              eng._rod["fixed"])
    sp = np.asarray(eng._species_of, np.uint8)
    states = [rod_oracle.snap(p, oracle.state_from_positions(np.stack(eng._pos[e]),
                                                             np.stack(eng._dir[e]), eng._box), rod)
              for e in range(eng.n_envs)]
    return p, sp, rod, states


def _assert_state(eng, states):
    got = eng.get_raw_state()
    n = eng.n_particles
    for e, st in enumerate(states):
        for k in ("q", "img", "ang"):
            assert np.array_equal(got[k][..., e * n:(e + 1) * n], st[k]), (k, e)


def _run_against_restatement(eng, force, n_slices, min_contacts):
    """integrate(1) n_slices times with a ConstForce on type 0, after every
    slice equal to the restatement (overlap removal, then BD with
    reuse_forces as the engine has it); returns the contacts seen per env."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction

    p, sp, rod, states = _restatement(eng)
    n = eng.n_particles
    f_swim = np.where(np.asarray(eng._types_list) == 0, force, 0.0).astype(np.float32)
    steps = eng.params.steps_per_slice
    states = [rod_oracle.sd_run(p, st, sp, 1000, rod)[0] for st in states]
    reuse = [rod_oracle.ReuseForces(st) for st in states]
    contacts = np.zeros(eng.n_envs, np.int64)
    ff = ForceFunction({"0": dummy_models.ConstForce(force)})
    for k in range(n_slices):
        eng.integrate(1, ff)
        for e in range(eng.n_envs):
            if eng.reuse_forces:
                states[e], info = reuse[e].run(p, states[e], sp, f_swim, np.zeros(n), steps, rod,
                                               step0=k * steps, env=e)
            else:
                states[e], info = rod_oracle.bd_run(p, states[e], sp, f_swim, np.zeros(n), steps,
                                                    rod, step0=k * steps, env=e)
            contacts[e] += info["contacts"]
        _assert_state(eng, states)
    # the condition of the case: the rod is pushed in every env
    assert np.all(contacts >= min_contacts), contacts
    return contacts


@pytest.mark.parametrize("reuse_forces", [True, False])
@pytest.mark.parametrize("fixed", [True, False])
def test_rod_run_bit_exact(tmp_path, fixed, reuse_forces):
    """E = 2, 24 swimmers of radius 1 in a ring around an 11-particle rod
    (length 20, thickness 3), kT > 0, 3 slices of 20 sub-steps: q, img and ang
    of every particle equal the restatement after every slice.  The swimmers
    on the rod's axis start inside its ends (the overlap removal pushes them
    to the cutoff), so they press on it from the first sub-steps."""
    ureg, eng = _engine(tmp_path, n_envs=2, reuse_forces=reuse_forces)
    pos, dirs = _ring((25.0, 25.0), 8.0, 24)
    _add_points(ureg, eng, pos, dirs, 1.0)
    _add_rod(ureg, eng, (25.0, 25.0), 20.0, 3.0, 0.3, 11, fixed)
    _run_against_restatement(eng, 5.0, 3, min_contacts=1)
    assert eng.step_count() == 60


def test_rod_run_wraps_the_periodic_boundary(tmp_path):
    """The same system with the rod's centre at (48, 25) and angle 0: beads
    and swimmers lie on both sides of the periodic boundary."""
    ureg, eng = _engine(tmp_path, n_envs=2)
    pos, dirs = _ring((48.0, 25.0), 8.0, 24)
    _add_points(ureg, eng, pos, dirs, 1.0)
    _add_rod(ureg, eng, (48.0, 25.0), 20.0, 3.0, 0.0, 11, False)
    _run_against_restatement(eng, 5.0, 3, min_contacts=1)
    img = eng.get_raw_state()["img"][0, :eng.n_particles]
    assert img.min() == 0 and img.max() == 1  # (particles on both sides)


def test_rod_run_on_a_grid_of_two_cells(tmp_path):
    """A 7 x 60 um box: 2 cells across, where both cells of a stencil row are
    one range and there is no wrap range.  A 7-particle rod of spacing 1
    (length 7, thickness 1) along y in the middle, 4 swimmers of radius 1 on
    either side facing it, 0.1 um inside the cutoff (the overlap removal
    pushes them out, then they press on the rod), E = 2, 3 slices of 20
    sub-steps."""
    ureg, eng = _engine(tmp_path, box=[7.0, 60.0, 60.0], n_envs=2)
    ys = 30.0 + 2.2 * (np.arange(4) - 1.5)
    pos = [(3.5 - side * 1.4, y) for side in (1.0, -1.0) for y in ys]
    dirs = [(side, 0.0) for side in (1.0, -1.0) for _ in ys]
    _add_points(ureg, eng, pos, dirs, 1.0)
    _add_rod(ureg, eng, (3.5, 30.0), 7.0, 1.0, np.pi / 2, 7, False)
    assert eng._rod["delta"] == 1.0
    assert oracle.cell_grid(_restatement(eng)[0], eng.n_particles, 2.0) == (1, 4)
    _run_against_restatement(eng, 5.0, 3, min_contacts=1)


def _large_system():
    """1100 swimmers of radius 0.5 around a 31-particle rod (length 40,
    thickness 2) in a 100 um box, nothing overlapping: two rows of 36 just
    outside the cutoff on either side of the rod, facing it, the rest on a
    grid away from it."""
    centre, angle = np.array([50.0, 50.0]), 0.4
    u = np.array([np.cos(angle), np.sin(angle)])
    v = np.array([-u[1], u[0]])
    pos, dirs = [], []
    for side in (1.0, -1.0):
        for k in range(36):
            pos.append(centre + (k - 17.5) * 1.1 * u + side * 1.52 * v)
            dirs.append(-side * v)
    for gx in np.arange(2.0, 99.0, 2.5):
        for gy in np.arange(2.0, 99.0, 2.5):
            if len(pos) == 1100:
                break
            r = np.array([gx, gy]) - centre
            if abs(r @ u) < 24.0 and abs(r @ v) < 4.0:
                continue
            pos.append(np.array([gx, gy]))
            dirs.append(u)
    assert len(pos) == 1100
    return np.array(pos), np.array(dirs), centre, angle


def test_rod_run_more_than_one_particle_per_thread(tmp_path):
    """1131 particles in one env (more than the workgroup's 1024 threads),
    72 swimmers pressing on the rod from both sides: contacts from several
    waves land in the rod's sums in the same sub-step."""
    ureg, eng = _engine(tmp_path, box=100.0, steps_per_slice=10)
    pos, dirs, centre, angle = _large_system()
    _add_points(ureg, eng, pos, dirs, 0.5)
    _add_rod(ureg, eng, centre, 40.0, 2.0, angle, 31, False)
    assert eng.n_particles == 1131
    _run_against_restatement(eng, 30.0, 1, min_contacts=8)


def test_overlap_removal_keeps_the_rod(tmp_path):
    """Swimmers placed on top of the rod: the overlap removal moves them
    exactly as or_rod_sd_run does and leaves the rod's bits alone."""
    ureg, eng = _engine(tmp_path, n_envs=2)
    pos, dirs = _ring((25.0, 25.0), 3.0, 8)
    _add_points(ureg, eng, pos, dirs, 1.0)
    _add_rod(ureg, eng, (25.0, 25.0), 20.0, 3.0, 0.3, 11, True)
    p, sp, rod, states = _restatement(eng)
    eng._setup_interactions()
    _assert_state(eng, states)  # the upload snapped the beads as the restatement does
    eng._remove_overlap()
    after = [rod_oracle.sd_run(p, st, sp, 1000, rod) for st in states]
    assert all(0 < steps < 1000 for _, steps in after)
    _assert_state(eng, [st for st, _ in after])
    c = rod.first
    for (st, _), st0 in zip(after, states):
        for k in ("q", "img", "ang"):
            assert np.array_equal(st[k][..., c:c + rod.n], st0[k][..., c:c + rod.n])
        assert not np.array_equal(st["q"][:, :c], st0["q"][:, :c])


def test_reference_rod_test_through_the_product_api(tmp_path):
    """CI/espresso_tests/unit_tests/test_rod.py: 50 colloids and a fixed
    31-particle rod; over 100 slices of 1000 sub-steps the centre stays where
    it is and the director turns; the colloid-rod WCA cutoff is
    r_colloid + thickness / 2.  (The full 101 slices: about 1 s of kernels.)"""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    params = MDParams(
        ureg=ureg,
        fluid_dyn_viscosity=ureg.Quantity(8.9e-4, "pascal * second"),
        WCA_epsilon=0.1 * ureg.Quantity(300, "kelvin") * ureg.boltzmann_constant,
        temperature=ureg.Quantity(300, "kelvin"),
        box_length=ureg.Quantity(3 * [50], "micrometer"),
        time_step=ureg.Quantity(0.0001, "second"),
        time_slice=ureg.Quantity(0.1, "second"),
        write_interval=ureg.Quantity(0.1, "second"),
    )
    runner = SwarmEngine(params, n_dims=2, out_folder=tmp_path, write_chunk_size=1)
    assert runner.colloids == []
    coll_rad = ureg.Quantity(1.0, "micrometer")
    runner.add_colloids(50, coll_rad, ureg.Quantity(np.array([25, 25, 0]), "micrometer"),
                        ureg.Quantity(25, "micrometer"), type_colloid=0)
    rod_thickness = ureg.Quantity(3, "micrometer")
    center_part = runner.add_rod(
        ureg.Quantity(np.array([25, 25, 0]), "micrometer"),
        ureg.Quantity(40, "micrometer"),
        rod_thickness,
        np.pi / 2.0,
        31,
        ureg.Quantity(10, "newton/ (meter / second)"),  # unused value because fixed
        ureg.Quantity(1e-17, "newton * meter * second"),
        2,
        fixed=True,
    )
    force_fn = ForceFunction(agents={"0": dummy_models.ConstForce(force=0)})
    runner.integrate(1, force_fn)
    center_before = np.copy(center_part.pos)
    director_before = np.copy(center_part.director)
    runner.integrate(100, force_fn)
    center_after = np.copy(center_part.pos)
    director_after = np.copy(center_part.director)

    np.testing.assert_allclose(center_before, center_after)
    assert np.linalg.norm(director_after - director_before) > 1e-3
    # the WCA cutoff between the differently sized particles: the engine's
    # pair table entry is (r_i + r_j)^2
    pc = runner._params_c
    s_c, s_r = runner._species_of[0], runner._species_of[50]
    assert pc.radius[s_c] + pc.radius[s_r] == (
        coll_rad.m_as("sim_length") + rod_thickness.m_as("sim_length") / 2)
    # the beads are still on the centre's line, the colloids outside the rod
    data = runner.get_particle_data()
    rod_pos, u = data["Unwrapped_Positions"][50:], data["Directors"][50]
    delta = (40.0 - 3.0) / 30
    for b in range(31):
        np.testing.assert_allclose(rod_pos[b], rod_pos[0] + rod_oracle.slot(b) * delta * u,
                                   atol=1e-5)
    runner.finalize()


def _colloid_lists(eng):
    """Per env the Colloid list of the downloaded raw state, in fp64."""
    from swarmrl_amd.components import Colloid

    raw = eng.get_raw_state()
    n = eng.n_particles
    lists = []
    for e in range(eng.n_envs):
        sl = slice(e * n, (e + 1) * n)
        pos = np.zeros((n, 3))
        for a in range(2):
            pos[:, a] = (raw["img"][a, sl].astype(np.float64)
                         + raw["q"][a, sl].astype(np.float64) / TWO32) * eng._box[a]
        th = raw["ang"][sl].astype(np.float64) * (2 * np.pi / TWO32)
        dirs = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1)
        lists.append([Colloid(pos[i], dirs[i], i, None, eng._types_list[i]) for i in range(n)])
    return lists


@pytest.mark.parametrize("direction", ["CCW", "CW"])
@pytest.mark.parametrize("partition", [True, False])
def test_rotate_rod_device_equals_list_path(tmp_path, direction, partition):
    """swarm_rod_reward against the numpy list path on the same downloaded
    states: E = 2, four calls with a history of 8 (the mean runs over the
    filled part only).  Both sides compute in fp64 and round to fp32 once."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.tasks import RotateRod

    ureg, eng = _engine(tmp_path, n_envs=2)
    pos, dirs = _ring((25.0, 25.0), 8.0, 24)
    _add_points(ureg, eng, pos, dirs, 1.0)
    _add_rod(ureg, eng, (25.0, 25.0), 20.0, 3.0, 0.3, 11, False)
    ff = ForceFunction({"0": dummy_models.ConstForce(5.0)})
    eng.integrate(1, ff)
    kw = dict(partition=partition, rod_type=2, particle_type=0, direction=direction,
              angular_velocity_scale=3, velocity_history=8)
    dev_task = RotateRod(**kw)
    list_tasks = [RotateRod(**kw) for _ in range(eng.n_envs)]
    dev_task.initialize(eng.swarm_view())
    for task, cols in zip(list_tasks, _colloid_lists(eng)):
        task.initialize(cols)
    for _ in range(4):
        eng.integrate(1, ff)
        got = dev_task(eng.swarm_view())
        assert got.shape == (2, 24) and got.dtype == torch.float32
        want = np.stack([task(cols) for task, cols in zip(list_tasks, _colloid_lists(eng))])
        assert np.all(want != 0.0)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-6, atol=0.0)


def test_vision_cone_sees_the_rod(tmp_path):
    """SubdividedVisionCones detecting the rod's type on a rod engine: the
    device view equals the list path, and a swimmer facing the rod sees it."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.components import Colloid
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.observables import SubdividedVisionCones

    ureg, eng = _engine(tmp_path)
    pos, dirs = _ring((25.0, 25.0), 8.0, 24)
    _add_points(ureg, eng, pos, dirs, 1.0)
    _add_rod(ureg, eng, (25.0, 25.0), 20.0, 3.0, 0.3, 11, True)
    eng.integrate(1, ForceFunction({"0": dummy_models.ConstForce(5.0)}))
    n = eng.n_particles
    radii = [1.0] * 24 + [1.5] * 11
    vc = SubdividedVisionCones(12.0, 0.6, 3, radii=radii, detected_types=[2], particle_type=0)
    dev = vc.compute_observable(eng.swarm_view())[0].cpu().numpy()
    data = eng.get_particle_data()
    cols = [Colloid(data["Unwrapped_Positions"][i], data["Directors"][i], i, None,
                    eng._types_list[i]) for i in range(n)]
    lst = np.stack(vc.compute_observable(cols))
    assert dev.shape == lst.shape == (24, 3, 1)
    # (the list path re-quantises fp64 positions: equal up to fp32 rounding,
    # except a bead exactly on a cone rim)
    assert (np.abs(dev - lst) > 1e-5).sum() <= 1
    # swimmer 6 sits about 8 um from the rod's flank and faces it
    assert dev[6].sum() > 0.0 and lst[6].sum() > 0.0


def test_training_with_rotate_rod(tmp_path):
    """ContinuousTrainer with RotateRod on the device path: 2 episodes of 3
    slices; finite rewards, and the network's weights change."""
    from swarmrl_amd.actions import Action
    from swarmrl_amd.agents import ActorCriticAgent
    from swarmrl_amd.networks import ActorCriticMLP, TorchModel
    from swarmrl_amd.observables import SubdividedVisionCones
    from swarmrl_amd.tasks import RotateRod
    from swarmrl_amd.trainers import ContinuousTrainer

    ureg, eng = _engine(tmp_path, n_envs=2)
    pos, dirs = _ring((25.0, 25.0), 8.0, 24)
    _add_points(ureg, eng, pos, dirs, 1.0)
    _add_rod(ureg, eng, (25.0, 25.0), 20.0, 3.0, 0.3, 11, True)
    net = TorchModel(ActorCriticMLP(3, 4, 32), input_shape=(3,), rng_key=3)
    before = [p.detach().clone() for p in net.model.parameters()]
    actions = {"a": Action(torque=np.array([0, 0, 10.0])), "b": Action(force=10.0),
               "c": Action(torque=np.array([0, 0, -10.0])), "d": Action()}
    agent = ActorCriticAgent(
        0, net, RotateRod(rod_type=2, particle_type=0, velocity_history=4),
        SubdividedVisionCones(12.0, np.pi / 2, 3, [1.0] * 24 + [1.5] * 11, detected_types=[2],
                              particle_type=0), actions)
    assert agent.supports_device()
    agent.loss.n_epochs = 2
    rewards = ContinuousTrainer([agent]).perform_rl_training(eng, n_episodes=2, episode_length=3,
                                                             load_bar=False)
    assert rewards.shape == (3,) and np.all(np.isfinite(rewards))
    after = list(net.model.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
