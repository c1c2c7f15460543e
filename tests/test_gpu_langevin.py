"""
The Langevin thermostat on the GPU: k_langevin_run (sub-steps and the overlap
removal) bit for bit against the CPU restatement tests/csrc/langevin_oracle.c
-- positions, image counters, angles, velocities -- with a flow field, a
potential and walls; the velocities through the product API; the reference's
test_flow_and_potential through SwarmEngine; the setters' refusals; and the
untouched Brownian path after a Langevin engine.
"""

import ctypes
import time

import numpy as np
import pytest
import torch

import langevin_oracle as lo
from oracle import oracle

pytestmark = pytest.mark.gpu

TWO32 = 4294967296.0
KT = EPS = 1.0239
DT = 0.005
# (radius, gamma_t, gamma_r, mass, rinertia): dt gamma / m = 0.04 and 0.033
SPECIES = [(0.5, 4.0, 6.0, 0.5, 0.8), (0.8, 6.0, 9.0, 0.9, 1.5)]
GAMMA_FLOW = 3.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


class Case:
    """An engine through the C ABI under the Langevin thermostat and the
    restatement's arguments for the same fields."""

    def __init__(self, box, species_of, n_envs, reuse=False, kT=KT, seed=17, flow=None,
                 potential=None, walls=None):
        from gpu_harness import Harness

        self.h = Harness(list(box), DT, kT, EPS, seed, SPECIES, species_of, n_envs=n_envs,
                         reuse=reuse)
        self.h.native.call("swarm_engine_set_langevin")
        self.sp = np.asarray(species_of, np.uint8)
        self.reuse = reuse
        self.kw = {}
        if walls:
            self.h.set_walls(walls)
            self.kw["walls"] = walls
        if potential is not None:
            phi, hs = potential
            phi = np.ascontiguousarray(phi, np.float32)
            hs = np.ascontiguousarray(hs, np.float64)
            self.h.native.call("swarm_engine_set_potential_field", phi.ctypes.data, phi.shape[0],
                               phi.shape[1], 1, hs.ctypes.data)
            self.kw["potential"] = (phi, hs)
        if flow is not None:
            u, hs = flow
            u = np.ascontiguousarray(u, np.float32)
            hs = np.ascontiguousarray(hs, np.float64)
            self.h.native.call("swarm_engine_set_flow_field", u.ctypes.data, u.shape[0],
                               u.shape[1], 1, hs.ctypes.data, GAMMA_FLOW)
            self.kw["flow"] = (u, GAMMA_FLOW)

    def velocities(self):
        M = self.h.E * self.h.n
        vel, om = np.zeros((3, M), np.float32), np.zeros(M, np.float32)
        self.h.native.call("swarm_engine_download_velocities", vel.ctypes.data, om.ctypes.data)
        return vel, om

    def assert_equal(self, states, vels, oms):
        got = self.h.download()
        vel, om = self.velocities()
        n = self.h.n
        for e, st in enumerate(states):
            for k in ("q", "img", "ang"):
                assert np.array_equal(got[e][k], st[k]), (k, e)
            assert np.array_equal(vel[:, e * n:(e + 1) * n], vels[e]), ("vel", e)
            assert np.array_equal(om[e * n:(e + 1) * n], oms[e]), ("omega", e)

    def run_bit_exact(self, states, slices=2, steps=25, sd_steps=0, min_pairs=1):
        """(overlap removal,) then `slices` runs of `steps` sub-steps with a
        swim force, a torque and a constant external force: q, img, ang, vel
        and omega of every particle equal the restatement after every run."""
        h, n, sp = self.h, self.h.n, self.sp
        rng = np.random.default_rng(3)
        f_swim = rng.uniform(2.0, 6.0, n).astype(np.float32)
        torque = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        f_ext = rng.uniform(-0.5, 0.5, (n, 3))
        f_ext[:, 2] = 0.0
        h.upload(states)
        h.set_external_force(np.tile(f_ext, (h.E, 1, 1)))
        fe = np.ascontiguousarray(f_ext.T, np.float32)
        vels = [np.zeros((3, n), np.float32) for _ in states]
        oms = [np.zeros(n, np.float32) for _ in states]
        if sd_steps:
            h.sd(sd_steps)
            states = [lo.sd_run(h.op, st, sp, sd_steps, f_ext=fe, **self.kw)[0] for st in states]
            self.assert_equal(states, vels, oms)  # (the velocities are still zero)
        h.set_actions(np.tile(f_swim, h.E), np.tile(torque, h.E))
        prev = [lo.ReuseForces(st) for st in states]
        pairs, viol = 0, 0
        for k in range(slices):
            h.integrate(steps)
            for e in range(h.E):
                args = (h.op, states[e], vels[e], oms[e], sp, f_swim, torque, steps)
                kw = dict(step0=k * steps, env=e, f_ext=fe, **self.kw)
                out = prev[e].run(*args, **kw) if self.reuse else lo.lv_run(*args, **kw)
                states[e], vels[e], oms[e], info = out
                pairs += info["pairs"]
                viol += info["violations"]
            self.assert_equal(states, vels, oms)
        assert pairs >= min_pairs, pairs
        assert all(np.any(v[:2] != 0.0) for v in vels) and all(np.any(w != 0.0) for w in oms)
        assert h.wall_violations() == viol
        return states, vels, oms


def _lattice_states(rng, n, box, jitter, n_envs, lo_=(0.0, 0.0)):
    """n particles on a jittered lattice over the box (shifted by lo_, folded
    into the box by the fixed-point conversion), random directors."""
    side = int(np.ceil(np.sqrt(n)))
    rows = int(np.ceil(n / side))
    out = []
    for _ in range(n_envs):
        k = np.arange(n)
        pos = np.stack([(k % side + 0.5) * (box[0] / side), (k // side + 0.5) * (box[1] / rows)], 1)
        pos = np.asarray(lo_) + pos + rng.uniform(-jitter, jitter, (n, 2))
        th = rng.uniform(0.0, 2.0 * np.pi, n)
        out.append(oracle.state_from_positions(
            np.concatenate([pos, np.zeros((n, 1))], 1),
            np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1), box))
    return out


def _fields(rng, box, shape=(8, 4)):
    hs = np.array([box[0] / shape[0], box[1] / shape[1], box[2]])
    u = rng.uniform(-2.0, 2.0, shape + (1, 3)).astype(np.float32)
    phi = rng.uniform(0.0, 2.0, shape + (1,)).astype(np.float32)
    return (u, hs), (phi, hs)


def _confining_walls(box):
    return [{"kind": 0, "normal": [1, 0, 0], "offset": 0.0},
            {"kind": 0, "normal": [-1, 0, 0], "offset": -box[0]},
            {"kind": 0, "normal": [0, 1, 0], "offset": 0.0},
            {"kind": 0, "normal": [0, -1, 0], "offset": -box[1]}]


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("with_flow", [True, False])
def test_langevin_run_bit_exact(with_flow, reuse):
    """2 envs x 300 particles of two species (radius, mass, frictions and
    inertia differ) at an area fraction of 0.3, an 8 x 4 flow field, an 8 x 4
    potential and confining walls; two runs of 25 sub-steps, so the
    velocities carry between launches."""
    rng = np.random.default_rng(201)
    box = [40.0, 35.0, 40.0]
    sp = np.arange(300) % 2
    phi_frac = sum(np.pi * SPECIES[s][0] ** 2 for s in sp) / (box[0] * box[1])
    assert 0.28 < phi_frac < 0.32
    flow, pot = _fields(rng, box)
    c = Case(box, sp, 2, reuse=reuse, flow=flow if with_flow else None, potential=pot,
             walls=_confining_walls(box))
    c.run_bit_exact(_lattice_states(rng, 300, box, 0.3, 2), min_pairs=300)


def test_more_particles_than_threads():
    """1100 particles in one env: a thread steps two of them and the strided
    loops over the velocity tail take a second pass."""
    rng = np.random.default_rng(202)
    box = [70.0, 70.0, 70.0]
    flow, pot = _fields(rng, box)
    c = Case(box, np.arange(1100) % 2, 1, reuse=True, flow=flow, potential=pot)
    c.run_bit_exact(_lattice_states(rng, 1100, box, 0.45, 1), slices=1, steps=10, min_pairs=100)


def test_grid_of_two_cells():
    """A 5 x 40 um box with the cutoff of 1.6: 2 x 16 cells, so both cells of
    a stencil row are one range and there is no wrap range; the two columns
    also meet through the periodic boundary in x."""
    rng = np.random.default_rng(203)
    n, box = 32, [5.0, 40.0, 40.0]
    flow, pot = _fields(rng, box)
    c = Case(box, np.arange(n) % 2, 2, reuse=True, flow=flow)
    assert oracle.cell_grid(c.h.op, n, 1.6) == (1, 4)
    states = []
    for _ in range(2):
        k = np.arange(n)
        pos = np.stack([1.25 + 2.5 * (k % 2), 1.0 + 2.0 * (k // 2), np.zeros(n)], 1)
        pos[:, :2] += rng.uniform(-0.5, 0.5, (n, 2))
        th = rng.uniform(0.0, 2.0 * np.pi, n)
        states.append(oracle.state_from_positions(
            pos, np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1), box))
    c.run_bit_exact(states, min_pairs=10)


def test_pairs_across_the_periodic_boundary():
    """The lattice shifted by half a box: particles within one cutoff of both
    periodic boundaries, image counters on both sides."""
    rng = np.random.default_rng(204)
    box = [24.0, 24.0, 24.0]
    flow, pot = _fields(rng, box)
    c = Case(box, np.arange(144) % 2, 2, flow=flow, potential=pot)
    states = _lattice_states(rng, 144, box, 0.45, 2, lo_=(12.0, 12.0))
    assert states[0]["img"][:2].min() == 0 and states[0]["img"][:2].max() == 1
    cut = 1.6 / 24.0 * TWO32
    assert np.any(states[0]["q"][0] < cut) and np.any(states[0]["q"][0] > TWO32 - cut)
    c.run_bit_exact(states, min_pairs=50)


def test_overlap_removal_from_an_overlapping_start():
    """96 particles dropped at random into a 20 um box: overlaps at the start;
    100 steepest-descent steps with the flow (at v = 0) and the potential
    equal the restatement and leave the velocities at zero, then the
    sub-steps."""
    rng = np.random.default_rng(205)
    n, box = 96, [20.0, 20.0, 20.0]
    flow, pot = _fields(rng, box)
    c = Case(box, np.arange(n) % 2, 2, flow=flow, potential=pot)
    states = []
    for _ in range(2):
        pos = np.concatenate([rng.uniform(0.0, 20.0, (n, 2)), np.zeros((n, 1))], 1)
        th = rng.uniform(0.0, 2.0 * np.pi, n)
        states.append(oracle.state_from_positions(
            pos, np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1), box))
    z3, z1 = np.zeros((3, n), np.float32), np.zeros(n, np.float32)
    _, _, _, info = lo.lv_run(c.h.op, states[0], z3, z1, c.sp, z1, z1, 1)
    assert info["pairs"] > 20  # (the start does overlap)
    # the flow moves a particle in the overlap removal: without it the result differs
    a = lo.sd_run(c.h.op, states[0], c.sp, 100, **c.kw)[0]
    b = lo.sd_run(c.h.op, states[0], c.sp, 100, potential=c.kw["potential"])[0]
    assert not np.array_equal(a["q"], b["q"])
    c.run_bit_exact(states, slices=1, steps=10, sd_steps=100, min_pairs=0)


def _product_engine(tmp_path, n_envs=1, thermostat="langevin", n_dims=2, periodic=True,
                    reuse_forces=True):
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    params = MDParams(
        ureg=ureg,
        fluid_dyn_viscosity=ureg.Quantity(8.9e-4, "pascal * second"),
        WCA_epsilon=ureg.Quantity(300, "kelvin") * ureg.boltzmann_constant,
        temperature=ureg.Quantity(300, "kelvin"),
        box_length=ureg.Quantity(3 * [40.0], "micrometer"),
        time_step=ureg.Quantity(DT, "second"),
        time_slice=ureg.Quantity(10 * DT, "second"),
        write_interval=ureg.Quantity(10 * DT, "second"),
        thermostat_type=thermostat,
        periodic=periodic,
    )
    return ureg, params, SwarmEngine(params, n_dims=n_dims, out_folder=tmp_path,
                                     write_chunk_size=1, n_envs=n_envs,
                                     reuse_forces=reuse_forces)


def _add(ureg, eng, n, mass=0.5, rinertia=0.8, gamma_t=4.0, gamma_r=6.0):
    eng.add_colloids(
        n, ureg.Quantity(0.5, "micrometer"), ureg.Quantity(np.array([20.0, 20.0, 0]), "micrometer"),
        ureg.Quantity(12.0, "micrometer"),
        gamma_translation=ureg.Quantity(gamma_t, "sim_force/sim_velocity"),
        gamma_rotation=ureg.Quantity(gamma_r, "sim_torque/sim_angular_velocity"),
        mass=ureg.Quantity(mass, "sim_mass"),
        rinertia=ureg.Quantity(3 * [rinertia], "sim_rinertia"))


def test_velocities_through_the_product_api(tmp_path):
    """get_raw_state(velocities=True) / set_raw_state(vel=, omega=): the round
    trip, and a slice from chosen velocities equals the restatement started
    from them (2 envs, a flow field added through add_flowfield)."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction

    ureg, params, eng = _product_engine(tmp_path, n_envs=2, reuse_forces=False)
    _add(ureg, eng, 48)
    rng = np.random.default_rng(7)
    u = rng.uniform(-2.0, 2.0, (8, 4, 1, 3))
    hs = np.array([5.0, 10.0, 40.0])
    eng.add_flowfield(ureg.Quantity(u, "sim_velocity"), ureg.Quantity(GAMMA_FLOW, "sim_mass/sim_time"),
                      ureg.Quantity(hs, "micrometer"))
    ff = ForceFunction({"0": dummy_models.ConstForce(5.0)})
    eng.integrate(1, ff)
    raw = eng.get_raw_state(velocities=True)
    n, M = eng.n_particles, 2 * eng.n_particles
    assert raw["vel"].shape == (3, M) and raw["omega"].shape == (M,)
    assert np.any(raw["vel"][:2] != 0.0) and np.all(raw["vel"][2] == 0.0)
    # get_particle_data reports the same (half-step) velocities
    np.testing.assert_array_equal(
        eng.get_particle_data()["Velocities"][0][:, :2].astype(np.float32), raw["vel"][:2, :n].T)
    vel = rng.normal(size=(3, M)).astype(np.float32)
    vel[2] = 0.0
    omega = rng.normal(size=M).astype(np.float32)
    eng.set_raw_state(raw["q"], raw["img"], raw["ang"], vel=vel, omega=omega)
    back = eng.get_raw_state(velocities=True)
    for k, want in (("q", raw["q"]), ("img", raw["img"]), ("ang", raw["ang"]), ("vel", vel),
                    ("omega", omega)):
        assert np.array_equal(back[k], want), k
    with pytest.raises(ValueError, match="together"):
        eng.set_raw_state(raw["q"], raw["img"], raw["ang"], vel=vel)
    eng.integrate(1, ff)
    got = eng.get_raw_state(velocities=True)
    (key,) = eng._species_keys
    p = oracle.make_params(eng._box, DT, eng._kT(), params.WCA_epsilon.m_as("sim_energy"),
                           eng.seed, [tuple(key)])
    sp = np.zeros(n, np.uint8)
    for e in range(2):
        sl = slice(e * n, (e + 1) * n)
        st = {"q": raw["q"][:, sl], "img": raw["img"][:, sl], "ang": raw["ang"][sl]}
        st, v, w, _ = lo.lv_run(p, st, vel[:, sl], omega[sl], sp, np.full(n, 5.0), np.zeros(n), 10,
                                step0=10, env=e, flow=(u, GAMMA_FLOW))
        for k in ("q", "img", "ang"):
            assert np.array_equal(got[k][..., sl], st[k]), (k, e)
        assert np.array_equal(got["vel"][:, sl], v) and np.array_equal(got["omega"][sl], w)
    assert eng.step_count() == 20
    eng.finalize()


def test_reference_flow_and_potential_through_the_product_api(tmp_path):
    """CI/espresso_tests/unit_tests/test_flow.py:14-158 verbatim: 10 colloids,
    a 100 x 100 x 1 flow and potential, ConstForceAndTorque, integrate(1000),
    and its two assertions: the swimmers are advected to the right (mean x >
    L / 2) and stay inside the arena (all x < L).  The restatement meets both
    from slice 1 on (tests/test_langevin_cpu.py) and runs the same 1000
    slices here, so the final state is also compared bit for bit."""
    import langevin_flow_case as fc

    ureg, runner, force_fn, box_l, case = fc.build(tmp_path)
    t0 = time.perf_counter()
    runner.integrate(1000, force_model=force_fn)
    poss = runner.get_particle_data()["Unwrapped_Positions"]
    print("integrate(1000) under the Langevin thermostat:", time.perf_counter() - t0, "s")
    np.testing.assert_array_less(box_l[0] / 2.0, np.mean(poss[:, 0]))
    np.testing.assert_array_less(poss[:, 0], box_l[0])
    got = runner.get_raw_state(velocities=True)
    st, vel, om = fc.restate(runner, case, 1000)
    for k in ("q", "img", "ang"):
        assert np.array_equal(got[k], st[k]), k
    assert np.array_equal(got["vel"], vel) and np.array_equal(got["omega"], om)
    assert runner.wall_violations() == 0
    runner.finalize()


def test_setters_refuse_what_the_kernel_cannot_run(tmp_path):
    from gpu_harness import Harness
    from swarmrl_amd import _capi

    def make(species=SPECIES[:1], n=8, box=40.0, **kw):
        return Harness([box] * 3, DT, KT, EPS, 1, species, np.zeros(n, int), **kw)

    u = np.zeros((4, 4, 1, 3), np.float32)
    hs = np.array([10.0, 10.0, 40.0])

    def set_flow(h, gamma=1.0, spacing=hs):
        h.native.call("swarm_engine_set_flow_field", u.ctypes.data, 4, 4, 1, spacing.ctypes.data,
                      float(gamma))

    h = make()
    h.integrate(1)
    with pytest.raises(RuntimeError, match="before the first integrate"):  # SWARM_ESTATE
        h.native.call("swarm_engine_set_langevin")
    with pytest.raises(ValueError, match="needs the Langevin thermostat"):  # a Brownian engine
        set_flow(h)
    # dt gamma_t / m = 0.005 * 4 / 0.005 = 4
    with pytest.raises(ValueError, match=r"dt \(gamma_t \+ gamma_flow\) / mass = 4\.0"):
        make(species=[(0.5, 4.0, 6.0, 0.005, 0.8)]).native.call("swarm_engine_set_langevin")
    with pytest.raises(ValueError, match=r"dt gamma_r / rinertia = 3\.0"):
        make(species=[(0.5, 4.0, 6.0, 0.5, 0.01)]).native.call("swarm_engine_set_langevin")
    with pytest.raises(ValueError, match="positive mass"):
        make(species=[(0.5, 4.0, 6.0, 0.0, 0.8)]).native.call("swarm_engine_set_langevin")
    with pytest.raises(ValueError, match="2-D only"):
        make(n_dims=3).native.call("swarm_engine_set_langevin")
    with pytest.raises(ValueError, match="periodic"):
        make(periodic=False).native.call("swarm_engine_set_langevin")
    big = make(n=4000, box=400.0)
    with pytest.raises(ValueError, match=r"at most 3\d\d\d particles"):
        big.native.call("swarm_engine_set_langevin")
    ok = make()
    ok.native.call("swarm_engine_set_langevin")
    with pytest.raises(ValueError, match="already"):
        ok.native.call("swarm_engine_set_langevin")
    set_flow(ok)
    with pytest.raises(ValueError, match="tile the box"):
        set_flow(ok, spacing=np.array([10.0, 9.0, 40.0]))
    # the flow's friction counts: dt (4 + 197) / 0.5 = 2.01
    with pytest.raises(ValueError, match="unstable Langevin step"):
        set_flow(ok, gamma=197.0)
    rod = _capi.SwarmRod()
    rod.first, rod.n, rod.delta, rod.fixed = 0, 3, 1.0, 1
    with pytest.raises(ValueError, match="Langevin"):
        ok.native.call("swarm_engine_set_rod", ctypes.byref(rod))
    ell = _capi.SwarmEllipsoids()
    ell.aspect_ratio = 3.0
    ell.gamma_par[0], ell.gamma_perp[0] = 4.0, 7.0
    with pytest.raises(ValueError, match="Langevin"):
        ok.native.call("swarm_engine_set_ellipsoids", ctypes.byref(ell))
    deferred = ctypes.c_int32(7)
    ok.native.call("swarm_engine_defer_build", ctypes.byref(deferred))
    assert deferred.value == 0
    ok.integrate(3)  # and the engine runs
    # the product API: the unstable ratio is a ValueError naming it, and the
    # capacity refusal states the limit
    ureg, params, eng = _product_engine(tmp_path / "a")
    _add(ureg, eng, 4, mass=0.005)
    with pytest.raises(ValueError, match=r"dt \(gamma_t \+ gamma_flow\) / mass"):
        eng.integrate(1)
    ureg, params, eng = _product_engine(tmp_path / "b")
    _add(ureg, eng, 4000)
    with pytest.raises(ValueError, match=r"at most \d+ particles per env"):
        eng.integrate(1)
    for kw, msg in ((dict(n_dims=3), "2d engines only"), (dict(periodic=False), "non-periodic")):
        ureg, params, eng = _product_engine(tmp_path / msg[:3], **kw)
        _add(ureg, eng, 4)
        with pytest.raises(NotImplementedError, match=msg):
            eng.integrate(1)
    ureg, params, eng = _product_engine(tmp_path / "rod")
    _add(ureg, eng, 4)
    with pytest.raises(NotImplementedError, match="a rod under the Langevin thermostat"):
        eng.add_rod(rod_center=ureg.Quantity(np.array([20, 20, 0]), "micrometer"),
                    rod_length=ureg.Quantity(10, "micrometer"),
                    rod_thickness=ureg.Quantity(1, "micrometer"), rod_start_angle=0.0,
                    n_particles=5, friction_rot=ureg.Quantity(1e-17, "newton * meter * second"),
                    rod_particle_type=2, fixed=True)


def test_spheres_after_a_langevin_engine_reproduce_the_golden_vectors():
    """A Brownian engine created after a Langevin engine in the same process
    runs the kernels it always ran: tests/golden/bd2d_wca.npz."""
    import pathlib

    from gpu_harness import Harness

    rng = np.random.default_rng(1)
    box = [24.0, 24.0, 24.0]
    c = Case(box, np.arange(96) % 2, 1, flow=_fields(rng, box)[0])
    c.h.upload(_lattice_states(rng, 96, box, 0.3, 1))
    c.h.integrate(3)
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
