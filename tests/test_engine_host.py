"""
Host-side logic of the engine surface on CPU: the HIP backend is replaced by
a recording fake, so the Python mirror of espresso.py (units, validation,
placement, the slice/write schedule, trajectory holder, action marshalling)
is tested against the reference's known answers without a GPU.
"""

import ctypes

import numpy as np
import pytest

from oracle import refsem
from swarmrl_amd import _capi
from swarmrl_amd.agents import dummy_models
from swarmrl_amd.engine import swarm_engine
from swarmrl_amd.engine.swarm_engine import MDParams, SwarmEngine
from swarmrl_amd.force_functions import ForceFunction
from swarmrl_amd.units import UnitRegistry


class FakeNative:
    instances = []

    def __init__(self, params, n_envs, species):
        self.params = params
        self.n_envs = n_envs
        self.n = len(species)
        self.calls = []
        self.pos = None
        FakeNative.instances.append(self)

    def bind_stream(self):
        pass

    def call(self, name, *args):
        self.calls.append((name, args))
        M = self.n_envs * self.n
        if name == "swarm_engine_upload_state":
            self.pos = np.ctypeslib.as_array(ctypes.cast(args[0], ctypes.POINTER(ctypes.c_double)),
                                             (M * 3,)).copy()
            self.dirs = np.ctypeslib.as_array(ctypes.cast(args[1], ctypes.POINTER(ctypes.c_double)),
                                              (M * 3,)).copy()
        if name == "swarm_engine_download_state":
            for k, src in enumerate([self.pos, self.dirs]):
                dst = np.ctypeslib.as_array(ctypes.cast(args[k], ctypes.POINTER(ctypes.c_double)),
                                            (M * 3,))
                dst[:] = src
        if name == "swarm_engine_set_actions":
            f = np.ctypeslib.as_array(ctypes.cast(args[0], ctypes.POINTER(ctypes.c_float)), (M,))
            self.last_f = f.copy()
        if name == "swarm_engine_set_external_force":
            # the C side reads 3 M doubles through the pointer, whatever the caller allocated
            self.ext = np.ctypeslib.as_array(ctypes.cast(args[0], ctypes.POINTER(ctypes.c_double)),
                                             (M * 3,)).copy().reshape(self.n_envs, self.n, 3)

    def runs(self):
        return [a[0] for n, a in self.calls if n == "swarm_engine_integrate"]


@pytest.fixture
def fake_backend(monkeypatch):
    FakeNative.instances = []
    monkeypatch.setattr(swarm_engine, "_NativeEngine", FakeNative)
    monkeypatch.setattr(_capi, "require_gpu", lambda: None)
    # exercise the reference's list-of-Colloid callback path on CPU
    monkeypatch.setattr(SwarmEngine, "_device_capable", staticmethod(lambda fm: False))
    return FakeNative


def _engine(tmp_path, slice_steps, write_steps, seed=42, n_envs=1):
    ureg = UnitRegistry()
    dt = ureg.Quantity(0.1, "second")
    params = MDParams(
        ureg=ureg,
        fluid_dyn_viscosity=ureg.Quantity(8.9e-4, "pascal * second"),
        WCA_epsilon=ureg.Quantity(293, "kelvin") * ureg.boltzmann_constant,
        temperature=ureg.Quantity(293, "kelvin"),
        box_length=ureg.Quantity(3 * [10], "micrometer"),
        time_step=dt,
        time_slice=dt * slice_steps,
        write_interval=dt * write_steps,
    )
    eng = SwarmEngine(params, n_dims=2, seed=seed, out_folder=tmp_path, write_chunk_size=10,
                      n_envs=n_envs)
    eng.add_colloids(1, ureg.Quantity(0.2, "micrometer"),
                     ureg.Quantity(np.array([5, 5, 0]), "micrometer"),
                     ureg.Quantity(1, "micrometer"), type_colloid=0)
    return eng


# test_integration.py:107-160 (the three (slice, write) cases)
@pytest.mark.parametrize(
    "slice_, write, calls, expect",
    [
        (5, 9, [2, 3], [(10, 2, 2, 1.0, 2), (25, 5, 3, 2.5, 3)]),
        (7, 3, [4, 2], [(28, 4, 10, 2.8, 0), (42, 6, 14, 4.2, 4)]),
        (2, 2, [4, 2], [(8, 4, 4, 0.8, 4), (12, 6, 6, 1.2, 6)]),
    ],
)
def test_integration_schedule_kat(fake_backend, tmp_path, slice_, write, calls, expect):
    eng = _engine(tmp_path, slice_, write)
    ff = ForceFunction(agents={"0": dummy_models.ConstForce(1)})
    assert eng.params.steps_per_slice == slice_
    assert eng.params.steps_per_write_interval == write
    np.testing.assert_equal(eng.system.time, 0)
    for n, (step, sl, wr, t, tl) in zip(calls, expect):
        eng.integrate(n, ff)
        assert (eng.step_idx, eng.slice_idx, eng.write_idx) == (step, sl, wr)
        np.testing.assert_almost_equal(eng.system.time, t)
        assert len(eng.traj_holder["Times"]) == tl
    # the chunk sizes handed to the integrator follow the reference schedule
    ref = refsem.schedule(slice_, write, calls, write_chunk_size=10)[-1]["runs"]
    assert fake_backend.instances[0].runs() == ref
    # overlap removal ran once, before the first sub-step
    names = [c[0] for c in fake_backend.instances[0].calls]
    assert names.count("swarm_engine_remove_overlap") == 1
    assert names.index("swarm_engine_remove_overlap") < names.index("swarm_engine_integrate")
    eng.finalize()


def test_const_force_actions_marshalled(fake_backend, tmp_path):
    eng = _engine(tmp_path, 5, 9)
    eng.integrate(1, ForceFunction(agents={"0": dummy_models.ConstForce(2.5)}))
    assert np.all(fake_backend.instances[0].last_f == np.float32(2.5))


# ------------------- add_const_force_to_colloids (espresso.py:834-851, ext_force)
SIM_FORCE = refsem.SIM_ENERGY / 1e-6  # newton per simulation force unit
F_A = np.array([1.0e-13, -2.5e-13, 0.7e-13])  # newton
F_B = np.array([-3.1e-14, 4.0e-14, 9.9e-14])


@pytest.fixture
def composed(monkeypatch):
    """Every array SwarmEngine composes for swarm_engine_set_external_force
    is checked to be (n_envs, n_particles, 3), and to have the rows the
    backend will read, before the backend gets its pointer."""
    shapes = []
    orig = SwarmEngine._compose_ext_force

    def checked(self):
        ext = orig(self)
        assert ext.shape == (self.n_envs, len(self._types_list), 3)
        assert ext.dtype == np.float64
        if self._native is not None:
            assert ext.shape[:2] == (self._native.n_envs, self._native.n)
        shapes.append(ext.shape)
        return ext

    monkeypatch.setattr(SwarmEngine, "_compose_ext_force", checked)
    return shapes


def _add(eng, n, p_type):
    ureg = eng.ureg
    eng.add_colloids(n, ureg.Quantity(0.2, "micrometer"),
                     ureg.Quantity(np.array([5, 5, 0]), "micrometer"),
                     ureg.Quantity(1, "micrometer"), type_colloid=p_type)


def _two_type_engine(tmp_path, n_envs=2):
    eng = _engine(tmp_path, 5, 9, n_envs=n_envs)  # one colloid of type 0
    _add(eng, 2, 1)
    _add(eng, 1, 0)
    assert eng._types_list == [0, 1, 1, 0]
    return eng


def _force(eng, newton):
    return eng.ureg.Quantity(newton, "newton")


def _start(eng):
    eng.integrate(1)  # (the list path of a force function is single-env)


def _expect_ext(eng, by_type):
    types = np.asarray(eng._types_list)
    want = np.zeros((eng.n_envs, len(types), 3))
    for t, newton in by_type.items():
        want[:, types == t, :] = newton / SIM_FORCE
    return want


def test_ext_force_set_before_the_native_engine_exists(fake_backend, composed, tmp_path):
    """The force reaches the backend as [E * N][3] doubles in simulation
    units, on the colloids of the type only, the same in every env, and
    before the overlap removal (which sees it, as the reference's does)."""
    eng = _two_type_engine(tmp_path)
    eng.add_const_force_to_colloids(_force(eng, F_A), 1)
    assert not fake_backend.instances and composed == []  # nothing uploaded yet
    _start(eng)
    fake = fake_backend.instances[0]
    assert composed == [(2, 4, 3)]
    np.testing.assert_allclose(fake.ext, _expect_ext(eng, {1: F_A}), rtol=1e-6, atol=0)
    assert np.array_equal(fake.ext[0], fake.ext[1])
    assert np.all(fake.ext[:, [0, 3]] == 0.0) and np.all(fake.ext[:, [1, 2]] != 0.0)
    assert np.array_equal(fake.ext[0, 1], fake.ext[0, 2])
    names = [c[0] for c in fake.calls]
    assert names.count("swarm_engine_set_external_force") == 1
    assert names.index("swarm_engine_upload_state") < names.index(
        "swarm_engine_set_external_force") < names.index("swarm_engine_remove_overlap")


def test_ext_force_set_after_the_native_engine_exists(fake_backend, composed, tmp_path):
    eng = _two_type_engine(tmp_path)
    _start(eng)
    fake = fake_backend.instances[0]
    assert "swarm_engine_set_external_force" not in [c[0] for c in fake.calls]
    eng.add_const_force_to_colloids(_force(eng, F_A), 0)
    assert composed == [(2, 4, 3)]
    np.testing.assert_allclose(fake.ext, _expect_ext(eng, {0: F_A}), rtol=1e-6, atol=0)
    assert np.all(fake.ext[:, [1, 2]] == 0.0)


def test_ext_force_two_types_in_two_calls(fake_backend, composed, tmp_path):
    """One type before the native engine exists and one after it: both
    forces are in the second upload; a repeated call replaces its type's."""
    eng = _two_type_engine(tmp_path, n_envs=3)
    eng.add_const_force_to_colloids(_force(eng, F_A), 0)
    _start(eng)
    fake = fake_backend.instances[0]
    eng.add_const_force_to_colloids(_force(eng, F_B), 1)
    np.testing.assert_allclose(fake.ext, _expect_ext(eng, {0: F_A, 1: F_B}), rtol=1e-6, atol=0)
    assert fake.ext.shape == (3, 4, 3) and np.all(fake.ext != 0.0)
    eng.add_const_force_to_colloids(_force(eng, F_B), 0)
    np.testing.assert_allclose(fake.ext, _expect_ext(eng, {0: F_B, 1: F_B}), rtol=1e-6, atol=0)
    assert composed == 3 * [(3, 4, 3)]


def test_ext_force_survives_colloids_added_after_the_call(fake_backend, composed, tmp_path):
    """Colloids may be added between add_const_force_to_colloids and the
    first integrate.  The array handed to the backend has a row for every
    colloid the engine has then (it used to keep the size of the first call,
    so the backend read past it), a second call with more colloids works,
    and the force is on every colloid of the type."""
    eng = _two_type_engine(tmp_path)
    eng.add_const_force_to_colloids(_force(eng, F_A), 1)
    _add(eng, 3, 1)
    _add(eng, 2, 0)
    eng.add_const_force_to_colloids(_force(eng, F_B), 0)  # (IndexError from a stale mask)
    _add(eng, 1, 2)
    assert eng._types_list == [0, 1, 1, 0, 1, 1, 1, 0, 0, 2]
    _start(eng)
    fake = fake_backend.instances[0]
    assert composed == [(2, 10, 3)] and fake.n == 10
    np.testing.assert_allclose(fake.ext, _expect_ext(eng, {1: F_A, 0: F_B}), rtol=1e-6, atol=0)
    assert np.all(fake.ext[:, 9] == 0.0) and np.all(fake.ext[:, :9] != 0.0)


def test_ext_force_on_an_unknown_type_raises(fake_backend, composed, tmp_path):
    """espresso.py:846-850: no particle of the type."""
    eng = _two_type_engine(tmp_path)
    with pytest.raises(ValueError, match="Particles of type 7 not added to engine. "
                                         "You currently have"):
        eng.add_const_force_to_colloids(_force(eng, F_A), 7)
    _start(eng)
    with pytest.raises(ValueError, match="Particles of type 7 not added to engine"):
        eng.add_const_force_to_colloids(_force(eng, F_A), 7)
    # the refused calls left nothing behind
    assert composed == [] and eng._ext_force == {}
    assert "swarm_engine_set_external_force" not in [c[0] for c in fake_backend.instances[0].calls]


def test_placement_matches_reference_draw_order(tmp_path):
    ureg = UnitRegistry()
    params = MDParams(ureg=ureg, box_length=ureg.Quantity([100.0, 100.0, 100.0], "micrometer"))
    eng = SwarmEngine(params, n_dims=2, seed=42, n_envs=3)
    eng.add_colloids(20, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(np.array([50.0, 50.0, 0.0]), "micrometer"),
                     ureg.Quantity(30.0, "micrometer"))
    for e in range(3):
        pos, dirs = refsem.placement(20, 30.0, np.array([50.0, 50.0, 0.0]), 42 + e)
        np.testing.assert_allclose(np.stack(eng._pos[e]), pos, atol=1e-12)
        np.testing.assert_allclose(np.stack(eng._dir[e]), dirs, atol=1e-12)


def test_friction_and_units():
    ureg = UnitRegistry()
    params = MDParams(ureg=ureg, box_length=ureg.Quantity([100.0, 100.0, 100.0], "micrometer"))
    eng = SwarmEngine(params, n_dims=2)
    eng.add_colloids(2, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(np.array([50.0, 50.0, 0.0]), "micrometer"),
                     ureg.Quantity(10.0, "micrometer"), type_colloid=3)
    gt, gr = eng.get_friction_coefficients(3)
    rgt, rgr = refsem.friction(1e-3, 1.0)
    assert gt == pytest.approx(rgt, rel=1e-12) and gr == pytest.approx(rgr, rel=1e-12)
    assert eng._kT() == pytest.approx(300 / 293, rel=1e-12)
    assert params.WCA_epsilon.m_as("sim_energy") == pytest.approx(300 / 293, rel=1e-12)
    with pytest.raises(ValueError):
        eng.get_friction_coefficients(7)


def test_engine_validation_errors():
    ureg = UnitRegistry()
    with pytest.raises(ValueError):
        SwarmEngine(MDParams(ureg=ureg), n_dims=4)
    with pytest.raises(ValueError):
        SwarmEngine(MDParams(ureg=ureg, time_slice=ureg.Quantity(0.10005, "second")), n_dims=2)
    eng = SwarmEngine(MDParams(ureg=ureg), n_dims=2)
    eng.add_colloid_on_point(ureg.Quantity(1.0, "micrometer"),
                             ureg.Quantity(np.array([5.0, 5.0, 0.0]), "micrometer"))
    with pytest.raises(ValueError):  # same type, different radius
        eng.add_colloid_on_point(ureg.Quantity(2.0, "micrometer"),
                                 ureg.Quantity(np.array([9.0, 5.0, 0.0]), "micrometer"))
    with pytest.raises(ValueError):  # director out of plane in 2-D
        eng.add_colloid_on_point(ureg.Quantity(1.0, "micrometer"),
                                 ureg.Quantity(np.array([9.0, 5.0, 0.0]), "micrometer"),
                                 init_direction=np.array([0, 0, 1.0]))


def test_mutation_after_integrate_raises(fake_backend, tmp_path):
    eng = _engine(tmp_path, 5, 9)
    eng.integrate(1, ForceFunction(agents={"0": dummy_models.ConstForce(1)}))
    ureg = eng.ureg
    with pytest.raises(RuntimeError):
        eng.add_colloids(1, ureg.Quantity(0.2, "micrometer"),
                         ureg.Quantity(np.array([5, 5, 0]), "micrometer"),
                         ureg.Quantity(1, "micrometer"))


def test_trajectory_chunks_written(fake_backend, tmp_path):
    from swarmrl_amd.engine.trajectory_writer import read_trajectory

    eng = _engine(tmp_path, 2, 2)
    eng.write_chunk_size = 3
    eng.integrate(7, ForceFunction(agents={"0": dummy_models.ConstForce(1)}))
    eng.finalize()
    traj = read_trajectory(eng.h5_filename)
    assert traj["Unwrapped_Positions"].shape == (7, 1, 3)
    assert traj["Times"].shape == (7, 1, 1)
    np.testing.assert_allclose(traj["Times"][:, 0, 0], 0.2 * np.arange(7), atol=1e-12)


def test_placement_3d_matches_reference_draw_order(fake_backend, tmp_path):
    """3-D add_colloids (espresso.py:91-105, 521-529): r = R cbrt(U), two
    get_random_angles draws per colloid (position, then director)."""
    ureg = UnitRegistry()
    params = MDParams(ureg=ureg, box_length=ureg.Quantity(3 * [100.0], "micrometer"))
    eng = SwarmEngine(params, n_dims=3, seed=11, out_folder=tmp_path)
    center = np.array([50.0, 50.0, 50.0])
    eng.add_colloids(7, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(center, "micrometer"), ureg.Quantity(20.0, "micrometer"))
    pos, dirs = refsem.placement3(7, 20.0, center, 11)
    h = eng._host()
    np.testing.assert_allclose(h["pos"][0], pos, rtol=0, atol=1e-12)
    np.testing.assert_allclose(h["dir"][0], dirs, rtol=0, atol=1e-12)


def test_walls_registration_and_errors(fake_backend, tmp_path):
    """add_confining_walls / add_walls (espresso.py:667-800): type checks,
    2 * n_dims constraints for the box faces, one slab per wall segment, and
    the wall table handed to the engine at setup."""
    ureg = UnitRegistry()
    params = MDParams(ureg=ureg, box_length=ureg.Quantity(3 * [10.0], "micrometer"))
    eng = SwarmEngine(params, n_dims=3, out_folder=tmp_path)
    eng.add_colloids(5, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(np.array(3 * [5.0]), "micrometer"),
                     ureg.Quantity(4.0, "micrometer"), type_colloid=1)
    with pytest.raises(ValueError):
        eng.add_confining_walls(1)
    eng.add_confining_walls(2)
    assert len(eng.system.constraints) == 2 * eng.n_dims
    faces = [(w["normal"], w["offset"]) for w in eng._walls]
    assert ([-1, 0, 0], -10.0) in faces and ([0, 0, 1], 0.0) in faces

    eng2 = SwarmEngine(MDParams(ureg=ureg, box_length=ureg.Quantity(3 * [100.0], "micrometer")),
                       n_dims=2, out_folder=tmp_path)
    eng2.add_colloids(5, ureg.Quantity(1.0, "micrometer"),
                      ureg.Quantity(np.array([50.0, 50.0, 0.0]), "micrometer"),
                      ureg.Quantity(4.0, "micrometer"), type_colloid=1)
    start = ureg.Quantity(np.array([[40, 40], [40, 40], [60, 60], [60, 60]]), "micrometer")
    end = ureg.Quantity(np.array([[40, 60], [60, 40], [40, 60], [60, 40]]), "micrometer")
    with pytest.raises(ValueError):
        eng2.add_walls(start, end, 1, ureg.Quantity(2, "micrometer"))
    eng2.add_walls(start, end, 2, ureg.Quantity(2, "micrometer"))
    assert len(eng2.system.constraints) == 4
    w0 = eng2._walls[0]  # start (40, 40) -> end (40, 60), thickness 2
    np.testing.assert_allclose(w0["a"], [0, 20, 0])
    np.testing.assert_allclose(w0["b"], [2, 0, 0])
    np.testing.assert_allclose(w0["corner"], [39, 40, 0])
    eng2.integrate(1, ForceFunction({"1": dummy_models.ConstForce(1.0)}))
    names = [c[0] for c in fake_backend.instances[-1].calls]
    assert "swarm_engine_set_walls" in names


class _RingNative(FakeNative):
    """FakeNative whose device keeps recording while the host drains: every
    entry read advances the published count by `advance` (a replay still
    queued on the stream)."""

    advance = 0

    def call(self, name, *args):
        super().call(name, *args)
        if name == "swarm_traj_entry_to_host":
            self.ring["count"][0] += self.advance
            step = np.ctypeslib.as_array(ctypes.cast(args[4], ctypes.POINTER(ctypes.c_uint64)), (1,))
            step[0] = 0


def _ring_engine(monkeypatch, tmp_path, cap, count, advance):
    monkeypatch.setattr(swarm_engine, "_NativeEngine", _RingNative)
    eng = _engine(tmp_path, 2, 2)
    eng._setup_interactions()
    eng._init_h5_output()
    _RingNative.advance = advance
    eng._native.ring = eng._ring = {"ptr": 0, "cap": cap, "entry": 64, "drained": 0,
                                    "count": np.array([count], np.uint64)}
    eng._time_offset = 0.0
    return eng


@pytest.mark.parametrize("count,advance,block,ok", [
    (8, 0, True, True),     # stream drained: all cap entries readable
    (8, 0, False, False),   # cap entries with work in flight: entry 0 may be being overwritten
    (7, 0, False, True),
    (7, 1, False, False),   # the device publishes entry 8 while entry 0..6 are read
    (4, 1, False, True),    # count reaches 8 only after entry 3 (< 0 + cap) has been read
])
def test_trajectory_ring_overflow_is_detected(fake_backend, monkeypatch, tmp_path, count, advance,
                                              block, ok):
    """drain_trajectory(block=False) between graph replays: entry k of a ring
    of capacity cap is overwritten by entry k + cap, whose write starts as
    soon as the published count reaches k + cap -- so k is readable only
    while count < k + cap (the checks used count - start > cap)."""
    monkeypatch.setattr(swarm_engine.torch.cuda, "current_stream",
                        lambda: type("S", (), {"synchronize": lambda self: None})())
    eng = _ring_engine(monkeypatch, tmp_path, 8, count, advance)
    if ok:
        assert eng.drain_trajectory(block=block) == count
    else:
        with pytest.raises(RuntimeError, match="overflow"):
            eng.drain_trajectory(block=block)
