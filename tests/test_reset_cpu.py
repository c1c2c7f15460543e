"""In-place reset on CPU: the placement's restatement against hand-computed
answers (tests/reset_ref.py, the reference of tests/test_gpu_reset.py), the
refusals SwarmEngine.reset_envs decides on the host, the reset plan it
derives from its add_* calls, and the episodic trainer's two reset paths on
the recording fake of test_engine_host."""

import ctypes

import numpy as np
import pytest

import reset_ref
from oracle import oracle
from swarmrl_amd import _capi
from swarmrl_amd.engine import MDParams, SwarmEngine
from swarmrl_amd.trainers import EpisodicTrainer
from swarmrl_amd.units import UnitRegistry
from test_engine_host import _engine, fake_backend  # noqa: F401 (fixture)
from test_trainers_cpu import _Learner


# ------------------------------------------------ the restatement's answers
def test_philox_restatement_matches_the_oracle():
    rng = np.random.default_rng(1)
    for _ in range(8):
        ctr = [int(v) for v in rng.integers(0, 2**32, 4)]
        key = [int(v) for v in rng.integers(0, 2**32, 2)]
        got = [int(v[0]) for v in reset_ref.philox4x32_10(ctr, key)]
        assert got == oracle.philox(ctr, key)


def _words(x, y, z, w):
    return [np.array([v], np.uint32) for v in (x, y, z, w)]


def test_place2_known_answers():
    box = [64.0, 64.0, 64.0]  # 2^32 / 64 = 2^26 fixed-point steps per unit
    # U1 = 1/2, U2 = 1/4: r = 8 max(U1, U2) = 4; polar angle 0 turns: (4, 0)
    q, img, ang = reset_ref.place2_from_words(
        _words(0x80000000, 0x40000000, 0, 0x12345678), [32.0, 16.0, 0.0], 8.0, box)
    assert q[:, 0].tolist() == [(1 << 31) + (1 << 28), 1 << 30]
    assert img[:, 0].tolist() == [0, 0]
    assert ang[0] == 0x12345678  # the director word is the angle
    # the low 8 bits of a radius word are not used: U1 = 1/2 still
    q2, _, _ = reset_ref.place2_from_words(
        _words(0x800000FF, 0x40000000, 0, 0), [32.0, 16.0, 0.0], 8.0, box)
    assert np.array_equal(q2, q)
    # a quarter turn: (0, 4); U2 = 3/4 > U1: r = 6 at half a turn: (-6, 0)
    q, img, _ = reset_ref.place2_from_words(
        _words(0x80000000, 0, 0x40000000, 0), [32.0, 16.0, 0.0], 8.0, box)
    assert q[:, 0].tolist() == [1 << 31, (1 << 30) + (1 << 28)]
    q, img, _ = reset_ref.place2_from_words(
        _words(0x80000000, 0xC0000000, 0x80000000, 0), [32.0, 16.0, 0.0], 8.0, box)
    assert q[:, 0].tolist() == [(1 << 31) - 6 * (1 << 26), 1 << 30]


def test_place2_folds_over_the_boundary():
    """A disc that reaches over the box edge: q wraps, the image counter counts."""
    box = [64.0, 64.0, 64.0]
    q, img, _ = reset_ref.place2_from_words(
        _words(0x80000000, 0, 0, 0), [62.0, 1.0, 0.0], 8.0, box)  # (+4, 0) from x = 62
    assert q[:, 0].tolist() == [2 * (1 << 26), 1 << 26] and img[:, 0].tolist() == [1, 0]
    q, img, _ = reset_ref.place2_from_words(
        _words(0x80000000, 0, 0xC0000000, 0), [62.0, 1.0, 0.0], 8.0, box)  # (0, -4) from y = 1
    assert q[:, 0].tolist() == [62 * (1 << 26), 61 * (1 << 26)] and img[:, 0].tolist() == [0, -1]
    # an unwrapped centre outside the box keeps its image
    q, img, _ = reset_ref.place2_from_words(
        _words(0, 0, 0, 0), [-3.0, 70.0, 0.0], 8.0, box)
    assert q[:, 0].tolist() == [61 * (1 << 26), 6 * (1 << 26)] and img[:, 0].tolist() == [-1, 1]


def test_place3_known_answers():
    box = [64.0, 64.0, 64.0]
    c = [32.0, 32.0, 32.0]
    # r = 8 max(1/4, 1/2, 1/8) = 4; z = 2 (1/2) - 1 = 0: in the plane, azimuth 0
    w1 = _words(0x40000000, 0x80000000, 0x20000000, 0)
    # director: z = 2 (3/4) - 1 = 1/2, azimuth a quarter turn: (0, sqrt(3)/2, 1/2)
    w2 = _words(0x80000000, 0xC0000000, 0x40000000, 0)
    q, img, d = reset_ref.place3_from_words(w1, w2, c, 8.0, box)
    assert q[:, 0].tolist() == [(1 << 31) + (1 << 28), 1 << 31, 1 << 31]
    assert not img.any()
    assert d[:, 0].tolist() == [0.0, float(np.sqrt(np.float32(0.75))), 0.5]
    # z = -1 (U = 0): the south pole, whatever the azimuth
    w2 = _words(0, 0, 0x12345678, 0)
    q, _, d = reset_ref.place3_from_words(w1, w2, c, 8.0, box)
    assert q[:, 0].tolist() == [1 << 31, 1 << 31, (1 << 31) - (1 << 28)]
    assert d[:, 0].tolist() == [0.0, 0.0, -1.0]


def test_place_env_groups_home_and_ordinal():
    box = [40.0, 40.0, 40.0]
    rng = np.random.default_rng(2)
    pos = np.zeros((9, 3))
    pos[:, :2] = rng.random((9, 2)) * 40
    home = oracle.state_from_positions(pos, np.tile([1.0, 0.0, 0.0], (9, 1)), box)
    groups = [(0, 4, [20.0, 20.0, 0.0], 5.0), (6, 3, [10.0, 10.0, 0.0], 0.0)]
    a = reset_ref.place_env(box, 2, 7, 0, 0, home, groups)
    b = reset_ref.place_env(box, 2, 7, 0, 1, home, groups)
    c = reset_ref.place_env(box, 2, 7, 1, 0, home, groups)
    for st in (a, b, c):  # outside every group, and the group of radius 0: home
        for k in ("q", "img", "ang"):
            assert np.array_equal(st[k][..., 4:], home[k][..., 4:])
        d = oracle.unwrapped(st, box)[:4, :2] - 20.0
        assert np.all(np.hypot(d[:, 0], d[:, 1]) <= 5.0 + 1e-6)
    # the ordinal and the env both change every draw
    assert not np.any(a["q"][0, :4] == b["q"][0, :4]) and not np.any(a["ang"][:4] == c["ang"][:4])


# --------------------------------------------------- host-side refusals
def _params(ureg, **kw):
    return MDParams(ureg=ureg, box_length=ureg.Quantity(3 * [100.0], "micrometer"),
                    time_step=ureg.Quantity(1e-3, "second"),
                    time_slice=ureg.Quantity(1e-2, "second"),
                    write_interval=ureg.Quantity(1e-2, "second"), **kw)


def test_reset_refusals_need_no_device(tmp_path, monkeypatch):
    """Decided on the host, before a device is asked for."""
    def no_device():
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(_capi, "require_gpu", no_device)
    monkeypatch.setattr(_capi, "lib", no_device)
    ureg = UnitRegistry()
    um = lambda v: ureg.Quantity(v, "micrometer")  # noqa: E731

    eng = SwarmEngine(_params(ureg), n_dims=2, out_folder=tmp_path)
    eng.add_colloids(3, um(1.0), um(np.array([50.0, 50.0, 0.0])), um(20.0))
    with pytest.raises(RuntimeError, match="integrate"):
        eng.reset_envs()  # nothing to reset yet

    eng = SwarmEngine(_params(ureg), n_dims=2, out_folder=tmp_path)
    eng.add_colloids(3, um(1.0), um(np.array([50.0, 50.0, 0.0])), um(20.0))
    eng.add_rod(um(np.array([50.0, 50.0, 0.0])), um(20.0), um(2.0), 0.0, 5,
                friction_rot=ureg.Quantity(1e-18, "newton * meter * second"),
                rod_particle_type=3)
    with pytest.raises(NotImplementedError, match="rod"):
        eng.reset_envs()

    eng = SwarmEngine(_params(ureg), n_dims=2, out_folder=tmp_path)
    eng.add_colloids(3, um(1.0), um(np.array([50.0, 50.0, 0.0])), um(20.0), aspect_ratio=2.0)
    with pytest.raises(NotImplementedError, match="ellipsoid"):
        eng.reset_envs()

    eng = SwarmEngine(_params(ureg, thermostat_type="langevin"), n_dims=2, out_folder=tmp_path)
    eng.add_colloids(3, um(1.0), um(np.array([50.0, 50.0, 0.0])), um(20.0),
                     mass=ureg.Quantity(1e-15, "kilogram"),
                     rinertia=ureg.Quantity(1e-27, "kilogram * meter**2"))
    with pytest.raises(NotImplementedError, match="Langevin"):
        eng.reset_envs()


# ------------------------------------------------------- the reset plan
def test_reset_plan_from_add_calls(tmp_path):
    ureg = UnitRegistry()
    um = lambda v: ureg.Quantity(v, "micrometer")  # noqa: E731
    eng = SwarmEngine(_params(ureg), n_dims=2, out_folder=tmp_path, n_envs=2)
    eng.add_colloids(5, um(1.0), um(np.array([30.0, 40.0, 0.0])), um(12.0), type_colloid=0)
    eng.add_colloid_on_point(um(2.0), um(np.array([70.0, 20.0, 0.0])), np.array([0.0, 1.0, 0.0]),
                             type_colloid=1)
    eng.add_colloids(3, um(1.5), um(np.array([60.0, 60.0, 0.0])), um(7.0), type_colloid=2)
    pos, dirs, groups = eng._reset_plan()
    assert pos.shape == dirs.shape == (2, 9, 3)
    assert [(g[0], g[1], g[3]) for g in groups] == [(0, 5, 12.0), (6, 3, 7.0)]
    assert groups[0][2].tolist() == [30.0, 40.0, 0.0] and groups[1][2].tolist() == [60.0, 60.0, 0.0]
    # the registered points are the home state, per env
    assert np.array_equal(pos, np.stack([np.stack(v) for v in eng._pos]))
    assert np.all(pos[:, 5] == [70.0, 20.0, 0.0]) and np.allclose(dirs[:, 5], [0.0, 1.0, 0.0])


def test_reset_envs_hands_the_plan_over_once(fake_backend, tmp_path):  # noqa: F811
    eng = _engine(tmp_path, 2, 2, n_envs=3)
    eng.integrate(1)
    eng._host()
    eng.reset_envs([2])
    eng.reset_envs(remove_overlap=False)
    assert eng._host_cache is None
    calls = [(n, a) for n, a in fake_backend.instances[-1].calls if "reset" in n]
    assert [n for n, _ in calls] == ["swarm_engine_set_reset_plan", "swarm_engine_reset_envs",
                                     "swarm_engine_reset_envs"]
    assert calls[0][1][3] == 1  # one add_colloids call: one group
    mask = np.ctypeslib.as_array(ctypes.cast(calls[1][1][0], ctypes.POINTER(ctypes.c_uint8)), (3,))
    assert mask.tolist() == [0, 0, 1] and calls[1][1][1:] == (1000, 0.1, 0.1)
    assert calls[2][1] == (None, 0, 0.1, 0.1)
    with pytest.raises(ValueError):
        eng.reset_envs([3])


# ---------------------------------------------------------- the trainer
def test_episodic_trainer_default_path_rebuilds(fake_backend, tmp_path):  # noqa: F811
    tags = []

    def get_engine(system, tag):
        tags.append(tag)
        return _engine(tmp_path / tag, 2, 2)

    EpisodicTrainer([_Learner()]).perform_rl_training(
        get_engine, None, n_episodes=3, episode_length=2, load_bar=False)
    assert tags == ["0", "1", "2"]
    assert not any("reset" in n for inst in fake_backend.instances for n, _ in inst.calls)


def test_episodic_trainer_reset_in_place(fake_backend, tmp_path):  # noqa: F811
    tags = []

    def get_engine(system, tag):
        tags.append(tag)
        eng = _engine(tmp_path, 2, 2)
        eng.h5_group_tag = tag  # (as SwarmEngine(..., h5_group_tag=tag))
        return eng

    learner = _Learner()
    trainer = EpisodicTrainer([learner])
    rewards = trainer.perform_rl_training(get_engine, None, n_episodes=5, episode_length=3,
                                          reset_frequency=2, load_bar=False, reset_in_place=True)
    assert tags == ["0"] and len(fake_backend.instances) == 1
    names = [n for n, _ in fake_backend.instances[0].calls]
    assert names.count("swarm_engine_reset_envs") == 2 and learner.resets == 3
    assert trainer.engine.h5_group_tag == "2" and rewards.shape == (6,)
    from swarmrl_amd.engine import trajectory_writer

    assert trajectory_writer.read_groups(trainer.engine.h5_filename) == ["0", "1", "2"]
