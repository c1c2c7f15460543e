"""
Envs that end their episodes on their own: swarm_engine_reset_marked (the
reset of the envs a device mask marks, with no host copy: placement bit for
bit against tests/reset_ref.py at the ordinal 2^63 | c_env, overlap removal
against the oracle, unmarked envs untouched to the bit, captured and replayed
with other mask contents, the run that follows), swarm_field_history_marked,
the slice schedule of SwarmEngine.set_auto_reset against the oracle and in a
captured graph, the done-aware fused PPO gradient (swarm_ppo_epoch_grad_ep and
its siblings) against torch autograd of the loss with the done-aware GAE, a
ContinuousTrainer on an auto-reset engine, and the refusals.

The helpers of tests/test_gpu_reset.py are imported, not restated.
"""

import ctypes

import numpy as np
import pytest
import torch

import potential_ref as pr
import reset_ref
from oracle import oracle
from test_gpu_reset import (SEED, WALLS, _assert_env_fresh, _assert_env_untouched, _env,
                            _everything, _field, _harness, _md_params, _reset, _set_plan, _start,
                            _stir)

pytestmark = pytest.mark.gpu

MARKED = 1 << 63


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


DEV = torch.device("cuda", 0)


def _mask(E, envs):
    m = torch.zeros(E, dtype=torch.uint8, device=DEV)
    if len(envs):
        m[list(envs)] = 1
    return m


def _mark(h, mask, sd_steps):
    h.native.bind_stream()
    h.native.call("swarm_engine_reset_marked", mask.data_ptr(), int(sd_steps), 0.1, 0.1)


def _counts(h):
    out = np.full(h.E, 99, np.uint32)
    h.native.bind_stream()
    h.native.call("swarm_engine_reset_counts", out.ctypes.data)
    return out.tolist()


# --------------------------------------------------------- placement, 2-D
def test_marked_placement_2d_counts_per_env():
    """E = 3, N = 70, two species, the groups of test_gpu_reset.  Masks
    {0, 2}, {0}, {1, 2} in turn, placement only: every marked env is the
    restatement at 2^63 | c_env (c_env counted here), every unmarked env
    identical to the bit in every array; an all-zero mask changes nothing,
    counts included; a host reset_envs in between draws with its own next
    ordinal and leaves the counts alone."""
    rng = np.random.default_rng(201)
    E, n, box = 3, 70, [40.0, 40.0, 40.0]
    sp = rng.integers(0, 2, n)
    h = _harness(box, sp, E)
    pos, dirs, states = _start(rng, E, n, box, 2, 2.0, 38.0)
    h.upload(states)
    h.sd(100)
    before = _stir(h, rng, 2)
    assert _counts(h) == [0, 0, 0]  # (no plan yet)
    groups = [(0, 40, [20.0, 20.0, 0.0], 6.0), (40, 29, [37.0, 3.0, 0.0], 8.0)]
    _set_plan(h, pos, dirs, groups)
    counts = [0] * E
    host_ordinal = 0

    def marked(envs):
        nonlocal before
        _mark(h, _mask(E, envs), 0)
        after = _everything(h)
        for e in range(E):
            if e not in envs:
                _assert_env_untouched(before, after, e, n)
                continue
            want = reset_ref.place_env(box, 2, SEED, e, MARKED | counts[e], states[e], groups)
            _assert_env_fresh(after, e, n, want, 2)
            assert not np.array_equal(_env(after["q"], e, n)[:, :69],
                                      _env(before["q"], e, n)[:, :69])
            counts[e] += 1
        assert _counts(h) == counts
        before = after

    marked((0, 2))
    marked(())  # an all-zero mask
    marked((0,))
    # the host path's stream is its own
    _reset(h, (1,), 0)
    after = _everything(h)
    want = reset_ref.place_env(box, 2, SEED, 1, host_ordinal, states[1], groups)
    _assert_env_fresh(after, 1, n, want, 2)
    for e in (0, 2):
        _assert_env_untouched(before, after, e, n)
    assert _counts(h) == counts
    before = after
    marked((1, 2))
    assert counts == [2, 1, 2]
    assert int(h.native._lib.swarm_engine_step_count(h.native.ptr)) == 20  # the noise goes on


# --------------------------------------------------------- placement, 3-D
@pytest.mark.parametrize("periodic", [True, False])
def test_marked_placement_3d(periodic):
    rng = np.random.default_rng(202)
    E, n, box = 2, 70, [40.0, 36.0, 44.0]
    sp = rng.integers(0, 2, n)
    h = _harness(box, sp, E, dims=3, periodic=periodic)
    pos, dirs, states = _start(rng, E, n, box, 3, 6.0, 30.0)
    h.upload(states)
    before = _stir(h, rng, 3)
    groups = [(1, 69, [36.0, 18.0, 22.0], 7.0)]
    _set_plan(h, pos, dirs, groups)
    for c in range(2):
        _mark(h, _mask(E, (1,)), 0)
        after = _everything(h)
        _assert_env_untouched(before, after, 0, n)
        want = reset_ref.place_env(box, 3, SEED, 1, MARKED | c, states[1], groups)
        _assert_env_fresh(after, 1, n, want, 3)
        assert np.array_equal(want["dir"][:, 0], states[1]["dir"][:, 0])  # particle 0: home
        before = after
    assert _counts(h) == [0, 2]


# ------------------------------------------------- masked overlap removal
@pytest.mark.parametrize("dims,periodic", [(2, True), (2, False), (3, True)])
def test_marked_overlap_removal_matches_the_oracle_per_env(dims, periodic):
    """The cases of test_gpu_reset's masked overlap removal with a device
    mask: 2-D periodic (the LDS body), 2-D non-periodic (the global body),
    3-D (k_global3_marked); the gridded potential acting, 200 steps."""
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
    _mark(h, _mask(E, (0, 2)), 200)
    after = _everything(h)
    _assert_env_untouched(before, after, 1, n)
    moved = 0
    for e in (0, 2):
        placed = reset_ref.place_env(box, dims, SEED, e, MARKED, states[e], groups)
        want = pr.sd_run_potential(h.op, placed, sp, 200, phi, inv_h, dims=dims)
        _assert_env_fresh(after, e, n, want, dims)
        moved += int((want["q"] != placed["q"]).sum())
    assert moved > n  # the placement did overlap
    assert _counts(h) == [1, 0, 1]
    # an all-zero mask with steps: nothing moves, though env 1 overlaps
    _mark(h, _mask(E, ()), 200)
    final = _everything(h)
    for k in after:
        assert np.array_equal(after[k], final[k]), k


# ---------------------------------------------------------------- captured
def test_captured_reset_replays_with_other_masks():
    """One swarm_engine_reset_marked with 100 steps in a graph, replayed three
    times with mask.copy_() in between: each replay equals the restatement
    with the advancing per-env counts, unmarked envs untouched."""
    rng = np.random.default_rng(203)
    E, n, box = 3, 70, [40.0, 40.0, 40.0]
    sp = rng.integers(0, 2, n)
    h = _harness(box, sp, E)
    pos, dirs, states = _start(rng, E, n, box, 2, 2.0, 38.0)
    h.upload(states)
    h.sd(100)
    before = _stir(h, rng, 2)
    groups = [(0, 45, [18.0, 20.0, 0.0], 5.0), (45, 24, [26.0, 21.0, 0.0], 3.0)]
    _set_plan(h, pos, dirs, groups)
    mask = _mask(E, ())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        _mark(h, mask, 100)
    torch.cuda.synchronize()
    after = _everything(h)
    for k in before:  # the capture ran nothing
        assert np.array_equal(before[k], after[k]), k
    counts = [0] * E
    for envs in ((0, 2), (1,), (0, 1)):
        mask.copy_(_mask(E, envs))
        g.replay()
        torch.cuda.synchronize()
        after = _everything(h)
        for e in range(E):
            if e not in envs:
                _assert_env_untouched(before, after, e, n)
                continue
            placed = reset_ref.place_env(box, 2, SEED, e, MARKED | counts[e], states[e], groups)
            want = oracle.sd_run(h.op, placed, sp, 100)[0]
            _assert_env_fresh(after, e, n, want, 2)
            counts[e] += 1
        assert _counts(h) == counts
        before = after
    del g


# ---------------------------------------------------------------- going on
def test_run_after_marked_reset_matches_the_oracle_on_the_cluster_path():
    """test_gpu_reset's run after a reset (reuse_forces, confining walls, the
    cluster windows) with a marked reset of {1}."""
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
    _mark(h, _mask(E, (1,)), 100)
    placed = reset_ref.place_env(box, 2, SEED, 1, MARKED, states[1], groups)
    cur[1] = oracle.sd_run(h.op, placed, sp, 100, walls=walls)[0]
    track[1] = oracle.ReuseForces(cur[1])
    assert int(h.native._lib.swarm_engine_step_count(h.native.ptr)) == step == 50
    run(25)
    run(25)
    fb, waves = h.window_stats()
    assert waves[0] > 0 and waves[2] > 0 and fb[0] == 0 and fb[2] == 0


# ----------------------------------------------------------------- history
def test_field_history_marked():
    """After moving, swarm_field_history_marked on {0, 2}: their history is
    the agents' current q / img, env 1's is unchanged to the bit."""
    rng = np.random.default_rng(204)
    E, n, box = 3, 70, [40.0, 40.0, 40.0]
    sp = rng.integers(0, 2, n)
    h = _harness(box, sp, E)
    _, _, states = _start(rng, E, n, box, 2, 2.0, 38.0)
    h.upload(states)
    h.sd(100)
    agents = np.nonzero(sp == 1)[0].astype(np.int32)
    A = len(agents)
    assert 0 < A < n
    idx = torch.as_tensor(agents, device=DEV)
    # an old history: recognisable values nothing else writes
    hq = torch.arange(3 * E * A, dtype=torch.int32, device=DEV).reshape(3, E * A) + 7
    hi = -hq
    hq0, hi0 = hq.cpu().numpy().copy(), hi.cpu().numpy().copy()
    _stir(h, rng, 2)
    h.native.bind_stream()
    h.native.call("swarm_field_history_marked", _mask(E, (0, 2)).data_ptr(), idx.data_ptr(), A,
                  hq.data_ptr(), hi.data_ptr())
    torch.cuda.synchronize()
    st = h.download()
    gq, gi = hq.cpu().numpy().view(np.uint32), hi.cpu().numpy()
    for e in range(E):
        sl = slice(e * A, (e + 1) * A)
        if e == 1:
            assert np.array_equal(gq[:, sl], hq0.view(np.uint32)[:, sl])
            assert np.array_equal(gi[:, sl], hi0[:, sl])
            continue
        assert np.array_equal(gq[:2, sl], st[e]["q"][:2, agents])
        assert np.array_equal(gi[:2, sl], st[e]["img"][:2, agents])
        assert not gq[2, sl].any() and not gi[2, sl].any()  # 2-D: no third axis


def _product_engine(tmp_path, n_envs, n=40, L=60.0, seed=9):
    from swarmrl_amd.engine import SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    um = lambda v: ureg.Quantity(v, "micrometer")  # noqa: E731
    eng = SwarmEngine(_md_params(ureg, L, time_slice=ureg.Quantity(1e-2, "second"),
                                 write_interval=ureg.Quantity(1e-2, "second")),
                      n_dims=2, seed=seed, out_folder=tmp_path, n_envs=n_envs)
    eng.add_colloids(n, um(1.0), um(np.array([25.0, 30.0, 0.0])), um(14.0), type_colloid=0)
    return eng


def test_histories_after_a_marked_reset_equal_a_fresh_initialize(tmp_path):
    """GradientSensing and ConcentrationField on a 3-env engine: after a
    marked reset of {0, 2} and reinitialize_envs, the next reward and
    observation of those envs are exactly what freshly initialised copies
    give; env 1 keeps its old history (and so differs from the copies)."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.observables import ConcentrationField
    from swarmrl_amd.tasks.searching import GradientSensing

    L = 60.0
    eng = _product_engine(tmp_path, 3, L=L)
    ff = ForceFunction({"0": dummy_models.ConstForce(8.0)})
    eng.integrate(1, ff)
    box = np.array([L, L, L])
    src = np.array([31.0, 28.0, 0.0])

    def make():
        return (GradientSensing(src, lambda d: 1 - d, box, 10, particle_type=0),
                ConcentrationField(src, lambda d: 1 - d, box, 100, particle_type=0))

    task, obs = make()
    view = eng.swarm_view()
    task.initialize(view)
    obs.initialize(view)
    eng.integrate(3, ff)
    mask = _mask(3, (0, 2))
    eng.reset_envs_where(mask)
    view = eng.swarm_view()
    task.reinitialize_envs(view, mask)
    obs.reinitialize_envs(view, mask)
    fresh_task, fresh_obs = make()
    fresh_task.initialize(view)
    fresh_obs.initialize(view)
    eng.integrate(2, ff)
    view = eng.swarm_view()
    r, o = task(view).cpu(), obs.compute_observable(view).cpu()
    fr, fo = fresh_task(view).cpu(), fresh_obs.compute_observable(view).cpu()
    for e in (0, 2):
        assert torch.equal(r[e], fr[e]) and torch.equal(o[e], fo[e]), e
    assert fo[1].abs().max() > 0
    assert not torch.equal(o[1], fo[1])  # env 1's history is three slices older
    assert eng.reset_counts().tolist() == [1, 0, 1]
    eng.finalize()


def test_pair_field_histories_refresh_marked_envs_only(tmp_path):
    """ParticleSensing and SpeciesSearch keep an [E, A] field history: the
    marked envs' rows become the current field, the others stay."""
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction
    from swarmrl_amd.observables.particle_sensing import ParticleSensing
    from swarmrl_amd.tasks.searching.species_search import SpeciesSearch

    L = 60.0
    eng = _product_engine(tmp_path, 3, L=L)
    ff = ForceFunction({"0": dummy_models.ConstForce(8.0)})
    eng.integrate(1, ff)
    box = np.array([L, L, L])
    items = [ParticleSensing(lambda d: 1 - d, box, sensing_type=0, particle_type=0),
             SpeciesSearch(lambda d: 1 - d, box, sensing_type=0, particle_type=0)]
    view = eng.swarm_view()
    for it in items:
        it.initialize(view)
    old = [it._dev_hist[1].clone() for it in items]
    eng.integrate(2, ff)
    mask = _mask(3, (1,))
    view = eng.swarm_view()
    for it, was in zip(items, old):
        it.reinitialize_envs(view, mask)
        now = it._field(view)
        assert torch.equal(it._dev_hist[1][1], now[1]) and not torch.equal(now[1], was[1])
        assert torch.equal(it._dev_hist[1][0], was[0]) and torch.equal(it._dev_hist[1][2], was[2])
    eng.finalize()


# ---------------------------------------------------------------- schedule
def _headline(seed=SEED, n_every=2):
    import argparse
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from swarmrl_amd.engine.termination import EverySlices

    N = 1024
    ns = argparse.Namespace(colloids=N, envs_per_gpu=1, write_interval=1.0)
    eng, ff, agent = bench.build_workload(ns, seed, DEV)
    eng.set_auto_reset(EverySlices(n_every))
    return eng, ff, agent, N


def _block(agent):
    t = agent.trajectory
    return {k: [torch.as_tensor(x).detach().cpu().numpy().copy() for x in getattr(t, k)]
            for k in ("actions", "rewards", "dones")}


def test_auto_reset_schedule_matches_the_oracle():
    """bench.build_workload at 1024 colloids, E = 1, EverySlices(2), 4 slices
    of one integrate call: rewards of every slice and the final state against
    the oracle's replay of the recorded actions, each reset restated as the
    placement at 2^63 | c + 1000 steps of steepest descent, the task's history
    taken from the fresh start; the terminal transition's reward comes from
    the pre-reset state.  dones is [0, 1, 0, 1]."""
    eng, ff, agent, N = _headline()
    pos0, dir0 = np.stack(eng._pos[0]), np.stack(eng._dir[0])
    eng.integrate(4, ff)
    blk = _block(agent)
    got = eng.get_raw_state()
    assert [int(d[0]) for d in blk["dones"]] == [0, 1, 0, 1]
    assert all(d.dtype == np.uint8 and d.shape == (1,) for d in blk["dones"])
    assert len(blk["rewards"]) == len(blk["actions"]) == 4
    assert eng.reset_counts().tolist() == [2]

    L = float(eng._box[0])
    box, src = np.array([L, L, L]), np.array([L / 2, L / 2, 0.0])
    p = oracle.make_params(eng._box, eng._time_step, eng._kT(),
                           eng.params.WCA_epsilon.m_as("sim_energy"), SEED, [eng._species_keys[0]])
    agents, sp = np.arange(N), np.zeros(N, np.uint8)
    ftab = np.array([0.0, 10.0, 0.0, 0.0], np.float32)
    ttab = np.array([10.0, 0.0, -10.0, 0.0], np.float32)
    f32 = np.float32
    home = oracle.state_from_positions(pos0, dir0, eng._box)
    hist = oracle.history_from_state(home, agents)  # the task saw the start
    st, _ = oracle.sd_run(p, home, sp, 1000)
    prev = {"f": np.zeros(N, f32), "t": np.zeros(N, f32), "ang": st["ang"].copy()}
    resets = 0
    for s in range(4):
        idx = blk["actions"][s].reshape(-1)
        f, t = ftab[idx], ttab[idx]
        st, _, _ = oracle.bd_run(p, st, sp, f, t, 100, step0=100 * s, prev=prev)
        prev = {"f": f, "t": t, "ang": st["ang"].copy()}
        dc, dp = oracle.field_distance(p, st, agents, src, box, hist, update=True)
        v = (f32(10.0) * ((f32(1.0) - dc) - (f32(1.0) - dp))).astype(f32)
        rew = np.where(v < 0, f32(0), v).astype(f32)
        assert np.array_equal(blk["rewards"][s].reshape(-1), rew), (s, "reward")
        if s % 2 == 1:  # done: the reset, then the history of the fresh start
            st = reset_ref.place_env(list(eng._box), 2, SEED, 0, MARKED | resets, home,
                                     eng._reset_groups)
            st, _ = oracle.sd_run(p, st, sp, 1000)
            hist = oracle.history_from_state(st, agents)
            prev = {"f": np.zeros(N, f32), "t": np.zeros(N, f32), "ang": st["ang"].copy()}
            resets += 1
    for key in ("q", "img", "ang"):
        assert np.array_equal(got[key], st[key]), key
    eng.finalize()


def test_auto_reset_schedule_captured_equals_eager():
    """Two equal engines run 4 eager slices; then 4 more, eagerly on one and
    as one captured graph replayed on the other: actions, rewards, dones, the
    final state and the reset counts are the same bits."""
    out = []
    for mode in ("eager", "graph"):
        eng, ff, agent, _ = _headline()
        eng.integrate(4, ff)
        agent.reset_trajectory()
        torch.cuda.synchronize()
        if mode == "graph":
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                eng.integrate(4, ff)
            g.replay()
            torch.cuda.synchronize()
        else:
            eng.integrate(4, ff)
        out.append((_block(agent), eng.get_raw_state(), eng.reset_counts().tolist()))
        if mode == "graph":
            del g
        eng.finalize()
    (ba, sa, ca), (bb, sb, cb) = out
    assert ca == cb == [4]
    assert [int(d[0]) for d in ba["dones"]] == [0, 1, 0, 1]
    for k in ba:
        assert len(ba[k]) == len(bb[k]) == 4
        for x, y in zip(ba[k], bb[k]):
            assert np.array_equal(x, y), k
    for k in ("q", "img", "ang"):
        assert np.array_equal(sa[k], sb[k]), k


# -------------------------------------------------------------- GAE, fused
def _dones(T, E):
    """Env 0: ends at t = 0 and T - 1; env 1: two consecutive ends; env 2: none."""
    d = torch.zeros(T, E, dtype=torch.uint8)
    d[0, 0] = d[T - 1, 0] = 1
    d[T // 2, 1] = d[T // 2 + 1, 1] = 1
    return d.to(DEV)


def _split(flat, layers):
    out, off = [], 0
    for t in layers:
        out.append(flat[off:off + t.numel()].view_as(t))
        off += t.numel()
    assert off == flat.numel()
    return out


@pytest.mark.parametrize("T", [5, 40])  # the register form and the loop form
@pytest.mark.parametrize("deep", [False, True])
def test_fused_epoch_grad_with_dones_matches_autograd(T, deep):
    """S = 3 envs x 7 agents.  The gradient of swarm_ppo_epoch_grad_ep (deep:
    swarm_ppo_deep_epoch_grad_ep) against torch autograd of the loss with the
    done-aware GAE, within the tolerance of test_gpu_ppo's
    test_fused_epoch_grad_matches_autograd; with all-zero dones each sibling
    is bit-identical to its existing entry."""
    import test_gpu_deep_ppo as deep_ppo
    import test_gpu_ppo as ppo
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    E, A = 3, 7
    S = E * A
    loss = ProximalPolicyLoss()
    if deep:
        net, x, actions, old, rewards = deep_ppo._episode(T, S, 3, 4, (24, 16), seed=T)
        layers, wrap = deep_ppo._flat_layers(net), deep_ppo._Wrap(net)
    else:
        net, x, actions, old, rewards = ppo._episode(T, S, 3, 4, 100, seed=T)
        layers, wrap = net.ppo_layers(), ppo._Wrap(net)
    dones = _dones(T, E)
    args = (x, actions, old, rewards, layers, loss.value_function.gamma,
            loss.value_function.lambda_, loss.epsilon, loss.entropy_coefficient)

    net.zero_grad(set_to_none=True)
    loss._calculate_loss(wrap, x, actions, rewards, old, dones).backward()
    want = [p.grad.detach().clone() for p in layers]
    net.zero_grad(set_to_none=True)
    loss._calculate_loss(wrap, x, actions, rewards, old).backward()
    plain = [p.grad.detach().clone() for p in layers]

    got = _split(ops.ppo_epoch_grad(*args, dones=dones), layers)
    differs = False
    for name, a, b, c in zip(range(len(layers)), got, want, plain):
        err = (a - b).norm().item()
        print(f"T={T} deep={deep} tensor {name}: norm err {err:.3e} of {b.norm().item():.3e}, "
              f"max err {(a - b).abs().max().item():.3e} of {b.abs().max().item():.3e}")
        assert err <= 2e-4 * b.norm().item() + 1e-6, (name, err, b.norm().item())
        assert (a - b).abs().max().item() <= 2e-3 * b.abs().max().item() + 1e-6, name
        differs = differs or (b - c).norm().item() > 1e-2 * c.norm().item()
    assert differs  # the cut is well outside the tolerance

    zero = torch.zeros_like(dones)
    assert torch.equal(ops.ppo_epoch_grad(*args, dones=zero), ops.ppo_epoch_grad(*args))
    # per_env = S: one env's flags over every column
    one = dones[:, :1].contiguous()
    assert not torch.equal(ops.ppo_epoch_grad(*args, dones=one), ops.ppo_epoch_grad(*args))
    for bad in (zero[:, :2], zero[:-1], zero.to(torch.int32), zero.cpu()):
        with pytest.raises(ValueError):
            ops.ppo_epoch_grad(*args, dones=bad)


def test_fused_adam_step_with_dones(monkeypatch):
    """swarm_ppo_epoch_step_ep: with all-zero dones bit-identical to
    swarm_ppo_epoch_step (parameters and gradient); with dones the gradient it
    leaves is that of swarm_ppo_epoch_grad_ep."""
    import test_gpu_ppo as ppo
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    T, E, A = 5, 3, 7
    loss = ProximalPolicyLoss()
    dones = _dones(T, E)
    res = {}
    for tag, dn in (("none", None), ("zero", torch.zeros_like(dones)), ("dones", dones)):
        net, x, actions, old, rewards = ppo._episode(T, E * A, 3, 4, 100, seed=3)
        layers = net.ppo_layers()
        opt = torch.optim.Adam(layers, lr=1e-3, capturable=True)
        for p in layers:
            p.grad = torch.zeros_like(p)
        opt.step()  # the state tensors, as the first eager episode leaves them
        adam = ops.adam_args(opt, layers)
        assert adam is not None
        args = (x, actions, old, rewards, layers, loss.value_function.gamma,
                loss.value_function.lambda_, loss.epsilon, loss.entropy_coefficient)
        want = ops.ppo_epoch_grad(*args, dones=dn).clone()
        grad = ops.ppo_epoch_grad(*args, adam=adam, dones=dn)
        torch.cuda.synchronize()
        assert torch.equal(grad, want), tag
        res[tag] = [p.detach().clone() for p in layers]
    for a, b, c in zip(res["none"], res["zero"], res["dones"]):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, c) for a, c in zip(res["none"], res["dones"]))


def _episode_with_dones(T, E, A, d, seed):
    g = torch.Generator().manual_seed(seed)
    dn = _dones(T, E)

    class Episode:
        features = [f.to(DEV) for f in torch.randn(T, E, A, d, generator=g)]
        actions = [a.to(DEV) for a in torch.randint(0, 4, (T, E, A), generator=g)]
        rewards = [r.to(DEV) for r in torch.randn(T, E, A, generator=g)]
        log_probs = [lp.to(DEV) for lp in -1.386 + 0.3 * torch.randn(T, E, A, generator=g)]
        dones = [row for row in dn]
    return Episode()


def test_compute_loss_with_dones_fused_equals_torch_path(monkeypatch):
    """Two epochs of compute_loss with SGD on an episode with dones: the fused
    path and the torch path end on the same parameters (the criterion of
    test_gpu_ppo's test_compute_loss_fused_equals_torch_path), and not where
    the same episode without dones ends."""
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss
    from swarmrl_amd.networks.torch_network import ActorCriticMLP, TorchModel

    T, E, A, d = 12, 3, 50, 1
    steps = {}
    for tag, fused, with_dones in (("fused", "1", True), ("torch", "0", True),
                                   ("plain", "1", False)):
        monkeypatch.setenv("SWARMRL_AMD_FUSED_PPO", fused)
        torch.manual_seed(0)
        model = TorchModel(ActorCriticMLP(d, 4, 128), input_shape=(d,), device=DEV,
                           optimizer=lambda ps: torch.optim.SGD(ps, lr=1e-4))
        before = [p.detach().clone() for p in model.model.ppo_layers()]
        ep = _episode_with_dones(T, E, A, d, 11)
        if not with_dones:
            ep.dones = []
        ProximalPolicyLoss(n_epochs=2).compute_loss(model, ep)
        steps[tag] = [p.detach() - b for p, b in zip(model.model.ppo_layers(), before)]
    apart = False
    for a, b, c in zip(steps["fused"], steps["torch"], steps["plain"]):
        assert (a - b).norm().item() <= 1e-3 * b.norm().item() + 1e-7
        apart = apart or (a - c).norm().item() > 1e-2 * c.norm().item()
    assert apart


def test_graph_epochs_with_dones_equal_eager(monkeypatch):
    """Three episodes with dones (their ends moving from episode to episode):
    the captured-graph epochs end on bit-identical parameters to the eager
    loop; the graph's signature records that dones are present, and an episode
    without dones afterwards recaptures."""
    monkeypatch.setenv("SWARMRL_AMD_FUSED_ADAM", "0")
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss
    from swarmrl_amd.networks.torch_network import ActorCriticMLP, TorchModel

    T, E, A, d = 12, 3, 40, 4

    def episode(k):
        ep = _episode_with_dones(T, E, A, d, 100 + k)
        ep.dones = [torch.roll(row, k) for row in ep.dones]
        return ep

    finals = []
    for graph in ("1", "0"):
        monkeypatch.setenv("SWARMRL_AMD_PPO_GRAPH", graph)
        torch.manual_seed(0)
        model = TorchModel(ActorCriticMLP(d, 4, 128), input_shape=(d,), device=DEV)
        loss = ProximalPolicyLoss(n_epochs=3)
        for k in range(3):
            loss.compute_loss(model, episode(k))
        if graph == "1":
            assert loss._ppo_graph is not None and len(loss._ppo_graph["inputs"]) == 5
            assert loss._ppo_graph["inputs"][4] is not None
            assert (T, E) in loss._ppo_graph["sig"]
            first = loss._ppo_graph["graph"]
        ep = episode(3)
        ep.dones = []
        loss.compute_loss(model, ep)
        if graph == "1":
            assert loss._ppo_graph["graph"] is not first and loss._ppo_graph["inputs"][4] is None
        finals.append([p.detach().clone() for p in model.model.ppo_layers()])
    for a, b in zip(*finals):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- training
def _learner(n, L, E):
    from swarmrl_amd.actions import Action
    from swarmrl_amd.agents import ActorCriticAgent
    from swarmrl_amd.networks import ActorCriticMLP, TorchModel
    from swarmrl_amd.observables import ConcentrationField
    from swarmrl_amd.tasks.searching import GradientSensing

    box = np.array([L, L, L])
    src = np.array([L / 2, L / 2, 0.0])
    task = GradientSensing(src, lambda d: 1 - d, box, 10, particle_type=1)
    obs = ConcentrationField(src, lambda d: 1 - d, box, 100, particle_type=1)
    net = TorchModel(ActorCriticMLP(1, 4, 32), input_shape=(1,), rng_key=3)
    actions = {"a": Action(torque=np.array([0, 0, 10.0])), "b": Action(force=10.0),
               "c": Action(torque=np.array([0, 0, -10.0])), "d": Action()}
    agent = ActorCriticAgent(1, net, task, obs, actions)
    agent.loss.n_epochs = 2
    return agent


def _train_engine(tmp_path, n, L, E):
    from swarmrl_amd.engine import SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    eng = SwarmEngine(_md_params(ureg, L, time_slice=ureg.Quantity(0.1, "second"),
                                 write_interval=ureg.Quantity(0.1, "second")),
                      n_dims=2, seed=42, out_folder=tmp_path, n_envs=E)
    eng.add_colloids(n, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(np.array([L / 2, L / 2, 0.0]), "micrometer"),
                     ureg.Quantity(L / 2 - 2, "micrometer"), type_colloid=1)
    return eng


def test_continuous_trainer_on_an_auto_reset_engine(tmp_path):
    """2 envs x 200 colloids, EverySlices(3, offset_per_env=1), 2 episodes of
    6 slices: finite rewards, dones stack to [6, 2] per episode and their sum
    is the increase of reset_counts."""
    from swarmrl_amd.engine.termination import EverySlices
    from swarmrl_amd.trainers import ContinuousTrainer

    n, L, E = 200, 100.0, 2
    eng = _train_engine(tmp_path, n, L, E)
    eng.set_auto_reset(EverySlices(3, offset_per_env=1))
    agent = _learner(n, L, E)
    seen = []
    update = agent.update_agent

    def recording(*a, **kw):
        seen.append(torch.stack(agent.trajectory.dones).cpu())
        return update(*a, **kw)

    agent.update_agent = recording
    rewards = ContinuousTrainer([agent]).perform_rl_training(eng, 2, 6, load_bar=False)
    assert rewards.shape == (3,) and np.all(np.isfinite(rewards))
    assert len(seen) == 2 and all(tuple(d.shape) == (6, 2) and d.dtype == torch.uint8
                                  for d in seen)
    # env 0 at calls 3, 6, 9, 12; env 1 at calls 2, 5, 8, 11
    assert seen[0].T.tolist() == [[0, 0, 1, 0, 0, 1], [0, 1, 0, 0, 1, 0]]
    assert seen[1].T.tolist() == [[0, 0, 1, 0, 0, 1], [0, 1, 0, 0, 1, 0]]
    total = torch.stack(seen).sum(dim=(0, 1)).tolist()
    assert eng.reset_counts().tolist() == total == [4, 4]
    assert agent.trajectory.dones == []  # a new trajectory after the update
    eng.finalize()


# ---------------------------------------------------------------- refusals
def test_native_refusals():
    from swarmrl_amd import _capi

    rng = np.random.default_rng(207)
    E, n, box = 2, 20, [40.0, 40.0, 40.0]
    sp = np.zeros(n, int)
    pos, dirs, states = _start(rng, E, n, box, 2, 2.0, 38.0)
    c = [20.0, 20.0, 0.0]
    mask = _mask(E, (0,))

    h = _harness(box, sp, E)
    h.upload(states)
    with pytest.raises(RuntimeError, match="reset plan"):  # SWARM_ESTATE
        _mark(h, mask, 0)
    _set_plan(h, pos, dirs, [(0, 5, c, 5.0)])
    with pytest.raises(ValueError):
        _mark(h, mask, -1)
    with pytest.raises(ValueError, match="null mask"):
        h.native.call("swarm_engine_reset_marked", None, 0, 0.1, 0.1)
    with pytest.raises(ValueError):
        h.native.call("swarm_engine_reset_counts", None)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    buf = torch.zeros(3, E, dtype=torch.int32, device=DEV)
    for args in ((None, idx.data_ptr(), 1, buf.data_ptr(), buf.data_ptr()),
                 (mask.data_ptr(), None, 1, buf.data_ptr(), buf.data_ptr()),
                 (mask.data_ptr(), idx.data_ptr(), 1, None, buf.data_ptr()),
                 (mask.data_ptr(), idx.data_ptr(), 1, buf.data_ptr(), None)):
        with pytest.raises(ValueError):
            h.native.call("swarm_field_history_marked", *args)

    def refused(prepare, dt=1e-3):
        hh = _harness(box, sp, E, reuse=False, dt=dt)
        hh.upload(states)
        prepare(hh)
        _set_plan(hh, pos, dirs, [(0, 5, c, 5.0)])
        with pytest.raises(ValueError, match="rod, ellipsoids or the Langevin"):
            _mark(hh, mask, 0)

    rod = _capi.SwarmRod()
    rod.first, rod.n, rod.delta, rod.fixed = 0, 5, 1.0, 1
    refused(lambda hh: hh.native.call("swarm_engine_set_rod", ctypes.byref(rod)))
    ell = _capi.SwarmEllipsoids()
    ell.aspect_ratio = 1.0
    for s in range(2):
        ell.gamma_par[s], ell.gamma_perp[s] = 4.0, 6.0
    refused(lambda hh: hh.native.call("swarm_engine_set_ellipsoids", ctypes.byref(ell)))
    refused(lambda hh: hh.native.call("swarm_engine_set_langevin"), dt=5e-8)


def test_engine_mask_refusals_and_capture_without_a_plan(tmp_path):
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction

    eng = _product_engine(tmp_path, 2)
    with pytest.raises(RuntimeError, match="integrate"):
        eng.reset_envs_where(_mask(2, ()))
    eng.integrate(1, ForceFunction({"0": dummy_models.ConstForce(5.0)}))
    for bad in (torch.zeros(2, dtype=torch.int32, device=DEV),
                torch.zeros(2, dtype=torch.bool, device=DEV),
                torch.zeros(3, dtype=torch.uint8, device=DEV),
                torch.zeros(2, 1, dtype=torch.uint8, device=DEV),
                torch.zeros(4, dtype=torch.uint8, device=DEV)[::2],
                torch.zeros(2, dtype=torch.uint8), np.zeros(2, np.uint8)):
        with pytest.raises(ValueError, match="mask"):
            eng.reset_envs_where(bad)
    assert eng.reset_counts().tolist() == [0, 0]
    # under capture without a plan: refused before anything is captured
    mask = _mask(2, (1,))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="reset plan"):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            mask.add_(0)  # (the capture is not empty)
            eng.reset_envs_where(mask)
    del g
    torch.cuda.synchronize()
    before = eng.get_raw_state()
    eng.reset_envs_where(mask)  # and outside it sets the plan
    after = eng.get_raw_state()
    N = eng.n_particles
    assert np.array_equal(before["q"][:, :N], after["q"][:, :N])
    assert not np.array_equal(before["q"][:, N:], after["q"][:, N:])
    assert eng.reset_counts().tolist() == [0, 1]
    eng.finalize()


def test_out_of_scope_trainers_refuse_dones(tmp_path):
    """EnsembleTrainer (and with it GeneticTraining) and EpisodeParallelTrainer
    raise when an agent's episode has dones, before any update."""
    from swarmrl_amd.trainers import EnsembleTrainer, EpisodeParallelTrainer

    agent = _learner(20, 60.0, 2)
    agent.trajectory.dones.append(_mask(2, (0,)))
    with pytest.raises(ValueError, match="EpisodeParallelTrainer does not support"):
        EpisodeParallelTrainer([agent])._update_agent(agent)
    ens = object.__new__(EnsembleTrainer)
    ens.agents, ens.n_members = {"1": agent}, 1
    with pytest.raises(ValueError, match="EnsembleTrainer does not support"):
        ens.update_rl()
