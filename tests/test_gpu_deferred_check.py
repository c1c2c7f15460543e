"""
A window's exact check riding in the reward launch (SWARMRL_AMD_DEFER_CHECK,
swarm_engine_hint_defer_check): the check
workgroups share the launch of the reward, the build sort, the vision grid
and the pair search, which run ahead of the per-env verdict where the check
changes nothing they read, and wait for it or redo their work where it does.
Where the check runs may not change a bit: every case builds the same engine with the switch
on and off and compares everything the slices produce, and requires from
swarm_engine_check_stats that the switch-on engine's checks did ride (or,
for the flush paths, did not).

Small shapes: 1024 colloids (one pair-search block per env) and 1500 (a
ragged second block), one and two envs (every per-env word indexed by env).
"""

import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_EPISODE = 4
# Translate force whose agents outrun the candidate lists (1.5 um a window)
UNUSABLE_FORCE = 100.0


def _host(traj):
    return {k: [torch.as_tensor(x).detach().cpu().numpy().copy() for x in getattr(traj, k)]
            for k in ("features", "actions", "rewards", "log_probs")}


def _stats(native, name):
    out = (ctypes.c_uint64 * 4)()
    native.call(name, out, 0)
    return list(out)


def _ring(eng):
    eng.drain_trajectory(block=True)
    h = eng.traj_holder
    return {k: np.asarray(v).copy() for k, v in h.items()} if h else {}


def _run_workload(switch, N, E, force, monkeypatch, eager_slices=3):
    """The headline's workload at a small size: one eager slice, an eager
    integrate of several slices (its inner slices defer), then the captured
    episode of T_EPISODE slices replayed twice."""
    sys.path.insert(0, ROOT)
    import bench
    from swarmrl_amd.actions import Action

    monkeypatch.setenv("SWARMRL_AMD_DEFER_CHECK", switch)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ns = argparse.Namespace(colloids=N, envs_per_gpu=E, write_interval=1.0)
    eng, ff, agent = bench.build_workload(ns, 42, dev)
    agent.actions["Translate"] = Action(force=force)
    agent._tables = None
    pos0 = np.stack(eng._pos[0]) if E == 1 else None
    dir0 = np.stack(eng._dir[0]) if E == 1 else None
    eng.integrate(1, ff)
    eng.integrate(eager_slices, ff)
    torch.cuda.synchronize()
    blocks = [_host(agent.trajectory)]
    agent.reset_trajectory()
    _, episode_graph, warm = bench.capture_episode(eng, ff, agent, T_EPISODE)
    blocks.append(_host(warm))
    for _ in range(2):
        episode_graph.replay()
        torch.cuda.synchronize()
        blocks.append(_host(agent.trajectory))
    out = {
        "blocks": blocks,
        "ring": _ring(eng),
        "state": eng.get_raw_state(),
        "build_stats": _stats(eng._native, "swarm_engine_build_stats"),
        "check_stats": _stats(eng._native, "swarm_engine_check_stats"),
        "pos0": pos0, "dir0": dir0, "eng": eng, "agent": agent,
    }
    del episode_graph
    return out


def _same(on, off):
    assert len(on["blocks"]) == len(off["blocks"])
    for b, (x, y) in enumerate(zip(on["blocks"], off["blocks"])):
        for k in ("features", "actions", "log_probs", "rewards"):
            assert len(x[k]) == len(y[k]), (b, k)
            for s, (u, v) in enumerate(zip(x[k], y[k])):
                assert np.array_equal(u, v), (b, k, s)
    for k in ("q", "img", "ang"):
        assert np.array_equal(on["state"][k], off["state"][k]), k
    assert on["ring"].keys() == off["ring"].keys()
    for k in on["ring"]:
        assert np.array_equal(on["ring"][k], off["ring"][k]), ("ring", k)
    assert on["build_stats"] == off["build_stats"], (on["build_stats"], off["build_stats"])
    assert sum(off["check_stats"]) == 0, off["check_stats"]


def _rode(E, eager_slices=3):
    # every slice of a multi-slice integrate but its last defers its check:
    # the eager integrate, the captured episode's capture and its two replays
    # (captured launches do not run while they are captured)
    return E * ((eager_slices - 1) + 2 * (T_EPISODE - 1))


@pytest.mark.parametrize("N,E", [(1024, 1), (1500, 1), (1024, 2), (1500, 2)])
def test_bench_swim_force_rides_and_is_bit_identical(N, E, monkeypatch):
    on = _run_workload("1", N, E, 10.0, monkeypatch)
    off = _run_workload("0", N, E, 10.0, monkeypatch)
    _same(on, off)
    print("check_stats", on["check_stats"], "build_stats", on["build_stats"])
    assert sum(on["check_stats"]) == _rode(E), on["check_stats"]
    # speculated: all but, perhaps, each env's first riding window (as
    # tests/test_gpu_l1_pairs.py allows for the lists)
    assert on["check_stats"][0] >= _rode(E) - E, on["check_stats"]
    filtered, waited, reruns, windows = on["build_stats"]
    assert filtered + waited == windows and waited <= E, on["build_stats"]


def test_bench_swim_force_matches_oracle(monkeypatch):
    """The switch-on engine against the oracle's replay of the recorded
    actions (as tests/test_gpu_l1_pairs.py), 1500 colloids."""
    N = 1500
    on = _run_workload("1", N, 1, 10.0, monkeypatch)
    eng, agent = on["eng"], on["agent"]
    L = float(eng._box[0])
    box = np.array([L, L, L])
    src = np.array([L / 2, L / 2, 0.0])
    p = oracle.make_params(eng._box, eng._time_step, eng._kT(),
                           eng.params.WCA_epsilon.m_as("sim_energy"), 42, [eng._species_keys[0]])
    agents = np.arange(N)
    radii = np.ones(N, np.float32)
    types = np.zeros(N, np.int32)
    ftab = np.array([0.0, 10.0, 0.0, 0.0], np.float32)
    ttab = np.array([10.0, 0.0, -10.0, 0.0], np.float32)
    sp = np.zeros(N, np.uint8)
    st = oracle.state_from_positions(on["pos0"], on["dir0"], eng._box)
    hist = oracle.history_from_state(st, agents)
    st, _ = oracle.sd_run(p, st, sp, 1000)
    prev = {"f": np.zeros(N, np.float32), "t": np.zeros(N, np.float32), "ang": st["ang"].copy()}
    f32 = np.float32
    step = 0
    for block in on["blocks"]:
        for s in range(len(block["actions"])):
            obs = oracle.vision_cone(p, st, agents, radii, types, 10.0, np.pi / 2, 3, [0],
                                     cells=True)
            assert np.array_equal(block["features"][s].reshape(obs.shape), obs), (step, "cone")
            idx = block["actions"][s].reshape(-1)
            f, t = ftab[idx], ttab[idx]
            st, _, _ = oracle.bd_run(p, st, sp, f, t, 100, step0=100 * step, prev=prev)
            prev = {"f": f, "t": t, "ang": st["ang"].copy()}
            dc, dp = oracle.field_distance(p, st, agents, src, box, hist, update=True)
            v = (f32(10.0) * ((f32(1.0) - dc) - (f32(1.0) - dp))).astype(np.float32)
            rew = np.where(v < 0, f32(0), v).astype(np.float32)
            assert np.array_equal(block["rewards"][s].reshape(-1), rew), (step, "reward")
            step += 1
    assert step == 1 + 3 + 2 + 2 * T_EPISODE
    for k in ("q", "img", "ang"):
        assert np.array_equal(on["state"][k], st[k]), k
    assert sum(on["check_stats"]) == _rode(1), on["check_stats"]
    assert on["check_stats"][0] >= _rode(1) - 1, on["check_stats"]


@pytest.mark.parametrize("N,E", [(1024, 1), (1500, 2)])
def test_unusable_lists_take_the_miss_path(N, E, monkeypatch):
    """Translate force 100: translating agents outrun the candidate lists, so
    the pair search of windows whose check rode along waits for the launch's
    own sort (tagged with the env's window number) and searches its cells.
    No window's speculation stands: each lands in "lists unusable" or, where
    the exact test failed as well, in "redone after a re-run"."""
    on = _run_workload("1", N, E, UNUSABLE_FORCE, monkeypatch)
    off = _run_workload("0", N, E, UNUSABLE_FORCE, monkeypatch)
    _same(on, off)
    print("check_stats", on["check_stats"], "build_stats", on["build_stats"])
    cs = on["check_stats"]
    assert sum(cs) == _rode(E) and cs[0] == 0 and cs[1] == 0, cs
    assert on["build_stats"][1] > E, on["build_stats"]  # pair searches that waited for the sort


def test_unusable_lists_without_a_rerun(monkeypatch):
    """Translate force 40: some windows pass the exact test although an agent
    moved further than the lists allow -- "lists unusable" proper, beside
    windows that stand and windows that re-run."""
    N, E = 1500, 2
    on = _run_workload("1", N, E, 40.0, monkeypatch)
    off = _run_workload("0", N, E, 40.0, monkeypatch)
    _same(on, off)
    print("check_stats", on["check_stats"], "build_stats", on["build_stats"])
    cs = on["check_stats"]
    assert sum(cs) == _rode(E) and cs[1] == 0, cs
    assert cs[2] > 0, cs


# ----------------------------------------------------------- C-ABI sequences
def _field(h, agents, hq, himg, dcur, dprev, box):
    src = (ctypes.c_double * 3)(box[0] / 2, box[1] / 2, 0.0)
    bs = (ctypes.c_double * 3)(*box)
    h.native.call("swarm_field_distance", ctypes.c_void_p(agents.data_ptr()), agents.numel(), src,
                  bs, ctypes.c_void_p(hq.data_ptr()), ctypes.c_void_p(himg.data_ptr()),
                  ctypes.c_void_p(dcur.data_ptr()), ctypes.c_void_p(dprev.data_ptr()), 1, 0)


class _Seq:
    """set_actions -> [hint] integrate -> defer_build -> reward, as
    SwarmEngine's slice does, straight on the C ABI."""

    def __init__(self, switch, box, states, seed, monkeypatch):
        from gpu_harness import Harness, species_list

        monkeypatch.setenv("SWARMRL_AMD_DEFER_CHECK", switch)
        # the cluster windows at any density (a dense box would take the
        # neighbour-list windows, whose check never rides)
        monkeypatch.setenv("SWARMRL_AMD_NLIST", "0")
        torch.cuda.set_device(0)
        self.dev = torch.device("cuda", 0)
        self.box = box
        self.E, self.n = len(states), len(states[0]["ang"])
        self.h = Harness(box, 1e-3, 1.0239, 1.0239, seed, species_list()[:1],
                         np.zeros(self.n, int), n_envs=self.E)
        self.h.upload(states)
        A = self.E * self.n
        self.agents = torch.arange(self.n, dtype=torch.int32, device=self.dev)
        self.hq = torch.zeros((3, A), dtype=torch.int32, device=self.dev)
        self.himg = torch.zeros((3, A), dtype=torch.int32, device=self.dev)
        self.dcur = torch.zeros(A, dtype=torch.float32, device=self.dev)
        self.dprev = torch.zeros(A, dtype=torch.float32, device=self.dev)
        self.rewards = []

    def window(self, nsteps, hint=True, reward=True):
        h = self.h
        h.native.bind_stream()
        if hint:
            h.native.call("swarm_engine_hint_defer_check")
        h.native.call("swarm_engine_integrate", int(nsteps))
        if reward:
            deferred = ctypes.c_int32()
            h.native.call("swarm_engine_defer_build", ctypes.byref(deferred))
            assert deferred.value == 1
            _field(h, self.agents, self.hq, self.himg, self.dcur, self.dprev, self.box)
            torch.cuda.synchronize()
            self.rewards.append((self.dcur.cpu().numpy().copy(), self.dprev.cpu().numpy().copy(),
                                 self.hq.cpu().numpy().copy(), self.himg.cpu().numpy().copy()))

    def result(self):
        return {"state": self.h.download(), "rewards": self.rewards,
                "build_stats": _stats(self.h.native, "swarm_engine_build_stats"),
                "check_stats": _stats(self.h.native, "swarm_engine_check_stats")}


def _same_seq(on, off):
    for e, (a, b) in enumerate(zip(on["state"], off["state"])):
        for k in ("q", "img", "ang"):
            assert np.array_equal(a[k], b[k]), (e, k)
    assert len(on["rewards"]) == len(off["rewards"])
    for w, (a, b) in enumerate(zip(on["rewards"], off["rewards"])):
        for u, v in zip(a, b):
            assert np.array_equal(u, v), w
    assert on["build_stats"] == off["build_stats"], (on["build_stats"], off["build_stats"])
    assert sum(off["check_stats"]) == 0


def _cross_skin_states(E):
    from gpu_harness import random_state, species_list

    rng = np.random.default_rng(9)
    # (sparser than tests/test_gpu_parity.py's 150 um box, whose random state
    # holds clusters wider than a wave: those windows wait, they are the next
    # test's)
    box = [300.0, 300.0, 300.0]
    n = 1500
    sp = np.zeros(n, int)
    op = oracle.make_params(box, 1e-3, 1.0239, 1.0239, 11, species_list()[:1])
    states = [random_state(rng, n, box) for _ in range(E)]
    states = [oracle.sd_run(op, s, sp, 300)[0] for s in states]
    t = rng.normal(size=E * n).astype(np.float32) * 5
    return box, states, t


def test_swimmers_that_cross_the_skin_rerun_inside_the_reward_launch(monkeypatch):
    """Force 400 (tests/test_gpu_parity.py::test_fast_swimmers_cross_skin_bit_exact):
    the window fails the exact test, so the check workgroup restores the
    window start and re-runs the env on the global path once the other roles
    of the launch have arrived, and they redo their work; two windows, two
    envs, against the oracle as well."""
    E = 2
    box, states, t = _cross_skin_states(E)
    n = len(states[0]["ang"])
    f = np.full(E * n, 400.0, np.float32)
    res = {}
    for switch in ("0", "1"):
        s = _Seq(switch, box, states, 11, monkeypatch)
        s.h.set_actions(f, t)
        for _ in range(2):
            s.window(100)
        res[switch] = s.result()
        op = s.h.op
    off, on = res["0"], res["1"]
    # the chosen seed does re-run within these windows (switch off: k_check)
    assert off["build_stats"][2] >= 1, off["build_stats"]
    _same_seq(on, off)
    print("check_stats", on["check_stats"], "build_stats", on["build_stats"])
    assert sum(on["check_stats"]) == 2 * E, on["check_stats"]
    assert on["check_stats"][3] >= 1, on["check_stats"]  # redone after a re-run
    sp = np.zeros(n, int)
    for e in range(E):
        ref = states[e]
        for k in range(2):
            ref, _, _ = oracle.bd_run(op, ref, sp, f[e * n:(e + 1) * n], t[e * n:(e + 1) * n], 100,
                                      step0=100 * k, env=e)
        for k in ("q", "img", "ang"):
            assert np.array_equal(on["state"][e][k], ref[k]), (e, k)


def _patch_state():
    rng = np.random.default_rng(21)
    box = [200.0, 200.0, 200.0]
    pts = []
    for cx, cy in ((40.0, 40.0), (120.0, 60.0), (80.0, 150.0)):
        for gx in range(10):
            for gy in range(10):
                pts.append((cx + 2.5 * gx, cy + 2.5 * gy))
    while len(pts) < 1000:
        p = rng.random(2) * 200.0
        if min((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 for q in pts) > 16.0:
            pts.append((p[0], p[1]))
    n = len(pts)
    pos = np.zeros((n, 3))
    pos[:, :2] = pts
    a = 2 * np.pi * rng.random(n)
    dirs = np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)
    return rng, box, oracle.state_from_positions(pos, dirs, box)


def test_big_clusters_run_in_the_check_workgroup_of_the_reward_launch(monkeypatch):
    """Patches wider than a wave (tests/test_gpu_parity.py::
    test_big_clusters_run_in_check_bit_exact): the check workgroup integrates
    them before its test, so the other roles, which ran ahead, do their work
    again after its verdict ("big clusters" in check_stats); bit-exact against
    the oracle, no global-path re-run."""
    rng, box, st0 = _patch_state()
    n = len(st0["ang"])
    acts = [(rng.choice([0.0, 5.0], n).astype(np.float32),
             rng.choice([-5.0, 0.0, 5.0], n).astype(np.float32)) for _ in range(2)]
    res = {}
    for switch in ("0", "1"):
        s = _Seq(switch, box, [st0], 5, monkeypatch)
        for (f, t), nsteps in zip(acts, (100, 60)):
            s.h.set_actions(f, t)
            s.window(nsteps)
        res[switch] = s.result()
        op = s.h.op
    off, on = res["0"], res["1"]
    _same_seq(on, off)
    print("check_stats", on["check_stats"], "build_stats", on["build_stats"])
    assert on["check_stats"][1] == 2 and sum(on["check_stats"]) == 2, on["check_stats"]
    assert on["build_stats"][2] == 0, on["build_stats"]
    st, step = st0, 0
    for (f, t), nsteps in zip(acts, (100, 60)):
        st, _, _ = oracle.bd_run(op, st, np.zeros(n), f, t, nsteps, step0=step)
        step += nsteps
    for k in ("q", "img", "ang"):
        assert np.array_equal(on["state"][0][k], st[k]), k


def test_anything_but_the_reward_flushes_a_pending_check(monkeypatch):
    """After the hint, a state download, set_actions and a second integrate
    each find the check pending and enqueue it as a launch of its own."""
    E = 2
    box, states, t = _cross_skin_states(E)
    n = len(states[0]["ang"])
    f = np.full(E * n, 40.0, np.float32)
    res = {}
    for switch in ("0", "1"):
        s = _Seq(switch, box, states, 11, monkeypatch)
        s.h.set_actions(f, t)
        mid = []
        s.window(100, reward=False)
        mid.append(s.h.download())      # a download
        s.window(100, reward=False)
        s.h.set_actions(f, -t)          # set_actions
        s.window(100, reward=False)
        s.window(100, hint=False, reward=False)  # a second integrate
        r = s.result()
        r["mid"] = mid
        res[switch] = r
    off, on = res["0"], res["1"]
    _same_seq(on, off)
    for e in range(E):
        for k in ("q", "img", "ang"):
            assert np.array_equal(on["mid"][0][e][k], off["mid"][0][e][k]), (e, k)
    assert on["build_stats"][3] == 4 * E, on["build_stats"]  # every window was checked
    assert sum(on["check_stats"]) == 0, on["check_stats"]


def test_a_captured_run_alone_keeps_its_check(monkeypatch):
    """SwarmEngine._run captured on its own (no reward follows, so no hint):
    the graph holds the check: three replays equal three eager windows of the
    switch-off engine."""
    sys.path.insert(0, ROOT)
    import bench

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ns = argparse.Namespace(colloids=1024, envs_per_gpu=2, write_interval=1.0)
    got = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("SWARMRL_AMD_DEFER_CHECK", switch)
        eng, ff, agent = bench.build_workload(ns, 42, dev)
        eng.integrate(1, ff)
        torch.cuda.synchronize()
        if switch == "1":
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                eng._run(100)
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            del g
        else:
            for _ in range(3):
                eng._run(100)
        got[switch] = (eng.get_raw_state(), _stats(eng._native, "swarm_engine_build_stats"),
                       _stats(eng._native, "swarm_engine_check_stats"))
    for k in ("q", "img", "ang"):
        assert np.array_equal(got["1"][0][k], got["0"][0][k]), k
    assert got["1"][1][3] == got["0"][1][3], (got["1"][1], got["0"][1])  # windows checked
    assert sum(got["1"][2]) == 0, got["1"][2]


# ------------------------------------------- above 4096 colloids per env
def _lattice_state(seed, k=65, a=5.0):
    """k x k colloids (4225: the one-workgroup sorts take 16 colloids per
    thread above 4096) on a square lattice of spacing a, jittered by 1 um: no
    overlaps, no cluster wider than a wave."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2)
    pos = np.zeros((k * k, 3))
    pos[:, :2] = (g + 0.5) * a + rng.uniform(-1.0, 1.0, (k * k, 2))
    th = 2 * np.pi * rng.random(k * k)
    box = [k * a, k * a, k * a]
    dirs = np.stack([np.cos(th), np.sin(th), np.zeros(k * k)], 1)
    return rng, box, oracle.state_from_positions(pos, dirs, box)


def _actions(rng, n):
    return (rng.choice([0.0, 10.0], n).astype(np.float32),
            rng.choice([-10.0, 0.0, 10.0], n).astype(np.float32))


@pytest.mark.parametrize("switch", ["0", "1"])
def test_reward_launch_above_4096_colloids_matches_oracle(switch, monkeypatch):
    """One env of 4225 colloids with the plain pair search (SWARMRL_AMD_LOCAL_UF=0,
    so the slice's launches carry the build and the pair search): the reward
    launch carries the 16-per-thread build sort and, with the switch on, the
    window's check (k_field_vgrid_sort<16, kCheck>).  Two windows of 5
    sub-steps; states, rewards and the field history bit-exact against the
    oracle."""
    rng, box, st0 = _lattice_state(31)
    n = len(st0["ang"])
    monkeypatch.setenv("SWARMRL_AMD_LOCAL_UF", "0")
    s = _Seq(switch, box, [st0], 13, monkeypatch)
    acts = [_actions(rng, n) for _ in range(2)]
    for f, t in acts:
        s.h.set_actions(f, t)
        s.window(5)
    got = s.result()
    print("check_stats", got["check_stats"], "build_stats", got["build_stats"])
    assert sum(got["check_stats"]) == (2 if switch == "1" else 0), got["check_stats"]
    agents = np.arange(n)
    src = np.array([box[0] / 2, box[1] / 2, 0.0])
    hist = {"q": np.zeros((3, n), np.uint32), "img": np.zeros((3, n), np.int32)}
    st = st0
    for w, (f, t) in enumerate(acts):
        st, _, _ = oracle.bd_run(s.h.op, st, np.zeros(n), f, t, 5, step0=5 * w)
        dc, dp = oracle.field_distance(s.h.op, st, agents, src, np.array(box), hist, update=True)
        dcur, dprev, hq, himg = got["rewards"][w]
        assert np.array_equal(dcur, dc) and np.array_equal(dprev, dp), w
        assert np.array_equal(hq.view(np.uint32), hist["q"]), w
        assert np.array_equal(himg, hist["img"]), w
    assert not np.array_equal(got["rewards"][1][0], got["rewards"][1][1])  # the colloids moved
    for k in ("q", "img", "ang"):
        assert np.array_equal(got["state"][0][k], st[k]), k


@pytest.mark.parametrize("k,local_uf", [(65, "0"), (65, "1"), (6, "0")])
def test_deferred_build_carried_by_the_cone_or_flushed_matches_oracle(k, local_uf, monkeypatch):
    """The deferred build carried by the vision cone and with no carrier at
    all (its three stages flushed before the window: k_build_sort<CH>,
    k_build_pairs<kLocal>, k_cluster_build<false, kLocal>); cone and states
    bit-exact against the oracle.  4225 colloids (k = 65): k_vgrid_sort<16>,
    then with the block-local pair search k_vision_pairs<.., true>, with the
    plain one the pair search beside the sort.  36 colloids in a 30 um box
    (k = 6: four build cells a side, too few for the candidate lists):
    k_vgrid_sort<4>, then k_vision_pairs<.., false>."""
    from gpu_harness import Harness, species_list
    from swarmrl_amd.engine import ops

    rng, box, st = _lattice_state(32, k=k)
    n = len(st["ang"])
    monkeypatch.setenv("SWARMRL_AMD_LOCAL_UF", local_uf)
    monkeypatch.setenv("SWARMRL_AMD_NLIST", "0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    h = Harness(box, 1e-3, 1.0239, 1.0239, 14, species_list()[:1], np.zeros(n, int))
    h.upload([st])
    agents = np.arange(0, n, 4, dtype=np.int32)
    radii = np.ones(n, np.float32)
    types = np.zeros(n, np.int32)
    t_agents = torch.as_tensor(agents, device=dev)
    t_radii = torch.as_tensor(radii, device=dev)
    t_types = torch.as_tensor(types, device=dev)
    vp = ops.vision_params(10.0, np.pi / 2, 3, [0])

    def defer():
        deferred = ctypes.c_int32()
        h.native.bind_stream()
        h.native.call("swarm_engine_defer_build", ctypes.byref(deferred))
        assert deferred.value == 1

    step = 0
    for carrier in (True, False, True):
        f, t = _actions(rng, n)
        h.set_actions(f, t)
        h.integrate(5)
        st, _, _ = oracle.bd_run(h.op, st, np.zeros(n), f, t, 5, step0=step)
        step += 5
        defer()
        if carrier:
            out = ops.vision_cone(h.native, 1, t_agents, t_radii, t_types, vp).cpu().numpy()
            ref = oracle.vision_cone(h.op, st, agents, radii, types, 10.0, np.pi / 2, 3, [0],
                                     cells=True)
            assert np.array_equal(out[0], ref)
            assert np.count_nonzero(ref) > len(agents)
    f, t = _actions(rng, n)
    h.set_actions(f, t)
    h.integrate(5)
    st, _, _ = oracle.bd_run(h.op, st, np.zeros(n), f, t, 5, step0=step)
    got = h.download()[0]
    for key in ("q", "img", "ang"):
        assert np.array_equal(got[key], st[key]), key
    fb, waves = h.window_stats()
    assert fb[0] == 0 and waves[0] > 0, (fb, waves)
    # what the host can see of the carrier: with the candidate lists (4225
    # colloids, plain pair search) the pair search of both carried builds ran
    # as a role of the cone's grid launch and counted itself
    filtered, waited, _, _ = _stats(h.native, "swarm_engine_build_stats")
    print("build_stats", filtered, waited)
    if k == 65 and local_uf == "0":
        assert filtered + waited >= 2, (filtered, waited)
