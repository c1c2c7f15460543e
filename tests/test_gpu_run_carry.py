"""
The latency schedule's run wave (k_cluster_run_wide) carries the image
counters once per window (window_carry in swarm_integrator.cuh) and sends the
pair's second end through ds_sub_u64, also in the speculation's fix-up pass.
Bit for bit against the CPU oracle, which carries per sub-step:

  * box-edge crossings the run wave makes itself, in both directions on both
    axes, with colloids that hop back and forth across an edge inside one
    window, and no window re-run (the images compared are the run wave's);
  * the guard: colloids that move a quarter of the box or more from the
    window start (in one window, or in one sub-step) send their env, and only
    theirs, to the exact re-run -- also where nothing else would (a lone
    mover with no other colloid in reach of its start);
  * pair forces beyond the int32 speculation (the fix-up pass);
  * on the CPU alone, the carry identity and its guard restated in numpy.

Shapes: E = 2 envs of N = 192 colloids of radius 0.05 um (so that 192 of them
form many small clusters in a 60 um box: the cluster link length is
2 r + skin), windows of 100 sub-steps, noise on, both settings of the
rotation helper.
"""

import pathlib
import re

import numpy as np
import pytest

from oracle import oracle

ROOT = pathlib.Path(__file__).resolve().parents[1]

E, N, WINDOW = 2, 192, 100
DT = 1e-3
GAMMA_T = 4.6595
SPECIES = [(0.05, GAMMA_T, 6.2126, 1.0358e-6, 4.143e-7)]
RC = 2.0 ** (1.0 / 6.0) * 0.1  # the WCA cutoff of two such colloids
HELPER = pytest.mark.parametrize("helper", ["1", "0"])


def _skin():
    """The engine's Verlet skin (um), from its planning header."""
    m = re.search(r"constexpr double kSkinUm = ([0-9.]+);",
                  (ROOT / "swarmrl_amd" / "csrc" / "swarm_plan.h").read_text())
    return float(m.group(1))


def _force_for(drift):
    """The constant force that moves a colloid by `drift` um per window."""
    return drift * GAMMA_T / (WINDOW * DT)


def _dirs(rng, n):
    th = 2 * np.pi * rng.random(n)
    return np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1)


def _fe(f_ext, e):
    return np.ascontiguousarray(f_ext[e].T).astype(np.float32)


# ------------------------------------------------------------ the edge case
# 60 um, not 40: with every colloid on the two edge lines, the groups they
# form must stay farther apart than the cluster link (2 r + skin = 2.1 um) and
# the env's pairs within it below the build's capacity (3 N); 40 groups of
# four or five fit 120 um of edge line, not 80
EDGE_L = 60.0
EDGE_DRIFT = 0.6  # um per window, < skin / 2 with the Brownian part (checked)
EDGE_KT = 0.02
EDGE_EPS = 0.02  # (soft enough that a 0.1 um contact is stable at this time step)
EDGE_SEED = 1503


def _edge_env(rng):
    """192 colloids in 40 groups on the box's two edge lines, 2.9 um apart.
    A group of line a (the edge coordinate a = 0) is a column of two or three
    colloids just above the edge (coordinate in (0, 0.4)), pushed down across
    it, and 0.15 um along the line a column just below it (in (L - 0.4, L)),
    pushed up: 48 colloids per side and line, every one within one window's
    drift of its edge.  A column of three has its deeper two 0.105 um apart: in
    contact (r_c = 0.112).  One colloid on each side of each line (four per
    env) instead starts within 0.02 um of the edge and feels no force.
    Returns positions, forces [N][3] and the indices of the force-free ones."""
    L = EDGE_L
    f0 = _force_for(EDGE_DRIFT)
    pos = np.zeros((N, 3))
    f = np.zeros((N, 3))
    still = []
    i = 0
    for a in (0, 1):
        for k in range(20):
            t = 2.0 + 2.9 * k
            # 16 groups of five (the third member on alternating sides), 4 of four
            n_up = 2 if k >= 16 else 3 - k % 2
            n_down = 2 if k >= 16 else 2 + k % 2
            for side, cnt in ((+1, n_up), (-1, n_down)):
                for depth in ((0.06, 0.27, 0.375) if cnt == 3 else (0.06, 0.38)):
                    d = depth + rng.uniform(-0.005, 0.005) * (depth < 0.1)
                    free = depth < 0.1 and k == (5 if side > 0 else 12)
                    if free:
                        d = rng.uniform(0.002, 0.018)
                        still.append(i)
                    pos[i, a] = d if side > 0 else L - d
                    pos[i, 1 - a] = t + (0.0 if side > 0 else 0.15) + rng.uniform(-0.002, 0.002)
                    if not free:
                        f[i, a] = -side * f0 * rng.uniform(0.95, 1.05)
                        f[i, 1 - a] = f0 * rng.uniform(-0.05, 0.05)
                    i += 1
    assert i == N and len(still) == 4
    return pos, f, np.array(still)


def _edge_case():
    rng = np.random.default_rng(EDGE_SEED)
    box = [EDGE_L] * 3
    envs = [_edge_env(rng) for _ in range(E)]
    states = [oracle.state_from_positions(p, _dirs(rng, N), box) for p, _, _ in envs]
    f_ext = np.stack([f for _, f, _ in envs])
    still = [s for _, _, s in envs]
    acts = [(rng.uniform(0.0, 1.0, E * N).astype(np.float32),
             (rng.normal(size=E * N) * 5).astype(np.float32)) for _ in range(3)]
    return box, states, f_ext, still, acts


def _edge_oracle(op, states, f_ext, still, acts):
    """The oracle's three windows per env, and what makes the case a test of
    the carry: the images' changes per window, each window's largest
    displacement, and the edge hops of the force-free colloids sub-step by
    sub-step."""
    sp = np.zeros(N, np.uint8)
    out, stats = [], []
    for e in range(E):
        st = states[e]
        s = slice(e * N, (e + 1) * N)
        hops = np.zeros(len(still[e]), int)
        dmax = 0.0
        for w, (f, t) in enumerate(acts):
            x0 = oracle.unwrapped(st, [EDGE_L] * 3)
            one = st
            for k in range(WINDOW):
                nxt, _, _ = oracle.bd_run(op, one, sp, f[s], t[s], 1, step0=w * WINDOW + k, env=e,
                                          f_ext=_fe(f_ext, e))
                hops += np.any(nxt["img"][:2, still[e]] != one["img"][:2, still[e]], axis=0)
                dmax = max(dmax, np.abs(oracle.unwrapped(nxt, [EDGE_L] * 3) - x0).max())
                one = nxt
            st, _, _ = oracle.bd_run(op, st, sp, f[s], t[s], WINDOW, step0=w * WINDOW, env=e,
                                     f_ext=_fe(f_ext, e))
            for key in ("q", "img", "ang"):  # (sub-step by sub-step is the same run)
                assert np.array_equal(st[key], one[key])
        dimg = st["img"][:2].astype(int) - states[e]["img"][:2].astype(int)
        out.append(st)
        stats.append({"dimg": dimg, "hops": hops, "dmax": dmax})
    return out, stats


def _edge_conditions(stats):
    for s in stats:
        up = [(s["dimg"][a] == 1).sum() for a in (0, 1)]
        down = [(s["dimg"][a] == -1).sum() for a in (0, 1)]
        print("edge case: +1", up, "-1", down, "hops", s["hops"], "dmax", s["dmax"])
        assert min(up) > 0 and min(down) > 0
        assert sum(up) + sum(down) >= N // 8
        assert np.abs(s["dimg"]).max() == 1
        # back and forth inside a window: three or more changes in 300 sub-steps
        assert (s["hops"] >= 3).sum() >= 2
        assert s["dmax"] < 0.5 * _skin()


def test_edge_case_conditions_hold_for_the_oracle(oracle_mod):
    """CPU: the seed's oracle run alone crosses every edge both ways, hops
    across it, and keeps every window's displacement below half the skin."""
    box, states, f_ext, still, acts = _edge_case()
    op = oracle.make_params(box, DT, EDGE_KT, EDGE_EPS, 42, SPECIES)
    _, stats = _edge_oracle(op, states, f_ext, still, acts)
    _edge_conditions(stats)


@pytest.fixture(scope="module")
def gpu():
    import torch

    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _compare(h, ref, what):
    got = h.download()
    for e in range(E):
        for key in ("q", "img", "ang"):
            assert np.array_equal(got[e][key], ref[e][key]), (what, e, key)


@pytest.mark.gpu
@HELPER
def test_run_wave_edge_crossings_bit_exact(gpu, helper, monkeypatch):
    from gpu_harness import Harness

    monkeypatch.setenv("SWARMRL_AMD_ROT_HELPER", helper)
    box, states, f_ext, still, acts = _edge_case()
    h = Harness(box, DT, EDGE_KT, EDGE_EPS, 42, SPECIES, np.zeros(N, int), n_envs=E)
    h.upload(states)
    h.set_external_force(f_ext)
    sp = np.zeros(N, np.uint8)
    ref = list(states)
    passes = set()
    for w, (f, t) in enumerate(acts):
        h.set_actions(f, t)
        h.integrate(WINDOW)
        for e in range(E):
            s = slice(e * N, (e + 1) * N)
            ref[e], _, _ = oracle.bd_run(h.op, ref[e], sp, f[s], t[s], WINDOW, step0=w * WINDOW,
                                         env=e, f_ext=_fe(f_ext, e))
        _compare(h, ref, ("window", w))
        fb, waves = h.window_stats()
        print("edge crossings helper", helper, "window", w, "fallback", fb, "waves", waves)
        assert np.all(fb == 0) and np.all(waves > 1), (fb, waves)
        passes.update(waves.tolist())
    _, stats = _edge_oracle(h.op, states, f_ext, still, acts)
    _edge_conditions(stats)


# ---------------------------------------------------------------- the guard
def _site_env(rng, L, k=8):
    """k x k sites on a square lattice, three colloids 0.2 um apart at each:
    clusters of three, the sites farther apart than the cluster link."""
    a = L / k
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2)
    tri = 0.2 / np.sqrt(3.0) * np.array([[np.cos(u), np.sin(u)]
                                         for u in (0.5, 0.5 + 2 * np.pi / 3, 0.5 + 4 * np.pi / 3)])
    pos = np.zeros((3 * k * k, 3))
    pos[:, :2] = ((g + 0.5) * a)[:, None, :].repeat(3, 1).reshape(-1, 2) + np.tile(tri, (k * k, 1))
    pos[:, :2] += rng.uniform(-0.01, 0.01, (3 * k * k, 2))
    return pos


GUARD_L = 20.0


def _guard_case(kind):
    """Env 1: the sites, no force.  Env 0, "crowd": four colloids taken to
    the lanes between the sites' rows and driven along them, three by 5.5, 6.5
    and 8 um per window, one by 7 um per sub-step (between a quarter and half
    a box).  Their env would re-run without the guard too: a mover that far
    fails the check's test against its non-neighbours.  Env 0, "lone": two
    colloids 0.5 um apart (a listed pair, so their wave runs pair passes)
    driven 5.5 um per window from the centre of a disc of 6.5 um that holds
    nothing else, every other colloid at rest, so the check's test passes (no
    non-neighbour within r_c + 5.5 um + the others' motion of their start)
    and the guard alone sends the env to the re-run."""
    rng = np.random.default_rng(1502)
    L = GUARD_L
    f_ext = np.zeros((E, N, 3))
    if kind == "crowd":
        pos0 = _site_env(rng, L)
        who = [0, 40, 80, 120]
        pos0[who, :2] = [[1.0, 2.5], [5.0, 18.0], [10.0, 3.0], [19.0, 12.5]]
        f_ext[0, 0, 0] = _force_for(5.5)
        f_ext[0, 40, 1] = -_force_for(6.5)
        f_ext[0, 80, 1] = _force_for(8.0)
        f_ext[0, 120, 0] = -_force_for(7.0 * WINDOW)
    else:
        g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2)
        sites = (g + 0.5) * (L / 8)
        sites = sites[np.hypot(*(sites - 0.5 * L).T) > 6.5]
        pos0 = np.zeros((N, 3))
        pos0[:2, :2] = [[0.5 * L, 0.5 * L - 0.25], [0.5 * L, 0.5 * L + 0.25]]
        for i in range(2, N):  # the others on rings of 0.15 um around the sites left
            k, m = (i - 2) % len(sites), (i - 2) // len(sites)
            u = 2 * np.pi * m / 5 + 0.3
            pos0[i, :2] = sites[k] + 0.15 * np.array([np.cos(u), np.sin(u)])
        assert (N - 2 + len(sites) - 1) // len(sites) <= 5
        who = [0, 1]
        f_ext[0, :2, 0] = _force_for(5.5)
    box = [L] * 3
    states = [oracle.state_from_positions(pos0, _dirs(rng, N), box),
              oracle.state_from_positions(_site_env(rng, L), _dirs(rng, N), box)]
    acts = [(rng.uniform(0.0, 1.0, E * N).astype(np.float32),
             (rng.normal(size=E * N) * 5).astype(np.float32)) for _ in range(2)]
    return box, states, f_ext, who, acts


def _guard_oracle(op, kind, box, states, f_ext, who, acts):
    """Both envs' two windows, and that the oracle's driven colloids end every
    window a quarter of the box or more from where they began it (the one
    driven per sub-step: its first sub-step between a quarter and a half)."""
    sp = np.zeros(N, np.uint8)
    ref = [[], []]
    for e in range(E):
        st = states[e]
        s = slice(e * N, (e + 1) * N)
        for w, (f, t) in enumerate(acts):
            kw = dict(step0=w * WINDOW, env=e, f_ext=_fe(f_ext, e))
            nxt, _, _ = oracle.bd_run(op, st, sp, f[s], t[s], WINDOW, **kw)
            if e == 0:
                far = np.abs(oracle.unwrapped(nxt, box) - oracle.unwrapped(st, box))[who].max(1)
                print("guard case", kind, "window", w, "driven colloids moved", far)
                assert np.all(far[:3] >= 0.25 * GUARD_L)
                if kind == "crowd":
                    one, _, _ = oracle.bd_run(op, st, sp, f[s], t[s], 1, **kw)
                    hop = np.abs(oracle.unwrapped(one, box) - oracle.unwrapped(st, box))[who[3]]
                    assert 0.25 * GUARD_L < hop.max() < 0.5 * GUARD_L
                else:  # nothing else moved far enough to matter to the check's test
                    rest = np.abs(oracle.unwrapped(nxt, box) - oracle.unwrapped(st, box))[2:]
                    assert rest.max() < 0.4
            st = nxt
            ref[e].append(st)
    return ref


@pytest.mark.parametrize("kind", ["crowd", "lone"])
def test_guard_case_conditions_hold_for_the_oracle(oracle_mod, kind):
    box, states, f_ext, who, acts = _guard_case(kind)
    op = oracle.make_params(box, DT, 0.02, 0.02, 42, SPECIES)
    _guard_oracle(op, kind, box, states, f_ext, who, acts)


@pytest.mark.gpu
@HELPER
@pytest.mark.parametrize("kind", ["crowd", "lone"])
def test_guard_sends_only_the_far_movers_env_to_the_rerun(gpu, kind, helper, monkeypatch):
    """A 20 um box (a quarter: 5 um), two windows (_guard_case).  Both envs
    equal the oracle, env 0 through the exact re-run, env 1 on its run waves."""
    from gpu_harness import Harness

    monkeypatch.setenv("SWARMRL_AMD_ROT_HELPER", helper)
    # (192 colloids in 400 um^2: the plan would take the neighbour-list path)
    monkeypatch.setenv("SWARMRL_AMD_NLIST", "0")
    box, states, f_ext, who, acts = _guard_case(kind)
    h = Harness(box, DT, 0.02, 0.02, 42, SPECIES, np.zeros(N, int), n_envs=E)
    ref = _guard_oracle(h.op, kind, box, states, f_ext, who, acts)
    h.upload(states)
    h.set_external_force(f_ext)
    for w, (f, t) in enumerate(acts):
        h.set_actions(f, t)
        h.integrate(WINDOW)
        _compare(h, [ref[0][w], ref[1][w]], ("window", w))
        fb, waves = h.window_stats()
        print("guard", kind, "helper", helper, "window", w, "fallback", fb, "waves", waves)
        assert fb[0] == 2 and fb[1] == 0 and waves[1] > 1, (fb, waves)


# ------------------------------------------------------- the fix-up pass
@pytest.mark.gpu
@HELPER
def test_second_end_through_the_fix_up_pass_bit_exact(gpu, helper, monkeypatch):
    """Pairs at 0.62, 0.7 and 0.78 sigma (epsilon 0.02): their forces, 4700,
    930 and 215 force units, exceed the 128 that fit the speculative int32
    conversion (2^31 units of 2^-24), so their waves add the remainder in the
    fix-up pass.  One window, on the run waves."""
    from gpu_harness import Harness

    monkeypatch.setenv("SWARMRL_AMD_ROT_HELPER", helper)
    rng = np.random.default_rng(1503)
    L = 40.0
    box = [L] * 3
    eps = 0.02
    states = []
    for e in range(E):
        pos = _site_env(rng, L)
        for k, frac in enumerate((0.62, 0.7, 0.78, 0.62, 0.7, 0.78)):
            i = 3 * (5 + 9 * k)  # the first two members of six sites
            u = 2 * np.pi * rng.random()
            pos[i + 1, :2] = pos[i, :2] + frac * 0.1 * np.array([np.cos(u), np.sin(u)])
        states.append(oracle.state_from_positions(pos, _dirs(rng, N), box))
    h = Harness(box, DT, 0.1, eps, 42, SPECIES, np.zeros(N, int), n_envs=E)
    h.upload(states)
    f = rng.uniform(0.0, 1.0, E * N).astype(np.float32)
    t = (rng.normal(size=E * N) * 5).astype(np.float32)
    h.set_actions(f, t)
    h.integrate(WINDOW)
    sp = np.zeros(N, np.uint8)
    ref = []
    for e in range(E):
        s = slice(e * N, (e + 1) * N)
        one, _, _ = oracle.bd_run(h.op, states[e], sp, f[s], t[s], 1, env=e)
        # the first sub-step's pair force moved the closest pair's ends by more
        # than 128 force units' worth
        step = np.abs(oracle.unwrapped(one, box) - oracle.unwrapped(states[e], box)).max()
        assert step > 128.0 * DT / GAMMA_T * 2, step
        ref.append(oracle.bd_run(h.op, states[e], sp, f[s], t[s], WINDOW, env=e)[0])
    _compare(h, ref, "fix-up")
    fb, waves = h.window_stats()
    print("fix-up helper", helper, "fallback", fb, "waves", waves)
    assert np.all(fb == 0) and np.all(waves > 1), (fb, waves)


# ------------------------------------------- the identity and its guard, CPU
def _windows(rng, n, steps, dq_max):
    q0 = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    dq = rng.integers(-dq_max, dq_max + 1, (n, steps)).astype(np.int64)
    return q0, dq


def _carry_both_ways(q0, dq):
    """Per window: the sum of the per-sub-step carries floor((q + dq) / 2^32)
    (advance), the one carry floor((q0 + d) / 2^32) from d = (int32)(q_end - q0)
    (window_carry), and whether |(int32)(q_s - q0)| < 2^30 after every s."""
    q = q0.astype(np.int64)
    per_step = np.zeros(len(q0), np.int64)
    ok = np.ones(len(q0), bool)
    for s in range(dq.shape[1]):
        t = q + dq[:, s]
        per_step += t >> 32
        q = t & 0xFFFFFFFF
        d = ((q - q0.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        ok &= np.abs(d.astype(np.int64)) < 2 ** 30
    d = ((q - q0.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)
    once = (q0.astype(np.int64) + d) >> 32
    return per_step, once, ok, d


def test_window_carry_identity_and_guard_numpy():
    rng = np.random.default_rng(1504)
    # 100-step windows, sub-step displacements up to 2^26 units: most stay
    # inside the guard, and every one that does carries the same either way
    q0, dq = _windows(rng, 20000, 100, 2 ** 26)
    per_step, once, ok, d = _carry_both_ways(q0, dq)
    assert ok.sum() > 15000 and (~ok).sum() > 0
    assert np.array_equal(per_step[ok], once[ok])
    assert np.array_equal(dq.sum(axis=1)[ok], d[ok])
    # single sub-steps of up to 2^31 - 1 units: whatever passes the guard is
    # still exact (a wrapped displacement cannot pass it)
    q0, dq = _windows(rng, 20000, 3, 2 ** 31 - 1)
    per_step, once, ok, d = _carry_both_ways(q0, dq)
    assert ok.sum() > 50
    assert np.array_equal(per_step[ok], once[ok])
    # the guard is needed: windows that drift more than half a box end with a
    # wrapped d, and the one carry is then wrong
    q0, dq = _windows(rng, 2000, 100, 2 ** 26)
    dq += 2 ** 25  # a drift of 100 * 2^25 = 0.78 box
    per_step, once, ok, d = _carry_both_ways(q0, dq)
    assert not ok.any()
    assert (per_step != once).sum() > 1000
    # and the float test of the kernel cannot pass a 2^30-unit displacement:
    # (float)(2^30) * sx squared against (0.99 L / 4)^2, over box sizes
    for L in rng.uniform(1.0, 1000.0, 2000):
        sx = np.float32(L / 2.0 ** 32)
        dd = np.float32(2 ** 30) * sx
        assert np.float32(dd * dd) >= np.float32((0.99 * 0.25 * L) ** 2)
