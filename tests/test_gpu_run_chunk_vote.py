"""
The latency schedule's run wave (k_cluster_run_wide) votes on its speculative
int32 conversions once per chunk of SWARM_RUN_VOTE_CHUNK sub-steps, and rolls
a flagged chunk back to redo it with the voting sub-step (run_chunks in
swarm_integrator.cuh).  Bit for bit against the CPU oracle, on the run waves
(no exact re-run), with both settings of the rotation helper:

  * a pair driven together by a constant external force whose WCA force
    first passes the 128 force units of the speculation (2^31 units of 2^-24)
    at a sub-step s* in the middle of a chunk after the first, and stays above
    them across a chunk boundary -- the pair accumulator and the rollback;
  * three colloids pressed together so that every pair force stays below 128
    units while their sum on one axis is above them -- the accumulator of the
    sums, which the pair test does not see;
  * the same three with the first such sum at the LAST sub-step of a chunk:
    only there does the accumulator of the sums decide alone (a sum overflow
    the wave misses earlier in a chunk presses the three together until,
    within a few sub-steps, a pair force passes the limit too, and the pair
    accumulator flags the chunk after all);
  * windows of 1, 2, 3, K, K + 1, 2 K - 1 and 100 sub-steps, with one pair
    overflowing from the window's start and one that arrives in the window's
    last, partial chunk;
  * the same in a wave with two pair passes (a cluster of 12: 66 pairs);
  * the same geometry with no drive: no overflow, no rollback.

The chunk grid: without the helper the chunks are sub-steps 1..K, K+1..2K,
... (sub-step 0 is peeled, the last computes velocities: both vote as before,
and so do the sub-steps left over after the last whole chunk).  With the
helper the chunks begin at the sub-step after the run wave first reads that
the helper has published the whole window, which depends on timing; the
polling sub-steps before it vote as before, so the conditions below are
stated on the first grid and the helper cases see the same overflows at some
other phase of theirs: only the cases without the helper pin a rollback to a
place in its chunk.  With the helper a short window (n <= K + 1) may never
enter a chunk, and no case can put an overflow into the first chunk after
kHelpDone by construction; the window-length cases' held pair overflows from
sub-step 0 to about sub-step 30, which covers that chunk whenever the helper
is done by then.

The conditions the cases rely on are asserted on the oracle alone (CPU), with
numpy WCA forces from its positions sub-step by sub-step.

Shapes: E = 2 envs of N = 192 colloids of radius 0.05 um in a 40 um box, in 64
sites of three (clusters of three: many waves per env), epsilon 0.02.  The
time step is 1e-4 (2e-5 for the three pressed together): at 1e-3 a contact of
more than 128 units throws the two apart in one sub-step.
"""

import functools
import pathlib
import re

import numpy as np
import pytest

from oracle import oracle

ROOT = pathlib.Path(__file__).resolve().parents[1]

E, N = 2, 192
L = 40.0
BOX = [L] * 3
GAMMA_T = 4.6595
SPECIES = [(0.05, GAMMA_T, 6.2126, 1.0358e-6, 4.143e-7)]
EPS = 0.02
RC = 0.1  # the WCA cutoff of two such colloids (the oracle's: r_i + r_j)
SIG = RC / 2.0 ** (1.0 / 6.0)
LIMIT = 128.0  # force units that fit the int32 speculation
HELPER = pytest.mark.parametrize("helper", ["1", "0"])

DT, KT = 1e-4, 0.02  # the pair cases
DRIVE = 200.0  # force units on each colloid of a driven pair
# a driven colloid's drift per sub-step; a pair closes at twice that
CLOSE = 2.0 * DRIVE * DT / GAMMA_T


def _chunk():
    """The engine's chunk length K (0: it votes in every sub-step)."""
    m = re.search(r"#define SWARM_RUN_VOTE_CHUNK (\d+)",
                  (ROOT / "swarmrl_amd" / "csrc" / "swarm_integrator.cuh").read_text())
    return int(m.group(1))


K = _chunk() or 10  # (switched off: the conditions of a grid of 10)


def _wca(r):
    r = np.asarray(r, float)
    return np.where(r < RC, 24.0 * EPS / r * (2.0 * (SIG / r) ** 12 - (SIG / r) ** 6), 0.0)


def _dirs(rng, n):
    th = 2 * np.pi * rng.random(n)
    return np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1)


def _site_env(rng, k=8):
    """k x k sites on a square lattice, at each a triangle of three colloids
    0.2 um apart, one of them straight above the site's centre."""
    a = L / k
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2)
    tri = 0.2 / np.sqrt(3.0) * np.array([[np.cos(u), np.sin(u)] for u in
                                         np.pi / 2 + 2 * np.pi / 3 * np.arange(3)])
    pos = np.zeros((3 * k * k, 3))
    pos[:, :2] = ((g + 0.5) * a)[:, None, :].repeat(3, 1).reshape(-1, 2) + np.tile(tri, (k * k, 1))
    pos[:, :2] += rng.uniform(-0.002, 0.002, (3 * k * k, 2))
    return pos


def _drive_pair(pos, fe, site, d0, drive=DRIVE):
    """The first two colloids of a site d0 apart on their line, driven
    together.  (The third, 0.2 um from the first and 60 degrees off that line,
    stays 0.17 um or more from both: no contact.)"""
    i = 3 * site
    u = pos[i + 1, :2] - pos[i, :2]
    u /= np.hypot(*u)
    pos[i + 1, :2] = pos[i, :2] + d0 * u
    fe[i, :2] = drive * u
    fe[i + 1, :2] = -drive * u
    return (i, i + 1)


def _fe(f_ext, e):
    return np.ascontiguousarray(f_ext[e].T).astype(np.float32)


def _actions(rng):
    return (rng.uniform(0.0, 1.0, E * N).astype(np.float32),
            (rng.normal(size=E * N) * 5).astype(np.float32))


def _pair_forces(x, groups):
    """Per group of colloid indices: the largest pair force in it and the
    largest |axis sum| on one of its colloids (numpy WCA, unwrapped x)."""
    out = []
    for grp in groups:
        pmax, sums = 0.0, np.zeros((len(grp), 2))
        for a, i in enumerate(grp):
            for j in grp:
                if i != j:
                    d = x[i, :2] - x[j, :2]
                    r = np.hypot(*d)
                    f = float(_wca(r))
                    pmax = max(pmax, f)
                    sums[a] += f * d / r
        out.append((pmax, np.abs(sums).max()))
    return np.array(out)


def _trace(op, state, f_ext, e, act, groups, n):
    """The oracle sub-step by sub-step: [n][groups][2] forces at each
    sub-step's start, and the state after n sub-steps in one run."""
    f, t = act
    s_ = slice(e * N, (e + 1) * N)
    sp = np.zeros(N, np.uint8)
    st, tr = state, []
    for s in range(n):
        tr.append(_pair_forces(oracle.unwrapped(st, BOX), groups))
        st, _, _ = oracle.bd_run(op, st, sp, f[s_], t[s_], 1, step0=s, env=e, f_ext=_fe(f_ext, e))
    end, _, _ = oracle.bd_run(op, state, sp, f[s_], t[s_], n, env=e, f_ext=_fe(f_ext, e))
    for key in ("q", "img", "ang"):  # (sub-step by sub-step is the same run)
        assert np.array_equal(st[key], end[key])
    return np.array(tr).reshape(n, len(groups), 2), end


# --------------------------------------------------- mid-window pair overflow
MID_N = 100
# gaps tried in turn for a first overflow in mid-chunk (one more sub-step of
# approach each); the first whose oracle run meets _mid_ok is the case
MID_GAPS = [0.18 + CLOSE * k for k in range(-2, 8)]


def _mid_ok(F):
    """F[s]: the pair's force.  s*: its first sub-step above the limit, in a
    whole chunk after the first and not that chunk's first sub-step; and
    above the limit on both sides of a later boundary between whole chunks."""
    over = F > LIMIT
    if not over.any():
        return None
    s = int(np.argmax(over))
    whole = (MID_N - 2) // K  # chunks 1..K, ..., all before the last sub-step
    if not (K < s <= whole * K and (s - 1) % K != 0):
        return None
    bounds = [b for b in range(K, whole * K, K) if b >= s and over[b] and over[b + 1]]
    return (s, bounds) if bounds else None


def _mid_env(rng, gap, two_pass):
    pos = _site_env(rng)
    if two_pass:  # sites 1, 2, 3 beside site 0: one cluster of 12, 66 pairs
        for k, off in ((1, (0.5, 0.0)), (2, (0.0, 0.5)), (3, (0.5, 0.5))):
            c = pos[3 * k:3 * k + 3, :2].mean(0)
            pos[3 * k:3 * k + 3, :2] += pos[0:3, :2].mean(0) + np.array(off) - c
    fe = np.zeros((N, 3))
    pair = _drive_pair(pos, fe, 0 if two_pass else 20, gap)
    return pos, fe, pair


@functools.lru_cache(maxsize=None)
def _mid_case(two_pass):
    """Both envs with one driven pair each, env 1's one sub-step of approach
    farther apart; the gap: the first of MID_GAPS whose env 0 meets _mid_ok."""
    op = oracle.make_params(BOX, DT, KT, EPS, 42, SPECIES)
    for gap in MID_GAPS:
        rng = np.random.default_rng(1601)
        envs = [_mid_env(rng, gap + e * CLOSE, two_pass) for e in range(E)]
        states = [oracle.state_from_positions(p, _dirs(rng, N), BOX) for p, _, _ in envs]
        f_ext = np.stack([f for _, f, _ in envs])
        act = _actions(rng)
        tr0, end0 = _trace(op, states[0], f_ext, 0, act, [envs[0][2]], MID_N)
        ok = _mid_ok(tr0[:, 0, 0])
        if ok:
            tr1, end1 = _trace(op, states[1], f_ext, 1, act, [envs[1][2]], MID_N)
            return states, f_ext, act, [end0, end1], ok, tr0[:, 0, 0], tr1[:, 0, 0]
    raise AssertionError("no gap of MID_GAPS puts the first overflow in mid-chunk")


@pytest.mark.parametrize("two_pass", [False, True])
def test_mid_window_overflow_conditions_hold_for_the_oracle(oracle_mod, two_pass):
    _, _, _, _, (s, bounds), F0, F1 = _mid_case(two_pass)
    print("mid-window overflow, K", K, "two-pass", two_pass, "s*", s, "boundaries", bounds)
    print(np.round(F0[:60]), np.round(F1[:60]), sep="\n")
    assert F0[s] > LIMIT and np.all(F0[:s] <= LIMIT)
    assert K < s and (s - 1) % K != 0
    assert all(F0[b] > LIMIT and F0[b + 1] > LIMIT and b % K == 0 for b in bounds)
    assert (F1 > LIMIT).any()


@pytest.fixture(scope="module")
def gpu():
    import torch

    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _run_and_compare(helper, monkeypatch, dt, kT, states, f_ext, act, n, ref, what):
    from gpu_harness import Harness

    monkeypatch.setenv("SWARMRL_AMD_ROT_HELPER", helper)
    h = Harness(BOX, dt, kT, EPS, 42, SPECIES, np.zeros(N, int), n_envs=E)
    h.upload(states)
    h.set_external_force(f_ext)
    h.set_actions(*act)
    h.integrate(n)
    got = h.download()
    fb, waves = h.window_stats()
    print(what, "helper", helper, "n_steps", n, "fallback", fb, "waves", waves)
    for e in range(E):
        for key in ("q", "img", "ang"):
            assert np.array_equal(got[e][key], ref[e][key]), (what, n, e, key)
    assert np.all(fb == 0) and np.all(waves > 1), (fb, waves)


@pytest.mark.gpu
@HELPER
@pytest.mark.parametrize("two_pass", [False, True])
def test_mid_window_pair_overflow_bit_exact(gpu, two_pass, helper, monkeypatch):
    states, f_ext, act, ref, _, _, _ = _mid_case(two_pass)
    _run_and_compare(helper, monkeypatch, DT, KT, states, f_ext, act, MID_N, ref,
                     "mid-window overflow" + (", two passes" if two_pass else ""))


# --------------------------------------------------------------- sum overflow
SUM_DT, SUM_KT, SUM_N = 2e-5, 0.002, 60
SUM_DRIVE, SUM_R = 155.0, 0.053
SUM_SITES = (20, 41)
SUM_END_DT = 4e-5


def _sum_build(radius, sites, seed, dt=None):
    """At `sites` of each env the three colloids on a circle of `radius` about
    their centre (pairs just in contact), each pressed towards it: at rest a
    pair force of SUM_DRIVE / sqrt(3) and, on the colloid straight above the
    centre, a y sum of SUM_DRIVE.  Env 1's circles are 0.5 nm wider."""
    rng = np.random.default_rng(seed)
    op = oracle.make_params(BOX, dt or SUM_DT, SUM_KT, EPS, 42, SPECIES)
    states, fes, groups = [], [], []
    for e in range(E):
        pos = _site_env(rng)
        fe = np.zeros((N, 3))
        for site in sites:
            i = 3 * site
            c = pos[i:i + 3, :2].mean(0)
            for k in range(3):
                u = pos[i + k, :2] - c
                u /= np.hypot(*u)
                pos[i + k, :2] = c + (radius + 0.0005 * e) * u
                fe[i + k, :2] = -SUM_DRIVE * u
        states.append(oracle.state_from_positions(pos, _dirs(rng, N), BOX))
        fes.append(fe)
        groups.append([tuple(range(3 * s, 3 * s + 3)) for s in sites])
    f_ext = np.stack(fes)
    act = _actions(rng)
    out = [_trace(op, states[e], f_ext, e, act, groups[e], SUM_N) for e in range(E)]
    return states, f_ext, act, [o[1] for o in out], [o[0] for o in out]


@functools.lru_cache(maxsize=None)
def _sum_case():
    return _sum_build(SUM_R, SUM_SITES, 1602)


def _sum_end_ok(tr):
    """tr: env 0's trace.  The first sub-step with an axis sum above the
    limit is the LAST of a whole chunk (of the grid 1..K, K+1..2K, ...), by
    3 % or more, with every sum before it and every pair force of the window
    below the limit by 3 % or more."""
    sums, pairs = tr[:, :, 1].max(1), tr[:, :, 0].max(1)
    over = sums > LIMIT
    if not over.any() or pairs.max() >= 0.97 * LIMIT:
        return None
    s = int(np.argmax(over))
    whole = (SUM_N - 2) // K
    if s % K != 0 or not K <= s <= whole * K:
        return None
    if sums[s] <= 1.03 * LIMIT or sums[:s].max() >= 0.97 * LIMIT:
        return None
    return s


@functools.lru_cache(maxsize=None)
def _sum_end_case():
    """One pressed site per env, at twice the time step (the sums then rise by
    more per sub-step than the two margins take); the circle's radius: the
    first of a ladder of 0.1 nm steps that meets _sum_end_ok.
    A chunk whose only overflow is a sum at its last sub-step is flagged by
    the sums' accumulator alone, and by its last term (the one added after
    the chunk's loop): nothing later in the chunk can show the damage.  (An
    unseen sum overflow earlier in a chunk presses the three together, and
    within a few sub-steps a pair force passes the limit too.)"""
    for k in range(80):
        case = _sum_build(SUM_R + 0.0001 * k, (20,), 1604, SUM_END_DT)
        s = _sum_end_ok(case[4][0])
        if s is not None:
            return case + (s,)
    raise AssertionError("no radius of the ladder puts the first sum overflow at a chunk's end")


def test_sum_overflow_conditions_hold_for_the_oracle(oracle_mod):
    """Every pair force below the limit by 3 % or more at every sub-step, an
    axis sum above it by 3 % or more at some sub-step of a whole chunk."""
    traces = _sum_case()[4]
    for e, tr in enumerate(traces):
        over = tr[:, :, 1].max(1) > 1.03 * LIMIT
        print("sum overflow env", e, "largest pair", tr[:, :, 0].max(), "largest sum",
              tr[:, :, 1].max(), "first above", int(np.argmax(over)), "sub-steps above", over.sum())
        assert tr[:, :, 0].max() < 0.97 * LIMIT
        whole = (SUM_N - 2) // K
        assert over[1:whole * K + 1].any()


@pytest.mark.gpu
@HELPER
def test_sum_overflow_bit_exact(gpu, helper, monkeypatch):
    states, f_ext, act, ref, _ = _sum_case()
    _run_and_compare(helper, monkeypatch, SUM_DT, SUM_KT, states, f_ext, act, SUM_N, ref,
                     "sum overflow")


def test_sum_overflow_at_a_chunk_end_conditions_hold_for_the_oracle(oracle_mod):
    case = _sum_end_case()
    tr, s = case[4][0], case[5]
    sums, pairs = tr[:, :, 1].max(1), tr[:, :, 0].max(1)
    print("sum overflow at a chunk's end, K", K, "sub-step", s, "sums", np.round(sums[:s + 2]),
          "largest pair", pairs.max())
    assert s % K == 0 and K <= s <= (SUM_N - 2) // K * K
    assert sums[s] > 1.03 * LIMIT and sums[:s].max() < 0.97 * LIMIT
    assert pairs.max() < 0.97 * LIMIT


@pytest.mark.gpu
@HELPER
def test_sum_overflow_at_a_chunk_end_bit_exact(gpu, helper, monkeypatch):
    states, f_ext, act, ref, _, _ = _sum_end_case()
    _run_and_compare(helper, monkeypatch, SUM_END_DT, SUM_KT, states, f_ext, act, SUM_N, ref,
                     "sum overflow at a chunk's end")


# ------------------------------------------------------------- window lengths
LENGTHS = sorted({1, 2, 3, K, K + 1, 2 * K - 1, 100})
HELD_GAP = 0.071  # a pair in contact above the limit from the window's start


def _late_gap(n):
    """The gap of a pair that arrives about two sub-steps before the window's
    last, partial chunk ends (in a window too short for one: at its middle)."""
    return 0.0725 + CLOSE * max(n - 4, n // 2)


@functools.lru_cache(maxsize=None)
def _length_case(n, quiet=False):
    rng = np.random.default_rng(1603)
    op = oracle.make_params(BOX, DT, KT, EPS, 42, SPECIES)
    states, fes, groups = [], [], []
    for e in range(E):
        pos = _site_env(rng)
        fe = np.zeros((N, 3))
        drive = 0.0 if quiet else DRIVE
        # (quiet: the same geometry with the held pair just out of contact)
        groups.append([_drive_pair(pos, fe, 20 + e, RC + 0.002 if quiet else HELD_GAP, drive),
                       _drive_pair(pos, fe, 43 - e, _late_gap(n), drive)])
        states.append(oracle.state_from_positions(pos, _dirs(rng, N), BOX))
        fes.append(fe)
    f_ext = np.stack(fes)
    act = _actions(rng)
    out = [_trace(op, states[e], f_ext, e, act, groups[e], n) for e in range(E)]
    return states, f_ext, act, [o[1] for o in out], [o[0] for o in out]


@pytest.mark.parametrize("n", LENGTHS)
def test_window_length_conditions_hold_for_the_oracle(oracle_mod, n):
    """An overflow at the window's first sub-step and, where the window has
    sub-steps left over after its last whole chunk, one among them."""
    for tr in _length_case(n)[4]:
        over = (tr[:, :, 0] > LIMIT).any(1)
        whole = max(n - 2, 0) // K
        left = over[whole * K + 1:n - 1]
        print("window of", n, "overflowing sub-steps", np.flatnonzero(over))
        assert over[0]
        assert left.any() or left.size == 0
        assert n < 100 or left.size > 0


@pytest.mark.gpu
@HELPER
@pytest.mark.parametrize("n", LENGTHS)
def test_window_lengths_bit_exact(gpu, n, helper, monkeypatch):
    states, f_ext, act, ref, _ = _length_case(n)
    _run_and_compare(helper, monkeypatch, DT, KT, states, f_ext, act, n, ref, "window length")


def test_quiet_window_has_no_overflow_for_the_oracle(oracle_mod):
    for tr in _length_case(100, True)[4]:
        assert tr[:, :, 0].max() < 0.5 * LIMIT and tr[:, :, 1].max() < 0.5 * LIMIT


@pytest.mark.gpu
@HELPER
def test_quiet_window_bit_exact(gpu, helper, monkeypatch):
    states, f_ext, act, ref, _ = _length_case(100, True)
    _run_and_compare(helper, monkeypatch, DT, KT, states, f_ext, act, 100, ref, "quiet window")
