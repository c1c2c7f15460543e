"""
The action sampler's draws (k_sample_actions, the anchor every policy kernel
is compared with bit for bit) against the numpy restatement of the kernel
header's specification, tests/sampler_ref.py: Philox counter layout, key split,
word-to-action map, the exploration block, per-group counters.

Comparison rule.  idx is exact on every agent whose Gumbel gap (largest minus
second largest score in the restatement) is >= 1e-4 and whose exploration
switch is not fractional (`frac`).  The margin: u >= 2^-25 gives
log(-log u) <= 2.86, u <= 1 - 2^-24 gives >= -16.64; with |logit| <= 10 every
score has |g| < 32, where one fp32 ulp is 1.9e-6; the inner logf's relative
error is an absolute error of the outer one.  With the device's logf within
2 ulp (no larger bound is documented for it) the total stays below 1e-5; the
margin is ten times that.  The agents left out may be at most 0.5 % of a case
(asserted; the share is in the message).  An agent with u == 1.0f has an
infinite gap and is compared.  logp: against the restatement's float64 value
on the compared agents, atol 2e-6 (test_gpu_policy.py's figure) + rtol 1e-6
(near log(1e-8) = -18.4 one fp32 ulp is already 1.9e-6).  f and t equal the
tables at idx exactly; every group with an agent advances its counter by
exactly one and the rest of `state` is untouched.

`frac` agents (switch strictly inside (0, 1), about 1e-6 of the draws at
0 < p < 1) blend two indices, idx = (int)(idx * tbc + rnd * keep).  The
library is built with -ffp-contract=off (number formats: fixed fp32
operation order), so the blend is the restatement's one-rounding-per-operation
value; test_fractional_switch_blend builds such agents and holds them to it.
Every other case keeps them in the left-out share, as the rule says (none of
them holds one).
"""

import numpy as np
import pytest
import torch

import sampler_ref
from sampler_ref import F32

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEED = 0x0123456789ABCDEF  # non-zero high word: key1 = 0x01234567
CTR = 2**32 + 5            # non-zero high counter word
MIN_GAP = 1e-4
CAP = 0.005
LOG_EPS = float(np.log(np.float64(F32(1e-8))))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


# ------------------------------------------------------------------ helpers
def _logits(n, k, seed):
    """normal * 3 clipped to |l| <= 10, fp32."""
    rng = np.random.default_rng(seed)
    return np.clip(rng.normal(size=(n, k)) * 3.0, -10.0, 10.0).astype(F32)


def _group_state(n, spare=2, base=CTR):
    """Every group its own counter, state[g] = base + 7 g, plus spare entries."""
    return base + 7 * np.arange((n + 63) // 64 + spare, dtype=np.int64)


def _tables(k):
    return (torch.arange(k, dtype=torch.float32, device=DEV) * 2.0 + 1.0,
            -torch.arange(k, dtype=torch.float32, device=DEV) - 0.5)


def _launch(logits, seed, state, explore_p):
    """ops.sample_actions on host arrays -> (idx, logp, f, t) as numpy, the
    state afterwards, and the tables."""
    from swarmrl_amd.engine import ops

    lg = torch.from_numpy(logits).to(DEV)
    st = torch.from_numpy(np.array(state, np.int64)).to(DEV)
    ftab, ttab = _tables(logits.shape[1])
    out = ops.sample_actions(lg, seed, st, explore_p, ftab, ttab)
    return [o.cpu().numpy() for o in out], st.cpu().numpy(), (ftab.cpu().numpy(),
                                                                ttab.cpu().numpy())


def _compare(case, out, tables, logits, seed, ctr, explore_p, min_gap=MIN_GAP, pin_frac=False):
    """The outputs of n agents against the restatement at the per-agent
    counters ctr; returns (restatement, compared mask)."""
    idx, logp, f, t = out
    n = len(idx)
    ref = sampler_ref.sample(logits, seed, ctr, explore_p)
    ok = (ref.gap >= min_gap) & (~ref.frac | pin_frac)
    left = int(n - ok.sum())
    print(f"{case}: left out {left} of {n} agents ({ref.frac.sum()} frac), cap {CAP * n:g}")
    assert left <= CAP * n, f"{case}: {left} of {n} agents left out ({left / n:.4%} > {CAP:.1%})"
    assert idx.min() >= 0 and idx.max() < logits.shape[1], case
    bad = np.nonzero(ok & (idx != ref.idx))[0]
    assert bad.size == 0, (case, f"{bad.size} of {ok.sum()} actions differ", bad[:8],
                           idx[bad[:8]], ref.idx[bad[:8]], ref.gap[bad[:8]])
    assert not np.isnan(logp).any(), case
    err = np.abs(logp.astype(np.float64) - ref.logp)
    tol = 2e-6 + 1e-6 * np.abs(ref.logp)
    assert np.all(err[ok] <= tol[ok]), (case, "logp", float((err - tol)[ok].max()))
    ftab, ttab = tables
    assert np.array_equal(f, ftab[idx]) and np.array_equal(t, ttab[idx]), case
    return ref, ok


def _check_counters(case, before, after, n, by=1):
    g = (n + 63) // 64
    assert np.array_equal(after[:g], before[:g] + by), case
    assert np.array_equal(after[g:], before[g:]), case


def _case(case, logits, seed, state, explore_p, min_gap=MIN_GAP, pin_frac=False):
    n = logits.shape[0]
    out, after, tables = _launch(logits, seed, state, explore_p)
    ref, ok = _compare(case, out, tables, logits, seed, sampler_ref.agent_counters(state, n),
                       explore_p, min_gap, pin_frac)
    _check_counters(case, np.asarray(state, np.int64), after, n)
    return out, ref, ok


# -------------------------------------------------------------------- cases
@pytest.mark.parametrize("explore_p", [0.0, 0.3])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 16, 63, 64])
def test_action_counts(k, explore_p):
    """n = 1000 (ragged against 64 and 256), ragged and full Philox blocks up
    to word block 15, every group its own counter with the high word set."""
    n = 1000
    _case(f"k={k} p={explore_p}", _logits(n, k, 100 + k), SEED, _group_state(n), explore_p)


def test_key_words_each_matter():
    n, k = 256, 4
    logits = _logits(n, k, 1)
    state = _group_state(n)
    a = _case("seed", logits, SEED, state, 0.3)[0]
    b = _case("seed + 2^32", logits, SEED + 2**32, state, 0.3)[0]
    c = _case("seed + 1", logits, SEED + 1, state, 0.3)[0]
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[0], c[0])
    assert not np.array_equal(b[0], c[0])


def test_counter_words_each_matter():
    n, k = 256, 4
    logits = _logits(n, k, 2)
    lo = _group_state(n, base=5)
    a = _case("ctr", logits, SEED, lo, 0.3)[0]
    b = _case("ctr + 2^32", logits, SEED, lo + 2**32, 0.3)[0]
    assert not np.array_equal(a[0], b[0])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_edges_of_n(n):
    _case(f"n={n}", _logits(n, 6, n), SEED, _group_state(n), 0.3)


@pytest.mark.parametrize("explore_p", [1e-7, 0.3, 1.0])
def test_exploration(explore_p):
    """The number of agents moved off their Gumbel choice is the
    restatement's, exactly."""
    n, k = 4096, 6
    out, ref, ok = _case(f"p={explore_p}", _logits(n, k, 7), SEED, _group_state(n), explore_p)
    assert np.count_nonzero(out[0][ok] != ref.greedy[ok]) == np.count_nonzero(
        ref.idx[ok] != ref.greedy[ok])
    if explore_p == 1.0:
        assert ok.all()  # the Gumbel choice plays no part


def test_exploration_off_a_certain_greedy_action():
    n, k = 4096, 6
    logits = _logits(n, k, 8)
    logits[:, 3] = 50.0  # outside |l| <= 10, but its gap is ~40
    out, ref, ok = _case("p=0.5 certain", logits, SEED, _group_state(n), 0.5)
    assert ok.all() and np.all(ref.greedy == 3)
    moved = np.count_nonzero(out[0] != 3)
    assert moved == np.count_nonzero(ref.idx != 3)
    assert 0.5 * 5 / 6 - 0.04 < moved / n < 0.5 * 5 / 6 + 0.04


@pytest.mark.parametrize("steps", [1, 8])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_fractional_switch_blend(which, steps):
    """explore_p set `steps` grid points (2^-24) below one agent's switch
    uniform u in [0.5, 1): u - p is exact, tbc = steps * 0.0596 lies strictly
    inside (0, 1) and that agent's action is the blend (int)(idx * tbc + rnd *
    keep), with keep = 0.404 at one step and 0 at eight.  The greedy action is
    certain (logit +50 on action 5), so the blend is neither input in general.
    Held to the restatement's fp32 value, `frac` agents included."""
    from reset_ref import philox4x32_10

    n, k = 256, 6
    state = _group_state(n)
    ctr = sampler_ref.agent_counters(state, n)
    r = philox4x32_10((np.arange(n, dtype=np.uint32), (ctr & np.uint64(0xFFFFFFFF)),
                       ctr >> np.uint64(32), sampler_ref.EXPLORE_WORD),
                      sampler_ref.split_seed(SEED))
    u = sampler_ref.uniform24(r[0])
    target = np.nonzero((u >= F32(0.5)) & (u < F32(0.9)))[0][which]
    p = u[target] - F32(steps * 2.0 ** -24)
    assert p.dtype == F32 and u[target] - p == F32(steps * 2.0 ** -24)
    logits = _logits(n, k, 13)
    logits[:, 5] = 50.0
    out, ref, ok = _case(f"frac agent {target} steps={steps}", logits, SEED, state, float(p),
                         pin_frac=True)
    assert ok.all() and ref.frac[target] and np.all(ref.greedy == 5)
    want = int(F32(5.0) * F32(F32(steps * 2.0 ** -24) * F32(1e6)))
    if steps == 8:  # keep = 0: (int)(5 * 0.4768) = 2
        assert want == 2 and ref.idx[target] == 2
    assert out[0][target] == ref.idx[target]


def test_extreme_logits():
    """Rows [50, 0, 0, 0] and [0, -80, 0, 0] with explore_p = 1, so that the
    underflowing actions are drawn: their logp is log(float32(1e-8)), nothing
    is NaN.  These rows are outside |l| <= 10 (|g| up to 97, an fp32 ulp of
    7.6e-6), so idx is compared only where the gap is >= 1e-3."""
    n, k = 256, 4
    logits = np.zeros((n, k), F32)
    logits[0::2, 0] = 50.0
    logits[1::2, 1] = -80.0
    out, ref, ok = _case("extreme", logits, SEED, _group_state(n), 1.0, min_gap=1e-3)
    idx, logp = out[0], out[1]
    under = ok & np.where(np.arange(n) % 2 == 0, idx != 0, idx == 1)
    assert under[0::2].sum() > 60 and under[1::2].sum() > 15  # both rows' cases are drawn
    assert np.all(np.abs(logp[under] - LOG_EPS) <= 2e-6 + 1e-6 * abs(LOG_EPS))
    assert np.isfinite(logp).all()
    # and without exploration the certain action is taken
    out0 = _case("extreme p=0", logits, SEED, _group_state(n), 0.0, min_gap=1e-3)[0]
    assert np.all(out0[0][0::2] == 0) and np.all(out0[0][1::2] != 1)


def test_unit_uniform_takes_the_action_whatever_its_logit():
    """Seed 99, counter 16: word 2 of agent 24813's block 0 has r >> 8 ==
    0xFFFFFF, so u == 1.0f, -logf(1.0f) = -0.0f, logf(-0.0f) = -inf and the
    score is +inf: action 2 is taken although its logit is 20 below the
    others; logp comes from the logits alone and stays finite."""
    n, k = 24832, 4
    logits = np.tile(np.array([10.0, 10.0, -10.0, 10.0], F32), (n, 1))
    state = np.full(n // 64, 16, np.int64)
    out, ref, ok = _case("u == 1", logits, 99, state, 0.0)
    assert ref.idx[24813] == 2 and np.isinf(ref.gap[24813]) and ok[24813]
    assert out[0][24813] == 2 and np.isfinite(out[1][24813])
    assert abs(out[1][24813] - ref.logp[24813]) <= 2e-6 + 1e-6 * abs(ref.logp[24813])


def test_captured_graph_replays_draw_at_the_advancing_counters():
    """One captured ops.sample_actions: replay i draws at the counters the
    state held before it.  Launches that ran: the warm-up and three replays
    (capturing launches nothing), so the state ends at start + 4."""
    from swarmrl_amd.engine import ops

    n, k, p = 1000, 6, 0.3
    logits = _logits(n, k, 9)
    start = _group_state(n)
    lg = torch.from_numpy(logits).to(DEV)
    st = torch.from_numpy(start.copy()).to(DEV)
    ftab, ttab = _tables(k)
    tables = (ftab.cpu().numpy(), ttab.cpu().numpy())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm = ops.sample_actions(lg, SEED, st, p, ftab, ttab)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.sample_actions(lg, SEED, st, p, ftab, ttab)
    torch.cuda.synchronize()
    _check_counters("after capture", start, st.cpu().numpy(), n, by=1)
    _compare("warm-up", [o.cpu().numpy() for o in warm], tables, logits, SEED,
             sampler_ref.agent_counters(start, n), p)
    seen = []
    for i in range(3):
        before = st.cpu().numpy()
        _check_counters(f"before replay {i}", start, before, n, by=1 + i)
        g.replay()
        torch.cuda.synchronize()
        got = [o.cpu().numpy() for o in out]
        _compare(f"replay {i}", got, tables, logits, SEED,
                 sampler_ref.agent_counters(before, n), p)
        seen.append(got[0])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    _check_counters("after three replays", start, st.cpu().numpy(), n, by=4)


# ------------------------------------------- one link per kernel family
def test_one_kernel_mlp_policy_draws_as_restated():
    """ops.policy_mlp_sample's actions against the restatement on the logits
    it returns: the pin reaches sample_logits_reg without passing through
    k_sample_actions."""
    from swarmrl_amd.engine import ops
    from swarmrl_amd.networks import ActorCriticMLP

    n, d_in, hidden, k, p = 1000, 3, 100, 6, 0.3
    torch.manual_seed(11)
    net = ActorCriticMLP(d_in, k, hidden).to(DEV)
    obs = torch.randn(n, d_in, device=DEV)
    start = _group_state(n)
    st = torch.from_numpy(start.copy()).to(DEV)
    ftab, ttab = _tables(k)
    with torch.no_grad():
        *out, lg = ops.policy_mlp_sample(obs, *net.rollout_layers(), SEED, st, p, ftab, ttab,
                                         want_logits=True)
    logits = lg.cpu().numpy()
    assert np.abs(logits).max() <= 10.0  # the margin's premise
    _compare("mlp", [o.cpu().numpy() for o in out], (ftab.cpu().numpy(), ttab.cpu().numpy()),
             logits, SEED, sampler_ref.agent_counters(start, n), p)
    _check_counters("mlp", start, st.cpu().numpy(), n)


def test_ensemble_policy_members_draw_as_restated():
    """ops.policy_ensemble_sample: member m draws with seeds[m] at
    state[m][row >> 6], the agent index being the row within the member."""
    from swarmrl_amd.engine import ops

    M, n_per, d_in, hidden, k, p = 3, 130, 3, 100, 6, 0.3
    gen = torch.Generator().manual_seed(12)
    obs = torch.randn(M, n_per, d_in, generator=gen).to(DEV)
    w1 = (torch.randn(M, hidden, d_in, generator=gen) / d_in ** 0.5).to(DEV)
    b1 = (0.1 * torch.randn(M, hidden, generator=gen)).to(DEV)
    w2 = (torch.randn(M, k, hidden, generator=gen) / hidden ** 0.5).to(DEV)
    b2 = (0.1 * torch.randn(M, k, generator=gen)).to(DEV)
    seeds = [SEED, 0x7EDCBA9876543210, 0x0000000500000003]
    start = np.stack([_group_state(n_per, spare=1, base=CTR + 1000 * m) for m in range(M)])
    st = torch.from_numpy(start.copy()).to(DEV)
    ftab, ttab = _tables(k)
    *out, lg = ops.policy_ensemble_sample(obs, w1, b1, w2, b2,
                                          torch.tensor(seeds, dtype=torch.int64, device=DEV), st,
                                          p, ftab, ttab, want_logits=True)
    logits = lg.cpu().numpy().reshape(M, n_per, k)
    assert np.abs(logits).max() <= 10.0  # the margin's premise
    out = [o.cpu().numpy().reshape(M, n_per) for o in out]
    after = st.cpu().numpy()
    tables = (ftab.cpu().numpy(), ttab.cpu().numpy())
    idx = []
    for m in range(M):
        _compare(f"member {m}", [o[m] for o in out], tables, logits[m], seeds[m],
                 sampler_ref.agent_counters(start[m], n_per), p)
        _check_counters(f"member {m}", start[m], after[m], n_per)
        idx.append(sampler_ref.sample(logits[m], seeds[m],
                                      sampler_ref.agent_counters(start[m], n_per), p).idx)
    # the members' streams differ where their logits do not decide
    assert not np.array_equal(idx[0], idx[1]) and not np.array_equal(idx[1], idx[2])
