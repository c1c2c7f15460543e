"""The action sampler's restatement (tests/sampler_ref.py, the reference of
tests/test_gpu_sampler.py) on the CPU: it samples the reference's distribution
(gumbel_distribution.py:37-40 with random_exploration.py:54-71), feeds Philox
no counter twice, and holds uniform24's fp32 grid, the u == 1.0f draw
included."""

import numpy as np
import pytest

import sampler_ref
from sampler_ref import F32

ROW = {4: [0.1, 1.0, -0.5, 0.3], 6: [0.1, 1.0, -0.5, 0.3, 2.0, -1.5]}


@pytest.mark.parametrize("k", [4, 6])
@pytest.mark.parametrize("explore_p", [0.0, 0.3, 1.0])
def test_restatement_samples_the_reference_distribution(k, explore_p):
    """One logit row over 50 000 agents at four call counters (the high word
    set in two): frequencies (1 - p) softmax + p / k within the bound of
    test_gpu_policy.py's frequency test, 4 binomial standard deviations plus
    1e-4."""
    n_agents, counters = 50_000, [0, 1, 2**32, 2**32 + 7]
    n = n_agents * len(counters)
    logits = np.tile(np.array(ROW[k], F32), (n_agents, 1))
    count = np.zeros(k)
    for c in counters:
        s = sampler_ref.sample(logits, 0x0123456789ABCDEF, np.full(n_agents, c, np.uint64),
                               explore_p)
        count += np.bincount(s.idx, minlength=k)
        assert s.idx.min() >= 0 and s.idx.max() < k
        if explore_p == 0.0:
            assert np.array_equal(s.idx, s.greedy)
    row = np.array(ROW[k], F32).astype(np.float64)
    soft = np.exp(row - row.max()) / np.exp(row - row.max()).sum()
    want = (1.0 - explore_p) * soft + explore_p / k
    freq = count / n
    assert np.all(np.abs(freq - want) < 4 * np.sqrt(want * (1 - want) / n) + 1e-4), (freq, want)
    # logp is the chosen action's, whoever chose it
    assert np.allclose(s.logp, np.log(soft + np.float64(F32(1e-8)))[s.idx], rtol=0, atol=1e-12)


def test_no_philox_word_is_used_twice():
    """k = 64 with exploration, agents 0..255, counters {0, 1, 2^32}: every
    (counter, key) fed to Philox is distinct across agents, blocks and calls,
    and within an agent no (counter, word) is consumed twice."""
    logits = np.zeros((256, 64), F32)
    fed = set()
    total = 0
    for c in (0, 1, 2**32):
        s = sampler_ref.sample(logits, 0x0123456789ABCDEF, np.full(256, c, np.uint64), 0.3)
        assert s.words.shape == (256, 66, 5)
        for a in range(256):
            per_agent = {tuple(int(v) for v in w) for w in s.words[a]}
            assert len(per_agent) == 66, a  # 64 Gumbel words + switch + random action
            blocks = {w[:4] for w in per_agent}
            assert len(blocks) == 17, a  # 16 action blocks + the exploration block
            assert all(w[0] == a for w in blocks)
            fed |= {(*b, *s.key) for b in blocks}
            total += 17
    assert len(fed) == total == 3 * 256 * 17
    # the exploration block is the one with word 0x80000000; actions use 0..15
    assert {b[3] for b in fed} == set(range(16)) | {sampler_ref.EXPLORE_WORD}
    # counters 0 and 2^32 differ in the high word only
    assert {(b[1], b[2]) for b in fed} == {(0, 0), (1, 0), (0, 1)}


def test_word_to_action_map_and_first_maximum():
    """Action j's uniform is word j & 3 of block j >> 2: with flat logits the
    choice is the argmin of log(-log u) over the words in that order."""
    from reset_ref import philox4x32_10

    seed, c, n, k = 0xABCDEF0112345678, 2**32 + 5, 64, 7
    s = sampler_ref.sample(np.zeros((n, k), F32), seed, np.full(n, c, np.uint64), 0.0)
    a = np.arange(n, dtype=np.uint32)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    w = philox4x32_10((a, 5, 1, 0), key) + philox4x32_10((a, 5, 1, 1), key)
    u = np.stack([sampler_ref.uniform24(w[j]) for j in range(k)], 1)
    assert np.array_equal(s.idx, np.argmax(u, axis=1))  # -log(-log u) grows with u
    tie = sampler_ref.sample(np.zeros((4, 1), F32), seed, np.zeros(4, np.uint64), 0.0)
    assert np.array_equal(tie.idx, np.zeros(4, np.int64)) and np.all(np.isinf(tie.gap))


def test_unit_draw_is_found_and_wins_against_any_logit():
    """r >> 8 == 0xFFFFFF gives u == 1.0f and a Gumbel score of +inf.  Key
    (99, 0), block 0: the first hit below 2^20 agents is agent 24813 at
    counter 16, word 2 (find_unit_draws' docstring lists all three)."""
    hits = sampler_ref.find_unit_draws((99, 0), 2**15, range(17))
    assert hits[0] == (24813, 16, 2), hits
    n = 24813 + 1
    logits = np.tile(np.array([10.0, 10.0, -10.0, 10.0], F32), (n, 1))
    s = sampler_ref.sample(logits, 99, np.full(n, 16, np.uint64), 0.0)
    assert s.idx[24813] == 2 and np.isinf(s.gap[24813])
    assert np.isfinite(s.logp).all()
    assert abs(s.logp[24813] - np.log(np.exp(-20.0) / (3 + np.exp(-20.0)) + 1e-8)) < 1e-6
    # nobody else takes the action 20 below the others
    assert np.count_nonzero(s.idx == 2) == 1


def test_uniform24_grid_in_fp32():
    u = sampler_ref.uniform24(np.array([0xFFFFFFFF, 0x00000000, 0x80000100, 0x7FFFFF00],
                                       np.uint32))
    assert u.dtype == F32
    assert u[0] == F32(1.0)  # 16777215.5 rounds to even: 2^24
    assert u[1] == F32(2.0 ** -25)
    assert u[2] == F32(8388610.0 * 2.0 ** -24)  # 8388609.5 ties to even, upwards
    assert u[3] == F32(8388607.5 * 2.0 ** -24)  # below 2^23 the half is exact


def test_exploration_switch_arithmetic_in_fp32():
    """The switch is the reference's clip chain: below p the random action,
    above p + 1e-6 the Gumbel choice, in between (`frac`) a blend."""
    n, k, seed = 4096, 6, 7
    logits = np.zeros((n, k), F32)
    logits[:, 3] = 50.0
    s = sampler_ref.sample(logits, seed, np.zeros(n, np.uint64), 0.5)
    assert np.all(s.greedy == 3) and not s.frac.any()
    from reset_ref import philox4x32_10

    r = philox4x32_10((np.arange(n, dtype=np.uint32), 0, 0, 0x80000000), (7, 0))
    explore = sampler_ref.uniform24(r[0]) <= F32(0.5)
    rnd = np.minimum((sampler_ref.uniform24(r[1]) * F32(k)).astype(np.int64), k - 1)
    assert np.array_equal(s.idx, np.where(explore, rnd, 3))
    assert 0.45 < explore.mean() < 0.55
    agent = sampler_ref.agent_counters(np.array([5, -1, 2**32 + 9], np.int64), 130)
    assert agent.dtype == np.uint64 and agent[63] == 5 and agent[64] == 2**64 - 1
    assert agent[127] == 2**64 - 1 and agent[129] == 2**32 + 9
