"""
CPU restatement of the action sampler (swarm_policy.cuh: sample_logits, the
anchor every policy kernel is compared with), in numpy, from the kernel
header's written specification.  TEST INFRASTRUCTURE ONLY.

    key      (seed & 0xFFFFFFFF, seed >> 32)
    counter  action block b of agent a (its row index): (a, ctr lo, ctr hi, b);
             word q of block b belongs to action 4 b + q
    u        uniform24(word), in fp32 exactly as the kernel writes it
    g_j      logits_j - log(-log u_j), float64 from the fp32 u and logit;
             idx = the first maximum
    explore  (explore_p > 0 only) one block with counter word 0x80000000:
             word 0 the switch, word 1 the random action; the reference's
             clip arithmetic in fp32, one rounding per operation
    logp     log(softmax(logits)_idx + float32(1e-8)), float64

Nothing here is bit-equal through logf / expf: `gap` says how far the choice
is from flipping, and the GPU test compares idx only where it is wide enough.
"""

from types import SimpleNamespace

import numpy as np

from reset_ref import philox4x32_10

F32 = np.float32
M32 = 0xFFFFFFFF
EXPLORE_WORD = 0x80000000


def uniform24(word):
    """swarm::uniform24: ((float)(r >> 8) + 0.5f) * 2^-24 in fp32.  For
    r >> 8 >= 2^23 the sum is not representable and rounds to even, so the
    range is (0, 1] and r >> 8 == 0xFFFFFF gives exactly 1.0f."""
    m = (np.asarray(word, np.uint32) >> np.uint32(8)).astype(F32)
    return (m + F32(0.5)) * F32(2.0 ** -24)


def split_seed(seed):
    return int(seed) & M32, (int(seed) >> 32) & M32


def agent_counters(state, n):
    """Per-agent call counters of a state tensor: ctr[a] = state[a >> 6]."""
    state = np.ascontiguousarray(np.asarray(state).astype(np.int64, copy=False)).view(np.uint64)
    return state[np.arange(n) >> 6]


def sample(logits, seed, ctr, explore_p):
    """logits fp32 [n, k], ctr uint64 [n] (the agents' call counters) ->
    namespace of
      idx     int64 [n]    the action (after exploration)
      greedy  int64 [n]    the Gumbel-max choice before exploration
      logp    float64 [n]
      gap     float64 [n]  largest minus second largest g (inf for k = 1, and
                           for a lone u == 1; 0 where two scores are +inf)
      frac    bool [n]     the exploration switch tbc is strictly inside
                           (0, 1): idx is a blend of two indices there
      words   uint32 [n, k (+ 2), 5]  every Philox word consumed, as
                           (counter x, y, z, w, word index within the block)
      key     the Philox key (k0, k1)
    """
    logits = np.asarray(logits)
    assert logits.dtype == F32 and logits.ndim == 2
    n, k = logits.shape
    key = split_seed(seed)
    ctr = np.broadcast_to(np.asarray(ctr, np.uint64), (n,))
    a = np.arange(n, dtype=np.uint32)
    lo = (ctr & np.uint64(M32)).astype(np.uint32)
    hi = (ctr >> np.uint64(32)).astype(np.uint32)

    def used(block, q):
        return np.stack([a, lo, hi, np.full(n, block, np.uint32), np.full(n, q, np.uint32)], 1)

    u = np.empty((n, k), F32)
    words = []
    for b in range((k + 3) // 4):
        r = philox4x32_10((a, lo, hi, b), key)
        for q in range(4):
            if 4 * b + q < k:
                u[:, 4 * b + q] = uniform24(r[q])
                words.append(used(b, q))
    with np.errstate(divide="ignore"):  # u == 1: -log u = -0.0, log(-0.0) = -inf, g = +inf
        g = logits.astype(np.float64) - np.log(-np.log(u.astype(np.float64)))
    greedy = np.argmax(g, axis=1).astype(np.int64)  # the first maximum
    if k == 1:
        gap = np.full(n, np.inf)
    else:
        top = np.sort(g, axis=1)[:, -2:]
        with np.errstate(invalid="ignore"):
            gap = top[:, 1] - top[:, 0]
        gap = np.where(np.isnan(gap), 0.0, gap)  # inf - inf: two u == 1 in one row

    idx = greedy.copy()
    frac = np.zeros(n, bool)
    p = F32(explore_p)
    if p > 0:
        r = philox4x32_10((a, lo, hi, EXPLORE_WORD), key)
        words += [used(EXPLORE_WORD, 0), used(EXPLORE_WORD, 1)]
        zero, one = F32(0.0), F32(1.0)
        tbc = np.minimum(np.maximum(uniform24(r[0]) - p, zero), one)
        tbc = np.minimum(np.maximum(tbc * F32(1e6), zero), one)
        keep = np.minimum(np.maximum(tbc * F32(-10.0) + one, zero), one)
        rnd = np.minimum((uniform24(r[1]) * F32(k)).astype(np.int64), k - 1)
        blend = greedy.astype(F32) * tbc + rnd.astype(F32) * keep
        assert blend.dtype == F32 and keep.dtype == F32
        idx = blend.astype(np.int64)
        frac = (tbc > zero) & (tbc < one)

    lg = logits.astype(np.float64)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    prob = e[np.arange(n), idx] / e.sum(axis=1)
    logp = np.log(prob + np.float64(F32(1e-8)))
    return SimpleNamespace(idx=idx, greedy=greedy, logp=logp, gap=gap, frac=frac,
                           words=np.stack(words, 1), key=key)


def find_unit_draws(key, n_agents, counters, block=0):
    """Every (agent, counter, word) below n_agents, over the given call
    counters, whose word of this block has r >> 8 == 0xFFFFFF, that is
    uniform24 == 1.0f; sorted by agent.  For key (99, 0), 2^20 agents, block 0
    and counters 0..16 it finds (24813, 16, 2), (387769, 2, 3), (983179, 6, 1)."""
    a = np.arange(n_agents, dtype=np.uint32)
    hits = []
    for c in counters:
        r = philox4x32_10((a, int(c) & M32, int(c) >> 32, block), key)
        for q in range(4):
            for agent in np.nonzero((r[q] >> np.uint32(8)) == np.uint32(0xFFFFFF))[0]:
                hits.append((int(agent), int(c), q))
    return sorted(hits)
