"""
The ensemble rollout policy (swarm_policy_ensemble_sample,
csrc/swarm_ensemble.cuh) against its oracle: M calls of the single-model
kernel (ops.policy_mlp_sample) on the members' slices with the members' seeds
and cloned counters.  The contract is bit identity -- a member's results do
not depend on who shares the launch -- so every comparison is torch.equal.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _problem(M, n_per, d_in, hidden, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(M, n_per, d_in, generator=g).to(DEV)
    w1 = (torch.randn(M, hidden, d_in, generator=g) / d_in ** 0.5).to(DEV)
    b1 = (0.1 * torch.randn(M, hidden, generator=g)).to(DEV)
    w2 = (torch.randn(M, k, hidden, generator=g) / hidden ** 0.5).to(DEV)
    b2 = (0.1 * torch.randn(M, k, generator=g)).to(DEV)
    seeds = torch.randint(0, 2 ** 62, (M,), generator=g).to(DEV)
    state = torch.zeros(M, (n_per + 63) // 64, dtype=torch.int64, device=DEV)
    ftab = torch.arange(k, dtype=torch.float32, device=DEV) * 0.5
    ttab = torch.arange(k, dtype=torch.float32, device=DEV) - 1.0
    return obs, w1, b1, w2, b2, seeds, state, ftab, ttab


def _ensemble(p, explore_p, state):
    from swarmrl_amd.engine import ops

    obs, w1, b1, w2, b2, seeds, _, ftab, ttab = p
    return ops.policy_ensemble_sample(obs, w1, b1, w2, b2, seeds, state, explore_p, ftab, ttab,
                                      want_logits=True)


def _loop(p, explore_p, state):
    """The oracle: one policy_mlp_sample per member on its slices; advances
    `state` [M, groups] row by row."""
    from swarmrl_amd.engine import ops

    obs, w1, b1, w2, b2, seeds, _, ftab, ttab = p
    outs = []
    for m in range(obs.shape[0]):
        st = state[m].clone()
        outs.append(ops.policy_mlp_sample(obs[m], w1[m], b1[m], w2[m], b2[m],
                                          int(seeds[m].item()), st, explore_p, ftab, ttab,
                                          want_logits=True))
        state[m].copy_(st)
    return tuple(torch.cat([o[i] for o in outs]) for i in range(5))


# tests/test_gpu_policy.py::LADDER_CELLS for two members: every (D, K)
# template arm of the host's variant ladder at 4, 2 and 1 lanes per agent.
LADDER_CELLS = [(2, n_per, d_in, 100, k, 0.0) for n_per in (1000, 20_000, 70_000)
                for d_in, k in ((3, 4), (4, 6), (9, 4), (16, 16))]


@pytest.mark.parametrize("M,n_per,d_in,hidden,k,explore_p", [
    (3, 70, 3, 128, 4, 0.0),     # a partial counter group; a member boundary inside a block
    (2, 1, 1, 100, 3, 0.0),      # ragged hidden, one agent
    (3, 130, 16, 256, 16, 0.3),  # the wide template, with exploration
    (2, 16385, 3, 128, 4, 0.0),  # G = 2
    (2, 65537, 3, 128, 4, 0.0),  # G = 1
    *LADDER_CELLS,
])
def test_ensemble_equals_member_calls(M, n_per, d_in, hidden, k, explore_p):
    p = _problem(M, n_per, d_in, hidden, k, seed=n_per)
    st_e, st_l = p[6].clone(), p[6].clone()
    for call in range(2):  # the second call draws from the advanced counters
        got = _ensemble(p, explore_p, st_e)
        want = _loop(p, explore_p, st_l)
        for name, a, b in zip(("idx", "logp", "f", "t", "logits"), got, want):
            assert torch.equal(a, b), (name, call)
        assert torch.equal(st_e, st_l), call
    groups = (n_per + 63) // 64
    assert torch.equal(st_e, torch.full((M, groups), 2, dtype=torch.int64, device=DEV))


def test_members_draw_from_their_own_streams():
    """Equal weights and observations, different seeds: the members' actions
    differ (and with equal seeds they would not)."""
    M, n_per = 3, 512
    obs, w1, b1, w2, b2, seeds, state, ftab, ttab = _problem(M, n_per, 3, 128, 4)
    same = tuple(t[:1].expand_as(t).contiguous() for t in (obs, w1, b1, w2, b2))
    p = (*same, seeds, state, ftab, ttab)
    idx, logp, _, _, logits = _ensemble(p, 0.0, state.clone())
    idx, logits = idx.reshape(M, n_per), logits.reshape(M, n_per, 4)
    assert torch.equal(logits[0], logits[1]) and torch.equal(logits[0], logits[2])
    assert not torch.equal(idx[0], idx[1]) and not torch.equal(idx[1], idx[2])
    eq = (*same, seeds[:1].expand(M).contiguous(), state, ftab, ttab)
    idx = _ensemble(eq, 0.0, state.clone())[0].reshape(M, n_per)
    assert torch.equal(idx[0], idx[1]) and torch.equal(idx[0], idx[2])


def test_swapping_members_swaps_outputs():
    M, n_per, k = 3, 200, 4
    p = _problem(M, n_per, 3, 128, k, seed=3)
    state = p[6].clone()
    state[:, 0] = torch.tensor([5, 9, 2], device=DEV)  # counters that differ by member
    perm = torch.tensor([2, 1, 0], device=DEV)
    a = _ensemble(p, 0.0, state.clone())
    st_b = state[perm].contiguous()
    q = tuple(t[perm].contiguous() for t in p[:6]) + (st_b, p[7], p[8])
    b = _ensemble(q, 0.0, st_b)
    for x, y in zip(a, b):
        x = x.reshape(M, n_per, *x.shape[1:])
        y = y.reshape(M, n_per, *y.shape[1:])
        assert torch.equal(x[perm], y)


def test_out_of_limit_sizes_are_rejected_and_write_nothing():
    from swarmrl_amd.engine import ops

    def attempt(M, d_in, hidden, k, n_state=None):
        obs, w1, b1, w2, b2, seeds, state, ftab, ttab = _problem(M, 8, d_in, hidden, k)
        if n_state is not None:
            state = torch.zeros(M, n_state, dtype=torch.int64, device=DEV)
        n = M * 8
        out = (torch.full((n,), -7, dtype=torch.int64, device=DEV),
               *(torch.full((n,), -7.0, device=DEV) for _ in range(3)))
        with pytest.raises(ValueError):
            ops.policy_ensemble_sample(obs, w1, b1, w2, b2, seeds, state, 0.0, ftab, ttab,
                                       out=out)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in out)
        assert int(state.abs().sum()) == 0

    attempt(2, 17, 128, 4)    # d_in > 16
    attempt(2, 3, 257, 4)     # hidden > 256
    attempt(2, 3, 128, 17)    # k > 16
    attempt(1025, 1, 8, 2)    # M > 1024
    obs, w1, b1, w2, b2, seeds, _, ftab, ttab = _problem(2, 70, 3, 16, 4)
    short = torch.zeros(2, 1, dtype=torch.int64, device=DEV)  # 70 agents need 2 groups
    with pytest.raises(ValueError):
        ops.policy_ensemble_sample(obs, w1, b1, w2, b2, seeds, short, 0.0, ftab, ttab)
    with pytest.raises(ValueError):  # explore_p outside [0, 1]
        ops.policy_ensemble_sample(obs, w1, b1, w2, b2, seeds,
                                   torch.zeros(2, 2, dtype=torch.int64, device=DEV), 1.5, ftab,
                                   ttab)


def test_captured_launch_draws_fresh_numbers_and_matches_eager():
    from swarmrl_amd.engine import ops

    M, n_per, k = 3, 70, 4
    p = _problem(M, n_per, 3, 128, k, seed=8)
    obs, w1, b1, w2, b2, seeds, state, ftab, ttab = p
    st_g, st_e = state.clone(), state.clone()
    n = M * n_per
    out = (torch.empty(n, dtype=torch.int64, device=DEV),
           *(torch.empty(n, device=DEV) for _ in range(3)))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        ops.policy_ensemble_sample(obs, w1, b1, w2, b2, seeds, st_g, 0.0, ftab, ttab, out=out)
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append(tuple(t.clone() for t in out))
    assert not torch.equal(replays[0][0], replays[1][0])  # fresh numbers per replay
    for r in replays:
        want = _loop(p, 0.0, st_e)
        for a, b in zip(r, want[:4]):
            assert torch.equal(a, b)
    assert torch.equal(st_g, st_e)
