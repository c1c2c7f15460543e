"""
The deep ensemble rollout policy (swarm_policy_deep_ensemble_sample,
csrc/swarm_ensemble.cuh over csrc/swarm_deep.cuh) against its oracle: M calls
of the single-model kernel (ops.policy_deep_sample) on aligned clones of the
members (ens.member(m)) with the members' seeds and counter slices.  The
contract is bit identity -- a member's results do not depend on who shares the
launch, nor on where its slice of a stacked tensor starts -- so every
comparison is torch.equal.
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
    from swarmrl_amd.networks import EnsembleDeepActorCriticMLP

    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    ens = EnsembleDeepActorCriticMLP(M, d_in, k, hidden).to(DEV)
    obs = torch.randn(M, n_per, d_in, generator=g).to(DEV)
    seeds = torch.randint(0, 2 ** 62, (M,), generator=g).to(DEV)
    state = torch.zeros(M, (n_per + 63) // 64, dtype=torch.int64, device=DEV)
    ftab = torch.arange(k, dtype=torch.float32, device=DEV) * 0.5
    ttab = torch.arange(k, dtype=torch.float32, device=DEV) - 1.0
    return ens, obs, seeds, state, ftab, ttab


def _ensemble(p, explore_p, state):
    from swarmrl_amd.engine import ops

    ens, obs, seeds, _, ftab, ttab = p
    return ops.policy_deep_ensemble_sample(obs, *ens.rollout_layers(), seeds, state, explore_p,
                                           ftab, ttab, want_logits=True)


def _loop(p, members, explore_p, state):
    """The oracle: one policy_deep_sample per member; advances `state`
    [M, groups] row by row."""
    from swarmrl_amd.engine import ops

    _, obs, seeds, _, ftab, ttab = p
    outs = []
    for m, net in enumerate(members):
        ws, bs, wa, ba, _, _ = net.deep_layers()
        st = state[m].clone()
        outs.append(ops.policy_deep_sample(obs[m].clone(), ws, bs, wa, ba, int(seeds[m].item()),
                                           st, explore_p, ftab, ttab, want_logits=True))
        state[m].copy_(st)
    return tuple(torch.cat([o[i] for o in outs]) for i in range(5))


@pytest.mark.parametrize("M,n_per,d_in,hidden,k,explore_p", [
    (3, 1, 2, (16, 16), 4, 0.0),             # one agent per member
    (2, 64, 3, (128, 128), 4, 0.0),          # exactly one counter group
    (3, 65, 3, (13, 7), 3, 0.3),             # ragged second block and widths, unaligned slices
    (2, 200, 32, (128, 128, 128), 16, 0.0),  # every limit at once, K = 16, three layers
])
def test_ensemble_equals_member_calls(M, n_per, d_in, hidden, k, explore_p):
    p = _problem(M, n_per, d_in, hidden, k, seed=n_per)
    members = [p[0].member(m) for m in range(M)]
    st_e, st_l = p[3].clone(), p[3].clone()
    for call in range(2):  # the second call draws from the advanced counters
        got = _ensemble(p, explore_p, st_e)
        want = _loop(p, members, explore_p, st_l)
        for name, a, b in zip(("idx", "logp", "f", "t", "logits"), got, want):
            assert torch.equal(a, b), (name, call)
        assert torch.equal(st_e, st_l), call
    groups = (n_per + 63) // 64
    assert torch.equal(st_e, torch.full((M, groups), 2, dtype=torch.int64, device=DEV))
    # the members are different networks drawing from different streams
    logits = got[4].reshape(M, n_per, k)
    assert not torch.equal(logits[0], logits[1])


def _raw(M, n_per, d_in, hidden, k):
    """Stacked zero parameters of any size (the limit checks read no weight)."""
    prev, ws, bs = d_in, [], []
    for h in hidden:
        ws.append(torch.zeros(M, h, prev, device=DEV))
        bs.append(torch.zeros(M, h, device=DEV))
        prev = h
    wa, ba = torch.zeros(M, k, prev, device=DEV), torch.zeros(M, k, device=DEV)
    obs = torch.zeros(M, n_per, d_in, device=DEV)
    seeds = torch.zeros(M, dtype=torch.int64, device=DEV)
    tab = torch.zeros(k, device=DEV)
    return obs, ws, bs, wa, ba, seeds, tab


def test_out_of_limit_sizes_are_rejected_and_write_nothing():
    from swarmrl_amd.engine import ops

    def attempt(M, d_in, hidden, k, n_state=1, explore_p=0.0, n_per=8):
        obs, ws, bs, wa, ba, seeds, tab = _raw(M, n_per, d_in, hidden, k)
        state = torch.zeros(M, n_state, dtype=torch.int64, device=DEV)
        n = M * n_per
        out = (torch.full((n,), -7, dtype=torch.int64, device=DEV),
               *(torch.full((n,), -7.0, device=DEV) for _ in range(3)))
        with pytest.raises(ValueError):
            ops.policy_deep_ensemble_sample(obs, ws, bs, wa, ba, seeds, state, explore_p, tab,
                                            tab, out=out)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in out)
        assert int(state.abs().sum()) == 0

    attempt(1025, 1, (8, 8), 2)         # M > 1024
    attempt(2, 3, (129, 16), 4)         # a width of 129
    attempt(2, 3, (16, 129), 4)
    attempt(2, 3, (16,), 4)             # one hidden layer
    attempt(2, 3, (16, 16, 16, 16), 4)  # four hidden layers
    attempt(2, 33, (16, 16), 4)         # d_in > 32
    attempt(2, 3, (16, 16), 17)         # k > 16
    attempt(2, 3, (16, 16), 4, n_per=70)        # 70 agents need 2 counter groups
    attempt(2, 3, (16, 16), 4, explore_p=1.5)   # explore_p outside [0, 1]


def test_captured_launch_draws_fresh_numbers_and_matches_eager():
    from swarmrl_amd.engine import ops

    M, n_per, k = 3, 70, 4
    p = _problem(M, n_per, 3, (32, 24), k, seed=8)
    ens, obs, seeds, state, ftab, ttab = p
    members = [ens.member(m) for m in range(M)]
    st_g, st_e = state.clone(), state.clone()
    n = M * n_per
    out = (torch.empty(n, dtype=torch.int64, device=DEV),
           *(torch.empty(n, device=DEV) for _ in range(3)))
    layers = ens.rollout_layers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        ops.policy_deep_ensemble_sample(obs, *layers, seeds, st_g, 0.0, ftab, ttab, out=out)
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append(tuple(t.clone() for t in out))
    assert not torch.equal(replays[0][0], replays[1][0])  # fresh numbers per replay
    for r in replays:
        want = _loop(p, members, 0.0, st_e)
        for a, b in zip(r, want[:4]):
            assert torch.equal(a, b)
    assert torch.equal(st_g, st_e)
