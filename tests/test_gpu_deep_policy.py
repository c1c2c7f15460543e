"""
The rollout policy of a deep actor-critic MLP in one launch
(swarm_policy_deep_sample, csrc/swarm_deep.cuh): logits against the torch
module, the sampling tail bit for bit against swarm_sample_actions on the
kernel's own logits, an exact-integer check of the matrix-instruction lane
maps and the zero padding, and the agent's dispatch.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(1, 3, (16, 16), 4),             # less than one tile
         (65, 3, (128, 128), 4),          # crosses a counter group, ends in a partial tile
         (1000, 9, (100, 60), 6),         # ragged and unequal widths
         (4096, 3, (128, 128, 128), 4),
         (333, 32, (12, 12, 12), 16)]     # the reference's 3 x 12 net at the d_in and k limits


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _tables(dev):
    return (torch.tensor([0.0, 10.0, 0.0, 0.0], device=dev),
            torch.tensor([10.0, 0.0, -10.0, 0.0], device=dev))


@pytest.mark.parametrize("n,d_in,hidden,k", CASES)
def test_deep_policy_matches_torch_and_sampler(n, d_in, hidden, k):
    """Logits within rtol 1e-5, atol 1e-5 of the torch module (torch fp32 and
    a k-ordered fp32 chain both stay within 4e-7 of fp64 at these shapes;
    outputs are O(1)); actions and log-probs bit-identical to
    swarm_sample_actions on the kernel's own logits with the same counters;
    the table outputs; counters advance by exactly one."""
    from swarmrl_amd.engine import ops
    from swarmrl_amd.networks import DeepActorCriticMLP

    dev = torch.device("cuda", 0)
    torch.manual_seed(n + d_in)
    net = DeepActorCriticMLP(d_in, k, hidden).to(dev)
    obs = torch.randn(n, d_in, device=dev) * 3.0
    ftab = torch.arange(k, dtype=torch.float32, device=dev) * 2.0
    ttab = -torch.arange(k, dtype=torch.float32, device=dev)
    state = ops.counter_state(None, n, dev)
    state += 5
    ref_state = state.clone()
    ws, bs, wa, ba, _, _ = net.deep_layers()
    with torch.no_grad():
        idx, logp, f, t, lg = ops.policy_deep_sample(obs, ws, bs, wa, ba, 99, state, 0.0, ftab,
                                                     ttab, want_logits=True)
        ref_logits, _ = net(obs)
    torch.testing.assert_close(lg, ref_logits, rtol=1e-5, atol=1e-5)
    i2, lp2, f2, t2 = ops.sample_actions(lg, 99, ref_state, 0.0, ftab, ttab)
    assert torch.equal(idx, i2) and torch.equal(logp, lp2)
    assert torch.equal(f, ftab[idx]) and torch.equal(t, ttab[idx])
    assert torch.equal(state, ref_state) and bool((state == 6).all())


@pytest.mark.parametrize("hidden", [(16, 16), (100, 60), (128, 128, 128)])
def test_deep_policy_exact_integer_layout(hidden):
    """d_in = 3, observations in {-2..2}, every weight and bias in {-1, 0, 1}:
    every intermediate is an integer below 2^24 (worst case (128, 128, 128):
    |logit| <= 128 * 114 817 + 1 < 2^24), so the logits must equal the fp64
    evaluation exactly -- any operand lane-map or padding mistake shows
    deterministically (the random weights are asymmetric)."""
    from swarmrl_amd.engine import ops
    from swarmrl_amd.networks import DeepActorCriticMLP

    dev = torch.device("cuda", 0)
    n, d_in, k = 200, 3, 4
    gen = torch.Generator().manual_seed(sum(hidden))
    net = DeepActorCriticMLP(d_in, k, hidden)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randint(-1, 2, p.shape, generator=gen).float())
    obs = torch.randint(-2, 3, (n, d_in), generator=gen).float()
    with torch.no_grad():
        ref = net.double().logits(obs.double())
    assert float(ref.abs().max()) < 2.0 ** 24 and float(ref.abs().max()) > 0
    net = net.float().to(dev)
    ftab, ttab = _tables(dev)
    state = ops.counter_state(None, n, dev)
    ws, bs, wa, ba, _, _ = net.deep_layers()
    lg = ops.policy_deep_sample(obs.to(dev), ws, bs, wa, ba, 3, state, 0.0, ftab, ttab,
                                want_logits=True)[4]
    assert torch.equal(lg.cpu().double(), ref)


def test_deep_policy_exploration_probability_one_is_uniform():
    from swarmrl_amd.engine import ops
    from swarmrl_amd.networks import DeepActorCriticMLP

    dev = torch.device("cuda", 0)
    n = 200_000
    torch.manual_seed(1)
    net = DeepActorCriticMLP(3, 4, (16, 16)).to(dev)
    with torch.no_grad():
        net.actor.bias.copy_(torch.tensor([60.0, 0.0, 0.0, 0.0]))
        net.actor.weight.zero_()
    obs = torch.randn(n, 3, device=dev)
    ftab, ttab = _tables(dev)
    state = ops.counter_state(None, n, dev)
    ws, bs, wa, ba, _, _ = net.deep_layers()
    idx0 = ops.policy_deep_sample(obs, ws, bs, wa, ba, 5, state, 0.0, ftab, ttab)[0]
    assert bool((idx0 == 0).all())
    idx1 = ops.policy_deep_sample(obs, ws, bs, wa, ba, 5, state, 1.0, ftab, ttab)[0]
    freq = torch.bincount(idx1, minlength=4).double().cpu().numpy() / n
    assert np.all(np.abs(freq - 0.25) < 0.01), freq


def test_deep_policy_rejects_sizes_beyond_its_limits():
    """Outside 2 <= layers <= 3, width <= 128, d_in <= 32, k <= 16 the entry
    point returns an error and launches nothing."""
    from swarmrl_amd.engine import ops
    from swarmrl_amd.networks import DeepActorCriticMLP

    dev = torch.device("cuda", 0)
    for d_in, k, hidden in [(3, 4, (16,)), (3, 4, (8, 8, 8, 8)), (3, 4, (129, 16)),
                            (33, 4, (16, 16)), (3, 17, (16, 16))]:
        net = DeepActorCriticMLP(d_in, k, hidden).to(dev)
        obs = torch.zeros(10, d_in, device=dev)
        tab = torch.zeros(k, device=dev)
        state = ops.counter_state(None, 10, dev)
        ws, bs, wa, ba, _, _ = net.deep_layers()
        with pytest.raises(Exception):
            ops.policy_deep_sample(obs, ws, bs, wa, ba, 1, state, 0.0, tab, tab)
        assert bool((state == 0).all())


def test_stock_network_keeps_the_stock_kernels():
    """The deep path changes nothing for ActorCriticMLP, and the stock gates
    decline the deep class."""
    from swarmrl_amd.networks import ActorCriticMLP, DeepActorCriticMLP, TorchModel

    dev = torch.device("cuda", 0)
    stock = TorchModel(ActorCriticMLP(3, 4, 32), input_shape=(3,), device=dev)
    assert stock._mlp_layers(3, 4) is not None
    assert stock.fused_policy_args(64, 3, 4, dev) is not None
    assert stock._deep_layers(3, 4) is None
    deep = TorchModel(DeepActorCriticMLP(3, 4, (16, 16)), input_shape=(3,), device=dev)
    assert deep._mlp_layers(3, 4) is None
    assert deep.fused_policy_args(64, 3, 4, dev) is None
    assert deep._deep_layers(3, 4) is not None
    assert deep._deep_layers(4, 4) is None and deep._deep_layers(3, 5) is None


def test_agent_takes_the_deep_kernel_and_replays_fresh_draws(tmp_path, monkeypatch):
    """ActorCriticAgent.calc_action on a SwarmEngine view runs the deep
    network through ops.policy_deep_sample (not the torch fallback), the
    switch SWARMRL_AMD_FUSED_DEEP=0 turns it off, and under a captured HIP
    graph two replays draw different actions."""
    from swarmrl_amd.actions import Action
    from swarmrl_amd.agents import ActorCriticAgent
    from swarmrl_amd.engine import MDParams, SwarmEngine, ops
    from swarmrl_amd.networks import DeepActorCriticMLP, TorchModel
    from swarmrl_amd.observables import SubdividedVisionCones
    from swarmrl_amd.tasks.searching import GradientSensing
    from swarmrl_amd.units import UnitRegistry

    dev = torch.device("cuda", 0)
    ureg = UnitRegistry()
    n, L = 64, 60.0
    p = MDParams(ureg=ureg, box_length=ureg.Quantity([L, L, L], "micrometer"))
    eng = SwarmEngine(p, n_dims=2, seed=5, out_folder=tmp_path)
    eng.add_colloids(n, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(np.array([L / 2, L / 2, 0.0]), "micrometer"),
                     ureg.Quantity(25.0, "micrometer"), type_colloid=0)
    eng.integrate(1)
    torch.manual_seed(0)
    net = TorchModel(DeepActorCriticMLP(3, 4, (16, 16)), input_shape=(3,), device=dev)
    assert net._deep_layers(3, 4) is not None
    actions = {"a": Action(torque=np.array([0, 0, 10.0])), "b": Action(force=10.0),
               "c": Action(torque=np.array([0, 0, -10.0])), "d": Action()}
    agent = ActorCriticAgent(
        0, net, GradientSensing(np.array([L / 2, L / 2, 0]), lambda d: 1 - d,
                                np.array([L, L, L]), 10),
        SubdividedVisionCones(10.0, np.pi / 2, 3, [1.0] * n), actions)
    calls = []
    real = ops.policy_deep_sample
    monkeypatch.setattr(ops, "policy_deep_sample",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    chosen = agent.calc_action(eng.swarm_view())
    assert len(calls) == 1
    idx = agent.trajectory.actions[-1]
    ftab, ttab = agent._action_tables(dev)[1:3]
    assert torch.equal(chosen.f_swim, ftab[idx]) and torch.equal(chosen.torque_z, ttab[idx])
    monkeypatch.setenv("SWARMRL_AMD_FUSED_DEEP", "0")
    assert net._deep_layers(3, 4) is None
    agent.calc_action(eng.swarm_view())
    assert len(calls) == 1
    monkeypatch.setenv("SWARMRL_AMD_FUSED_DEEP", "1")

    obs = agent.trajectory.features[-1].reshape(n, -1).float().contiguous()
    out = {}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net.compute_action_fused(obs, ftab, ttab)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        out["r"] = net.compute_action_fused(obs, ftab, ttab)
    assert len(calls) == 3
    g.replay()
    first = out["r"][0].clone()
    g.replay()
    assert not torch.equal(first, out["r"][0])
    logits = net.model.logits(obs)
    ref = torch.log(torch.softmax(logits, -1) + 1e-8).gather(1, out["r"][0][:, None])[:, 0]
    assert torch.allclose(out["r"][1], ref, atol=1e-5)
