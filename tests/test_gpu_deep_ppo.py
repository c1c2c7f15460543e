"""
The fused PPO epoch gradient of the deep actor-critic MLP
(swarm_ppo_deep_epoch_grad, csrc/swarm_deep.cuh) against torch autograd of
ProximalPolicyLoss._calculate_loss on the same fp32 parameters and samples.

Tolerance: the criteria of tests/test_gpu_ppo.py -- each parameter tensor's
gradient in norm, |g_fused - g_torch| <= 2e-4 |g_torch| (+1e-6), and
elementwise within 2e-3 of the tensor's largest entry (+1e-6).  On the CPU,
at all seven shapes, torch fp32 against fp64 autograd deviates at most 6e-7
relative in norm and in max, so the reference alone is about 300x inside.
Nothing is excluded from the comparison.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(2, 1, 2, 4, (16, 16)),
         (3, 64, 2, 4, (16, 16)),
         (7, 333, 10, 3, (100, 60)),
         (20, 1000, 1, 4, (128, 128)),
         (5, 517, 32, 16, (128, 128, 128)),
         (40, 150, 2, 4, (128, 128)),       # T > 32: the GAE kernel's uncached loop
         (3, 200, 3, 4, (12, 12, 12))]
# The (K, L3) template cell of the host's variant ladder that CASES lacks:
# the 16-action kernel with two hidden layers (CASES has K = 4 with two and
# with three layers and K = 16 with three); 210 samples, ragged widths.
LADDER_CASES = [(3, 70, 4, 6, (40, 24))]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _episode(T, S, d, k, hidden, seed):
    """tests/test_gpu_ppo._episode for the deep network."""
    from swarmrl_amd.networks.torch_network import DeepActorCriticMLP

    g = torch.Generator().manual_seed(seed)
    dev = torch.device("cuda", 0)
    torch.manual_seed(seed)
    net = DeepActorCriticMLP(d, n_actions=k, hidden=hidden).to(dev)
    x = torch.randn(T, S, d, generator=g).to(dev)
    actions = torch.randint(0, k, (T, S), generator=g).to(dev)
    rewards = torch.randn(T, S, generator=g).to(dev)
    with torch.no_grad():
        logits, _ = net(x)
        logp = torch.log(torch.softmax(logits, -1) + 1e-8).gather(-1, actions[..., None])[..., 0]
    # old policy off by up to ~e^0.4: ratios on both sides of the clip range
    old = (logp + 0.4 * torch.randn(T, S, generator=g).to(dev)).contiguous()
    return net, x, actions, old, rewards


def _flat_layers(net):
    ws, bs, wa, ba, wc, bc = net.deep_layers()
    return (*(t for pair in zip(ws, bs) for t in pair), wa, ba, wc, bc)


class _Wrap:
    def __init__(self, net):
        self.net = net

    def __call__(self, features, obs_ndim=1):
        lead = features.shape[: features.ndim - obs_ndim]
        return self.net(features.reshape(*lead, -1))


def _torch_grads(loss, net, x, actions, old, rewards):
    net.zero_grad(set_to_none=True)
    loss._calculate_loss(_Wrap(net), x, actions, rewards, old).backward()
    return [p.grad.detach().clone() for p in _flat_layers(net)]


def _fused_grads(loss, net, x, actions, old, rewards):
    from swarmrl_amd.engine import ops

    layers = _flat_layers(net)
    flat = ops.ppo_epoch_grad(x, actions, old, rewards, layers, loss.value_function.gamma,
                              loss.value_function.lambda_, loss.epsilon,
                              loss.entropy_coefficient)
    out, off = [], 0
    for t in layers:
        out.append(flat[off:off + t.numel()].view_as(t))
        off += t.numel()
    assert off == flat.numel()
    return out, flat


@pytest.mark.parametrize("T,S,d,k,hidden", CASES + LADDER_CASES)
def test_deep_epoch_grad_matches_autograd(T, S, d, k, hidden):
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    loss = ProximalPolicyLoss()
    net, x, actions, old, rewards = _episode(T, S, d, k, hidden, seed=T * 1000 + S)
    want = _torch_grads(loss, net, x, actions, old, rewards)
    got, _ = _fused_grads(loss, net, x, actions, old, rewards)
    assert len(got) == len(want) == 2 * len(hidden) + 4
    names = [f"{n}{l + 1}" for l in range(len(hidden)) for n in ("W", "b")] + \
        ["Wa", "ba", "Wc", "bc"]
    for name, a, b in zip(names, got, want):
        err, ref = (a - b).norm().item(), b.norm().item()
        emax, rmax = (a - b).abs().max().item(), b.abs().max().item()
        print(f"{name}: norm err {err:.3e} of {ref:.3e}, max err {emax:.3e} of {rmax:.3e}")
        assert err <= 2e-4 * ref + 1e-6, (name, err, ref)
        assert emax <= 2e-3 * rmax + 1e-6, (name, emax, rmax)


def test_deep_epoch_grad_deterministic():
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    loss = ProximalPolicyLoss()
    # 40 000 samples: 625 tiles over 256 blocks, several tiles per block
    net, x, actions, old, rewards = _episode(20, 2000, 3, 4, (128, 128), seed=5)
    _, a = _fused_grads(loss, net, x, actions, old, rewards)
    _, b = _fused_grads(loss, net, x, actions, old, rewards)
    assert torch.equal(a, b)
    want = _torch_grads(loss, net, x, actions, old, rewards)
    got = torch.cat([t.reshape(-1) for t in want])
    assert (a - got).norm().item() <= 2e-4 * got.norm().item() + 1e-6


def test_deep_compute_loss_fused_equals_torch_path(monkeypatch):
    """Two epochs of compute_loss with SGD: the fused deep path and the torch
    path end on the same parameters (1e-3 in norm), and _fused_layers is not
    None exactly when SWARMRL_AMD_FUSED_DEEP is on."""
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss
    from swarmrl_amd.networks.torch_network import DeepActorCriticMLP, TorchModel

    dev = torch.device("cuda", 0)
    T, E, A, d = 20, 2, 500, 3
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(T, E, A, d, generator=g)
    acts = torch.randint(0, 4, (T, E, A), generator=g)
    rews = torch.randn(T, E, A, generator=g)
    olp = -1.386 + 0.3 * torch.randn(T, E, A, generator=g)

    class Episode:
        features = [f.to(dev) for f in feats]
        actions = [a.to(dev) for a in acts]
        rewards = [r.to(dev) for r in rews]
        log_probs = [lp.to(dev) for lp in olp]

    steps = []
    for fused in ("1", "0"):
        monkeypatch.setenv("SWARMRL_AMD_FUSED_DEEP", fused)
        torch.manual_seed(0)
        model = TorchModel(DeepActorCriticMLP(d, 4, (64, 48)), input_shape=(d,), device=dev,
                           optimizer=lambda ps: torch.optim.SGD(ps, lr=1e-4))
        before = [p.detach().clone() for p in _flat_layers(model.model)]
        loss = ProximalPolicyLoss(n_epochs=2)
        layers = loss._fused_layers(model, feats.reshape(T, E * A, d).to(dev),
                                    acts.reshape(T, E * A))
        assert (layers is not None) == (fused == "1")
        if layers is not None:
            assert len(layers) == 8
            assert all(a is b for a, b in zip(layers, _flat_layers(model.model)))
        loss.compute_loss(model, Episode())
        steps.append([p.detach() - b for p, b in zip(_flat_layers(model.model), before)])
    for a, b in zip(*steps):
        # SGD: the parameter change is lr x the summed gradients of the two epochs
        assert (a - b).norm().item() <= 1e-3 * b.norm().item() + 1e-7


def test_deep_graph_epochs_equal_eager(monkeypatch):
    """Three episodes of compute_loss with the default capturable Adam: the
    captured-graph epochs (episode 1 eager, 2 captured + replayed, 3
    replayed; gradient kernels + the optimizer's own step per epoch) end on
    bit-identical parameters to the eager loop."""
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss
    from swarmrl_amd.networks.torch_network import DeepActorCriticMLP, TorchModel

    dev = torch.device("cuda", 0)
    T, E, A, d = 20, 1, 300, 4

    def episode(seed):
        g = torch.Generator().manual_seed(seed)

        class Episode:
            features = [f.to(dev) for f in torch.randn(T, E, A, d, generator=g)]
            actions = [a.to(dev) for a in torch.randint(0, 4, (T, E, A), generator=g)]
            rewards = [r.to(dev) for r in torch.randn(T, E, A, generator=g)]
            log_probs = [lp.to(dev) for lp in -1.386 + 0.3 * torch.randn(T, E, A, generator=g)]
        return Episode()

    finals = []
    for graph in ("1", "0"):
        monkeypatch.setenv("SWARMRL_AMD_PPO_GRAPH", graph)
        torch.manual_seed(0)
        model = TorchModel(DeepActorCriticMLP(d, 4, (32, 32, 32)), input_shape=(d,), device=dev)
        loss = ProximalPolicyLoss(n_epochs=5)
        for ep in range(3):
            loss.compute_loss(model, episode(100 + ep))
        assert (getattr(loss, "_ppo_graph", None) is not None) == (graph == "1")
        assert model.epoch_count == 15
        finals.append([p.detach().clone() for p in _flat_layers(model.model)])
    for a, b in zip(*finals):
        assert torch.equal(a, b)


def test_deep_epoch_grad_rejects_sizes_beyond_its_limits():
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    loss = ProximalPolicyLoss()
    for d, k, hidden in [(2, 4, (8, 8, 8, 8)), (2, 4, (129, 16)), (33, 4, (16, 16)),
                         (2, 17, (16, 16))]:
        net, x, actions, old, rewards = _episode(2, 3, d, k, hidden, seed=1)
        with pytest.raises(Exception):
            _fused_grads(loss, net, x, actions, old, rewards)


def test_stock_network_keeps_the_stock_ppo_kernels():
    from swarmrl_amd.networks.torch_network import ActorCriticMLP, DeepActorCriticMLP, TorchModel

    dev = torch.device("cuda", 0)
    stock = TorchModel(ActorCriticMLP(3, 4, 32), input_shape=(3,), device=dev)
    layers = stock.ppo_layers(3)
    assert layers is not None and len(layers) == 6
    assert all(a is b for a, b in zip(layers, stock.model.ppo_layers()))
    deep = TorchModel(DeepActorCriticMLP(3, 4, (16, 16, 16)), input_shape=(3,), device=dev)
    layers = deep.ppo_layers(3)
    assert layers is not None and len(layers) == 10
    assert deep.ppo_layers(4) is None
    wide = TorchModel(DeepActorCriticMLP(3, 4, (129, 16)), input_shape=(3,), device=dev)
    assert wide.ppo_layers(3) is None and wide._deep_layers(3, 4) is None
