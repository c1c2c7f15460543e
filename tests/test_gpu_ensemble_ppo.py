"""
The ensemble PPO epoch gradient (swarm_ppo_ensemble_epoch_grad,
csrc/swarm_ensemble.cuh) against its oracle: M calls of the single-model
gradient (ops.ppo_epoch_grad) on the members' data and weights.  The contract
is bit identity per member and tensor (every per-member decision -- kernel
variants, number of gradient blocks -- is taken from the member's own T * S),
so the comparisons are torch.equal.  One case is also compared with torch
autograd of the loss's torch path, at the criteria of tests/test_gpu_ppo.py.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAMES = ("W1", "b1", "Wa", "ba", "Wc", "bc")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _member_episode(T, S, d, k, hidden, seed):
    """One member's network and episode, as tests/test_gpu_ppo.py::_episode."""
    from swarmrl_amd.networks.torch_network import ActorCriticMLP

    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = ActorCriticMLP(d, n_actions=k, hidden=hidden).to(DEV)
    x = torch.randn(T, S, d, generator=g).to(DEV)
    actions = torch.randint(0, k, (T, S), generator=g).to(DEV)
    rewards = torch.randn(T, S, generator=g).to(DEV)
    with torch.no_grad():
        logits, _ = net(x)
        logp = torch.log(torch.softmax(logits, -1) + 1e-8).gather(-1, actions[..., None])[..., 0]
    old = (logp + 0.4 * torch.randn(T, S, generator=g).to(DEV)).contiguous()
    return net, x, actions, old, rewards


def _ensemble_episode(M, T, S, d, k, hidden):
    """(stacked network, member-major x, actions, old_logp, rewards, members)."""
    from swarmrl_amd.networks.ensemble_network import EnsembleActorCriticMLP

    parts = [_member_episode(T, S, d, k, hidden, seed=1000 * T + S + 17 * m) for m in range(M)]
    ens = EnsembleActorCriticMLP.from_members([p[0] for p in parts]).to(DEV)
    data = tuple(torch.stack([p[i] for p in parts]).contiguous() for i in range(1, 5))
    return (ens, *data, parts)


def _hyper(loss):
    return (loss.value_function.gamma, loss.value_function.lambda_, loss.epsilon,
            loss.entropy_coefficient)


def _split(flat, layers):
    out, off = [], 0
    for t in layers:
        out.append(flat[off:off + t.numel()].view_as(t))
        off += t.numel()
    assert off == flat.numel()
    return out


# tests/test_gpu_ppo.py::LADDER_CELLS for two members: every (D, K) template
# arm of the host's variant ladder with one and with two unit waves.
LADDER_DK = [(1, 3), (3, 4), (4, 6), (10, 4), (16, 16), (20, 2), (32, 16)]
LADDER_CELLS = [(2, 3, 70, d, k, hidden) for hidden in (100, 160) for d, k in LADDER_DK]


@pytest.mark.parametrize("M,T,S,d,k,hidden", [
    (3, 5, 37, 3, 4, 128),      # coop: the waves of a block share each tile
    (2, 40, 50, 2, 4, 128),     # T > 32: the GAE kernel's uncached loop
    (2, 7, 333, 10, 3, 100),    # ragged hidden
    (2, 5, 129, 32, 6, 256),    # two unit waves
    (2, 20, 53000, 4, 4, 128),  # >= 2^20 samples a member: packed values, non-coop grads
    *LADDER_CELLS,
])
def test_ensemble_grad_equals_member_calls(M, T, S, d, k, hidden):
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    hp = _hyper(ProximalPolicyLoss())
    ens, x, actions, old, rewards, parts = _ensemble_episode(M, T, S, d, k, hidden)
    layers = ens.ppo_layers()
    got = _split(ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, layers, *hp), layers)
    for m, (net, xm, am, om, rm) in enumerate(parts):
        single = net.ppo_layers()
        want = _split(ops.ppo_epoch_grad(xm, am, om, rm, single, *hp), single)
        for name, a, b in zip(NAMES, got, want):
            assert torch.equal(a[m], b), (m, name)


def test_ensemble_grad_matches_autograd_of_the_torch_path():
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.ensemble_ppo_loss import EnsembleProximalPolicyLoss
    from swarmrl_amd.networks.ensemble_network import EnsembleTorchModel

    M, T, S, d, k, hidden = 2, 7, 333, 10, 3, 100
    ens, x, actions, old, rewards, _ = _ensemble_episode(M, T, S, d, k, hidden)
    loss = EnsembleProximalPolicyLoss()
    model = EnsembleTorchModel(ens, device=DEV)
    layers = ens.ppo_layers()
    loss._ensemble_loss(model, x, actions, rewards, old).backward()
    want = [p.grad.detach().clone() for p in layers]
    got = _split(ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, layers, *_hyper(loss)),
                 layers)
    for m in range(M):  # tests/test_gpu_ppo.py::_check, per member
        for name, a, b in zip(NAMES, got, want):
            a, b = a[m], b[m]
            err = (a - b).norm().item()
            assert err <= 2e-4 * b.norm().item() + 1e-6, (m, name, err, b.norm().item())
            assert (a - b).abs().max().item() <= 2e-3 * b.abs().max().item() + 1e-6, (m, name)


def test_ensemble_grad_deterministic():
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    hp = _hyper(ProximalPolicyLoss())
    ens, x, actions, old, rewards, _ = _ensemble_episode(3, 20, 2000, 1, 4, 128)
    a = ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, ens.ppo_layers(), *hp)
    b = ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, ens.ppo_layers(), *hp)
    assert torch.equal(a, b)


def test_wrong_workspace_size_is_rejected():
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    hp = _hyper(ProximalPolicyLoss())
    M, T, S, d, k, hidden = 3, 5, 37, 3, 4, 128
    ens, x, actions, old, rewards, _ = _ensemble_episode(M, T, S, d, k, hidden)
    need = ops.ppo_ensemble_workspace_bytes(M, T, S, d, hidden, k)
    small = torch.zeros(need - 256, dtype=torch.uint8, device=DEV)
    grad = torch.full((ops.ppo_ensemble_grad_size(M, d, hidden, k),), -7.0, device=DEV)
    with pytest.raises(ValueError):
        ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, ens.ppo_layers(), *hp, out=grad,
                                    workspace=small)
    torch.cuda.synchronize()
    assert bool((grad == -7.0).all())  # nothing was launched
    exact = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, ens.ppo_layers(), *hp, out=grad,
                                workspace=exact)
    with pytest.raises(ValueError):  # beyond the limits: no size at all
        ops.ppo_ensemble_workspace_bytes(1025, T, S, d, hidden, k)


def test_grouped_workspace_is_sized_by_the_blocks_launched():
    """64 small members: their partial rows are the blocks each launches, not
    64 x the single workspace's kPpoBlocks rows."""
    from swarmrl_amd import _capi
    from swarmrl_amd.engine import ops

    T, S, d, k, hidden = 5, 37, 3, 4, 128
    single = int(_capi.lib().swarm_ppo_workspace_bytes(T, S, d, hidden, k))
    grouped = ops.ppo_ensemble_workspace_bytes(64, T, S, d, hidden, k)
    assert 0 < grouped < 64 * single
    assert grouped < 8 * single  # far below: the single workspace is ~all partial rows
