"""
The deep ensemble PPO epoch gradient (swarm_ppo_deep_ensemble_epoch_grad,
csrc/swarm_ensemble.cuh over csrc/swarm_deep.cuh) against its oracle: M calls
of the single-model deep gradient (ops.ppo_epoch_grad with 2 L + 4 layers) on
the members' data and their own, separately allocated networks.  The contract
is bit identity per member and tensor (every per-member decision -- GAE
variant, number of gradient blocks -- is taken from the member's own T * S),
so the comparisons are torch.equal.  One case is also compared with torch
autograd of the loss's torch path, at the criteria of
tests/test_gpu_deep_ppo.py: per tensor 2e-4 in norm, 2e-3 of the largest
entry, + 1e-6 each; nothing is excluded.
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


def _names(hidden):
    return [f"{n}{l + 1}" for l in range(len(hidden)) for n in ("W", "b")] + \
        ["Wa", "ba", "Wc", "bc"]


def _flat_layers(net):
    ws, bs, wa, ba, wc, bc = net.deep_layers()
    return (*(t for pair in zip(ws, bs) for t in pair), wa, ba, wc, bc)


def _member_episode(T, S, d, k, hidden, seed):
    """One member's network and episode, as tests/test_gpu_deep_ppo.py::_episode."""
    from swarmrl_amd.networks.torch_network import DeepActorCriticMLP

    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = DeepActorCriticMLP(d, n_actions=k, hidden=hidden).to(DEV)
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
    from swarmrl_amd.networks import EnsembleDeepActorCriticMLP

    parts = [_member_episode(T, S, d, k, hidden, seed=1000 * T + S + 17 * m) for m in range(M)]
    ens = EnsembleDeepActorCriticMLP.from_members([p[0] for p in parts]).to(DEV)
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


@pytest.mark.parametrize("M,T,S,d,k,hidden", [
    (3, 2, 1, 2, 4, (16, 16)),               # the smallest case
    (2, 3, 64, 2, 4, (16, 16)),              # 192 samples: three full tiles, none ragged
    (3, 7, 37, 3, 3, (13, 7)),               # unaligned slices, ragged tiles
    (2, 40, 50, 2, 4, (128, 128)),           # T > 32: the GAE kernel's uncached loop
    (2, 5, 517, 32, 16, (128, 128, 128)),    # the limits, K = 16, three layers
    (2, 20, 900, 3, 4, (128, 128)),          # 282 tiles over 256 blocks: several tiles per block
    (2, 3, 70, 3, 3, (20, 12, 16)),          # the K = 4 kernel with three layers
    (2, 3, 70, 4, 6, (40, 24)),              # the K = 16 kernel with two layers
])
def test_ensemble_grad_equals_member_calls(M, T, S, d, k, hidden):
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    hp = _hyper(ProximalPolicyLoss())
    ens, x, actions, old, rewards, parts = _ensemble_episode(M, T, S, d, k, hidden)
    layers = ens.ppo_layers()
    assert len(layers) == 2 * len(hidden) + 4
    flat = ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, layers, *hp)
    assert flat.numel() == ops.ppo_ensemble_grad_size(M, d, hidden, k)
    got = _split(flat, layers)
    for m, (net, xm, am, om, rm) in enumerate(parts):
        single = _flat_layers(net)
        want = _split(ops.ppo_epoch_grad(xm, am, om, rm, single, *hp), single)
        for name, a, b in zip(_names(hidden), got, want):
            assert torch.equal(a[m], b), (m, name, (a[m] - b).abs().max().item())
    assert not torch.equal(got[0][0], got[0][1])  # the members learn different things


def test_ensemble_grad_matches_autograd_of_the_torch_path():
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.ensemble_ppo_loss import EnsembleProximalPolicyLoss
    from swarmrl_amd.networks import EnsembleTorchModel

    M, T, S, d, k, hidden = 2, 7, 333, 10, 3, (100, 60)
    ens, x, actions, old, rewards, _ = _ensemble_episode(M, T, S, d, k, hidden)
    loss = EnsembleProximalPolicyLoss()
    model = EnsembleTorchModel(ens, device=DEV)
    layers = ens.ppo_layers()
    assert model.ppo_layers(d) is not None and model.ppo_layers(d + 1) is None
    loss._ensemble_loss(model, x, actions, rewards, old).backward()
    want = [p.grad.detach().clone() for p in layers]
    got = _split(ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, layers, *_hyper(loss)),
                 layers)
    for m in range(M):  # tests/test_gpu_deep_ppo.py's criteria, per member
        for name, a, b in zip(_names(hidden), got, want):
            a, b = a[m], b[m]
            err, ref = (a - b).norm().item(), b.norm().item()
            emax, rmax = (a - b).abs().max().item(), b.abs().max().item()
            print(f"member {m} {name}: norm err {err:.3e} of {ref:.3e}, "
                  f"max err {emax:.3e} of {rmax:.3e}")
            assert err <= 2e-4 * ref + 1e-6, (m, name, err, ref)
            assert emax <= 2e-3 * rmax + 1e-6, (m, name, emax, rmax)


def test_ensemble_grad_deterministic():
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    hp = _hyper(ProximalPolicyLoss())
    ens, x, actions, old, rewards, _ = _ensemble_episode(3, 20, 900, 1, 4, (128, 128))
    a = ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, ens.ppo_layers(), *hp)
    b = ops.ppo_ensemble_epoch_grad(x, actions, old, rewards, ens.ppo_layers(), *hp)
    assert torch.equal(a, b)


def test_wrong_workspace_size_is_rejected():
    from swarmrl_amd.engine import ops
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    hp = _hyper(ProximalPolicyLoss())
    M, T, S, d, k, hidden = 3, 5, 37, 3, 4, (32, 16)
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
    torch.cuda.synchronize()
    assert bool((grad != -7.0).all())
    for bad in [(1025, d, hidden, k), (M, d, (129, 16), k), (M, d, (16,), k),
                (M, d, (8, 8, 8, 8), k), (M, 33, hidden, k), (M, d, hidden, 17)]:
        with pytest.raises(ValueError):  # beyond the limits: no size at all
            ops.ppo_ensemble_workspace_bytes(bad[0], T, S, bad[1], bad[2], bad[3])


def test_grouped_workspace_is_sized_by_the_blocks_launched():
    """64 small deep members: every member's partial rows are the blocks it
    launches, and the slices are packed -- below 64 single deep workspaces."""
    import ctypes

    from swarmrl_amd import _capi
    from swarmrl_amd.engine import ops

    T, S, d, k, hidden = 5, 37, 3, 4, (128, 128)
    widths = (ctypes.c_int32 * 2)(*hidden)
    single = int(_capi.lib().swarm_ppo_deep_workspace_bytes(
        T, S, d, 2, ctypes.cast(widths, ctypes.c_void_p), k))
    grouped = ops.ppo_ensemble_workspace_bytes(64, T, S, d, hidden, k)
    assert 0 < grouped < 64 * single
    # 3 tiles of 64 samples: 3 partial rows per member, not kDeepPpoBlocks = 256
    row = 4 * (ops.ppo_ensemble_grad_size(1, d, hidden, k))
    assert grouped < 64 * 4 * row
