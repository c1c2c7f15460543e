"""
The deep ensemble (EnsembleDeepActorCriticMLP) without a GPU: the stacked
network against its DeepActorCriticMLP members, the member round trips,
single-member export, the torch path of EnsembleProximalPolicyLoss against
ProximalPolicyLoss on each member's slice, and select_members (the gather of
a genetic selection) against sequential copy_member.
"""

import os

import pytest
import torch

from swarmrl_amd.losses import EnsembleProximalPolicyLoss, ProximalPolicyLoss
from swarmrl_amd.networks import (DeepActorCriticMLP, EnsembleActorCriticMLP,
                                  EnsembleDeepActorCriticMLP, EnsembleTorchModel, TorchModel)

CPU = torch.device("cpu")
M, D, K, HIDDEN = 3, 3, 4, (16, 12)
NAMES = ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias", "actor.weight",
         "actor.bias", "critic.weight", "critic.bias")


def _layers(net: DeepActorCriticMLP):
    ws, bs, wa, ba, wc, bc = net.deep_layers()
    return (*(t for pair in zip(ws, bs) for t in pair), wa, ba, wc, bc)


def test_members_are_initialised_as_deep_networks_constructed_in_order():
    for hidden in (HIDDEN, (8, 6, 5)):
        torch.manual_seed(3)
        ens = EnsembleDeepActorCriticMLP(M, D, K, hidden)
        torch.manual_seed(3)
        nets = [DeepActorCriticMLP(D, K, hidden) for _ in range(M)]
        assert len(ens.ppo_layers()) == 2 * len(hidden) + 4
        for m, net in enumerate(nets):
            for a, b in zip(ens.ppo_layers(), _layers(net)):
                assert torch.equal(a[m], b)
    assert [tuple(p.shape) for p in ens.ppo_layers()] == [
        (M, 8, D), (M, 8), (M, 6, 8), (M, 6), (M, 5, 6), (M, 5), (M, K, 5), (M, K), (M, 1, 5),
        (M, 1)]
    # the optimizer sees the parameters in the gradient's order
    assert [id(p) for p in ens.parameters()] == [id(p) for p in ens.ppo_layers()]
    ws, bs, wa, ba = ens.rollout_layers()
    assert [id(t) for t in (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], wa, ba)] == \
        [id(p) for p in ens.ppo_layers()[:8]]


def test_forward_equals_each_members_forward():
    """The criteria of tests/test_ensemble_cpu.py::
    test_forward_equals_each_members_forward: torch.equal at 32 rows per
    member (every product runs torch's GEMM in both the batched and the
    single form), fp32 rounding at 5 rows."""
    torch.manual_seed(0)
    ens = EnsembleDeepActorCriticMLP(M, D, K, (16, 16))
    x = torch.randn(M, 32, D)
    logits, values = ens(x)
    assert logits.shape == (M, 32, K) and values.shape == (M, 32, 1)
    for m in range(M):
        lm, vm = ens.member(m)(x[m])
        assert torch.equal(logits[m], lm) and torch.equal(values[m], vm)
    x = torch.randn(M, 5, D)
    logits, values = ens(x)
    for m in range(M):
        lm, vm = ens.member(m)(x[m])
        torch.testing.assert_close(logits[m], lm, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(values[m], vm, rtol=1e-5, atol=1e-6)


def test_from_members_member_and_set_member_round_trip():
    torch.manual_seed(1)
    nets = [DeepActorCriticMLP(D, K, HIDDEN) for _ in range(M)]
    ens = EnsembleDeepActorCriticMLP.from_members(nets)
    assert ens.n_members == M
    assert (ens.input_dim, ens.n_actions, ens.hidden_widths) == (D, K, HIDDEN)
    for m, net in enumerate(nets):
        copy = ens.member(m)
        assert isinstance(copy, DeepActorCriticMLP)
        for a, b in zip(_layers(copy), _layers(net)):
            assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    fresh = DeepActorCriticMLP(D, K, HIDDEN)
    ens.set_member(1, fresh)
    for a, b, c in zip(_layers(ens.member(1)), _layers(fresh), _layers(nets[1])):
        assert torch.equal(a, b) and not torch.equal(a, c)
    for a, b in zip(_layers(ens.member(0)), _layers(nets[0])):
        assert torch.equal(a, b)  # the other members are untouched
    with pytest.raises(ValueError):
        EnsembleDeepActorCriticMLP.from_members([nets[0], DeepActorCriticMLP(D, K, (16, 13))])
    sd = ens.member_state_dict(2)
    assert tuple(sd) == NAMES
    DeepActorCriticMLP(D, K, HIDDEN).load_state_dict(sd)  # strict: exactly the stock names
    torch.manual_seed(5)
    ens.reset_parameters()
    torch.manual_seed(5)
    again = [DeepActorCriticMLP(D, K, HIDDEN) for _ in range(M)]
    for m, net in enumerate(again):
        for a, b in zip(ens.ppo_layers(), _layers(net)):
            assert torch.equal(a[m], b)


def _trained_model(steps=2, seed=2):
    torch.manual_seed(seed)
    model = EnsembleTorchModel(EnsembleDeepActorCriticMLP(M, D, K, HIDDEN), device=CPU)
    x = torch.randn(M, 8, D)
    for _ in range(steps):
        logits, values = model.model(x)
        model.update_model((logits ** 2).sum() + values.sum())
    return model


def test_export_member_is_restored_by_a_stock_deep_model(tmp_path):
    model = _trained_model()
    for m in range(M):
        model.export_member(m, filename=f"m{m}", directory=os.fspath(tmp_path))
        stock = TorchModel(DeepActorCriticMLP(D, K, HIDDEN), device=CPU)
        stock.restore_model_state(f"m{m}", os.fspath(tmp_path))
        for a, b in zip(model.model.ppo_layers(), _layers(stock.model)):
            assert torch.equal(a[m], b)
        assert stock.epoch_count == model.epoch_count == 2
        for p, q in zip(model.model.ppo_layers(), _layers(stock.model)):  # Adam moments too
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(model.optimizer.state[p][key][m], stock.optimizer.state[q][key])
            assert float(stock.optimizer.state[q]["step"]) == 2.0
    model.export_model("all", os.fspath(tmp_path))
    other = EnsembleTorchModel(EnsembleDeepActorCriticMLP(M, D, K, HIDDEN), device=CPU)
    other.restore_model_state("all", os.fspath(tmp_path))
    for a, b in zip(model.model.ppo_layers(), other.model.ppo_layers()):
        assert torch.equal(a, b)


class _Wrap:
    def __init__(self, net):
        self.net = net

    def __call__(self, features, obs_ndim=1):
        lead = features.shape[: features.ndim - obs_ndim]
        return self.net(features.reshape(*lead, -1))


def test_torch_path_gives_each_member_its_own_ppo_gradient():
    """M = 2, T = 4, S = 6 on the CPU, the criteria of tests/test_ensemble_cpu.py::
    test_torch_path_gives_each_member_its_own_ppo_gradient: per tensor 2e-4 in
    norm, 2e-3 of the largest entry, + 1e-6 each."""
    members, T, S, d, k = 2, 4, 6, 3, 4
    g = torch.Generator().manual_seed(7)
    torch.manual_seed(7)
    ens = EnsembleDeepActorCriticMLP(members, d, k, HIDDEN)
    model = EnsembleTorchModel(ens, device=CPU)
    x = torch.randn(members, T, S, d, generator=g)
    actions = torch.randint(0, k, (members, T, S), generator=g)
    rewards = torch.randn(members, T, S, generator=g)
    old = -1.386 + 0.3 * torch.randn(members, T, S, generator=g)
    loss = EnsembleProximalPolicyLoss()
    loss._ensemble_loss(model, x, actions, rewards, old).backward()
    for m in range(members):
        net = ens.member(m)
        ProximalPolicyLoss()._calculate_loss(_Wrap(net), x[m], actions[m], rewards[m],
                                             old[m]).backward()
        for name, p, q in zip(NAMES, ens.ppo_layers(), _layers(net)):
            a, b = p.grad[m], q.grad
            err = (a - b).norm().item()
            assert err <= 2e-4 * b.norm().item() + 1e-6, (m, name, err, b.norm().item())
            assert (a - b).abs().max().item() <= 2e-3 * b.abs().max().item() + 1e-6, (m, name)


def test_select_members_gathers_where_sequential_copies_go_wrong():
    """parent_of = [1, 0, 0] on M = 3: members 0 and 1 swap and member 2
    becomes the OLD member 0.  copy_member(1, 0); copy_member(0, 1);
    copy_member(0, 2) overwrites member 0 before it is read, so members 1 and
    2 end as copies of the old member 1."""
    parent_of = [1, 0, 0]
    model, seq = _trained_model(), _trained_model()
    seeds = list(model.member_seeds)
    layers = model.model.ppo_layers()
    before = [p.detach().clone() for p in layers]
    moments = [{k: model.optimizer.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq")}
               for p in layers]
    pointers = [p.data_ptr() for p in layers]
    steps = [float(model.optimizer.state[p]["step"]) for p in layers]
    model.select_members(parent_of)
    for p, b, mom in zip(layers, before, moments):
        assert torch.equal(p.detach(), b[parent_of])
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(model.optimizer.state[p][key], mom[key][parent_of])
    assert [p.data_ptr() for p in layers] == pointers  # in place: a captured graph stays valid
    assert [float(model.optimizer.state[p]["step"]) for p in layers] == steps
    assert model.member_seeds == seeds  # seeds stay with the slot
    for dst, src in enumerate(parent_of):
        seq.copy_member(src, dst)
    w1, w1_seq = layers[0].detach(), seq.model.ppo_layers()[0].detach()
    assert torch.equal(before[0], _trained_model().model.ppo_layers()[0].detach())
    assert not torch.equal(w1_seq, w1)
    assert torch.equal(w1_seq[1], before[0][1]) and torch.equal(w1[1], before[0][0])
    # weights only: the moments stay
    kept = [model.optimizer.state[p]["exp_avg"].clone() for p in layers]
    now = [p.detach().clone() for p in layers]
    model.select_members([2, 2, 0], with_optimizer_state=False)
    for p, b, mom in zip(layers, now, kept):
        assert torch.equal(p.detach(), b[[2, 2, 0]])
        assert torch.equal(model.optimizer.state[p]["exp_avg"], mom)
    with pytest.raises(ValueError):
        model.select_members([0, 1])
    with pytest.raises(IndexError):
        model.select_members([0, 1, 3])


def test_select_members_serves_the_one_layer_ensemble_too():
    torch.manual_seed(4)
    model = EnsembleTorchModel(EnsembleActorCriticMLP(M, D, K, 8), device=CPU)
    before = [p.detach().clone() for p in model.model.ppo_layers()]
    model.select_members([2, 0, 1])
    for p, b in zip(model.model.ppo_layers(), before):
        assert torch.equal(p.detach(), b[[2, 0, 1]])
