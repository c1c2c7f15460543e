"""
DeepActorCriticMLP and its dispatch, without a GPU: the module against
hand-composed layers, the accessor's order, the gates (on the CPU every deep
network takes the torch path), training through torch autograd, checkpoints
and the size limits of the fused deep kernels.
"""

import ctypes

import pytest
import torch

from swarmrl_amd.networks import DeepActorCriticMLP, TorchModel
from swarmrl_amd.networks.torch_network import deep_mlp_within_limits


@pytest.mark.parametrize("hidden", [(16, 16), (12, 12, 12)])
def test_forward_equals_hand_composed_layers(hidden):
    torch.manual_seed(3)
    net = DeepActorCriticMLP(5, 4, hidden)
    x = torch.randn(37, 5)
    ws, bs, wa, ba, wc, bc = net.deep_layers()
    assert len(ws) == len(bs) == len(hidden)
    h = x
    for w, b in zip(ws, bs):
        h = torch.clamp(h @ w.t() + b, min=0.0)
    logits, value = net(x)
    assert logits.shape == (37, 4) and value.shape == (37, 1)
    torch.testing.assert_close(logits, h @ wa.t() + ba)
    torch.testing.assert_close(value, h @ wc.t() + bc)
    torch.testing.assert_close(net.logits(x), logits)


def test_deep_layers_order_and_layouts():
    net = DeepActorCriticMLP(3, 6, (10, 20, 30))
    ws, bs, wa, ba, wc, bc = net.deep_layers()
    assert [tuple(w.shape) for w in ws] == [(10, 3), (20, 10), (30, 20)]
    assert [tuple(b.shape) for b in bs] == [(10,), (20,), (30,)]
    assert all(w is m.weight and b is m.bias for w, b, m in zip(ws, bs, net.layers))
    assert wa is net.actor.weight and ba is net.actor.bias
    assert wc is net.critic.weight and bc is net.critic.bias
    assert tuple(wa.shape) == (6, 30) and tuple(wc.shape) == (1, 30)
    # every parameter, once
    flat = [*ws, *bs, wa, ba, wc, bc]
    assert {id(t) for t in flat} == {id(p) for p in net.parameters()}
    # the stock gates key on these names and must keep declining the class
    assert not hasattr(net, "rollout_layers") and not hasattr(net, "ppo_layers")


def test_cpu_model_takes_the_torch_path():
    model = TorchModel(DeepActorCriticMLP(3, 4, (16, 16)), input_shape=(3,), device="cpu")
    assert model._deep_layers(3, 4) is None
    assert model.ppo_layers(3) is None
    assert model._mlp_layers(3, 4) is None
    assert model.fused_policy_args(8, 3, 4, torch.device("cpu")) is None
    idx, logp = model.compute_action(torch.randn(8, 3))
    assert idx.shape == (8,) and logp.shape == (8,)


def test_compute_loss_on_cpu_trains_every_parameter():
    from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss

    torch.manual_seed(0)
    model = TorchModel(DeepActorCriticMLP(3, 4, (16, 16)), input_shape=(3,), device="cpu")
    before = [p.detach().clone() for p in model.model.parameters()]
    T, A = 6, 50
    g = torch.Generator().manual_seed(1)

    class Episode:
        features = list(torch.randn(T, A, 3, generator=g))
        actions = list(torch.randint(0, 4, (T, A), generator=g))
        rewards = list(torch.randn(T, A, generator=g))
        log_probs = list(-1.386 + 0.3 * torch.randn(T, A, generator=g))

    loss = ProximalPolicyLoss(n_epochs=2)
    assert loss._fused_layers(model, torch.stack(Episode.features),
                              torch.stack(Episode.actions)) is None
    loss.compute_loss(model, Episode())
    assert model.epoch_count == 2
    after = list(model.model.parameters())
    assert len(after) == 8
    assert all(not torch.equal(a, b) for a, b in zip(after, before))


def test_export_restore_round_trip(tmp_path):
    torch.manual_seed(0)
    a = TorchModel(DeepActorCriticMLP(3, 4, (12, 12, 12)), input_shape=(3,), device="cpu")
    a.epoch_count = 7
    a.export_model("deep", str(tmp_path))
    torch.manual_seed(1)
    b = TorchModel(DeepActorCriticMLP(3, 4, (12, 12, 12)), input_shape=(3,), device="cpu")
    assert any(not torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))
    b.restore_model_state("deep", str(tmp_path))
    assert b.epoch_count == 7
    assert all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))
    x = torch.randn(5, 3)
    assert torch.equal(a.model(x)[0], b.model(x)[0])


def test_size_gate():
    assert deep_mlp_within_limits(3, (128, 128), 4)
    assert deep_mlp_within_limits(32, (12, 12, 12), 16)
    assert deep_mlp_within_limits(1, (1, 1), 1)
    assert not deep_mlp_within_limits(3, (128,), 4)          # depth 1
    assert not deep_mlp_within_limits(3, (8, 8, 8, 8), 4)    # depth 4
    assert not deep_mlp_within_limits(3, (129, 16), 4)       # width 129
    assert not deep_mlp_within_limits(33, (16, 16), 4)       # d_in 33
    assert not deep_mlp_within_limits(3, (16, 16), 17)       # k 17


def test_library_size_gate_agrees():
    """swarm_ppo_deep_workspace_bytes (host arithmetic only) declines exactly
    the sizes the Python gate declines."""
    from swarmrl_amd import _capi

    lib = _capi.lib()
    for d_in, hidden, k in [(3, (128, 128), 4), (32, (12, 12, 12), 16), (3, (128,), 4),
                            (3, (8, 8, 8, 8), 4), (3, (129, 16), 4), (33, (16, 16), 4),
                            (3, (16, 16), 17)]:
        widths = (ctypes.c_int32 * len(hidden))(*hidden)
        nbytes = lib.swarm_ppo_deep_workspace_bytes(20, 100, d_in, len(hidden),
                                                    ctypes.cast(widths, ctypes.c_void_p), k)
        assert (nbytes > 0) == deep_mlp_within_limits(d_in, hidden, k), (d_in, hidden, k)
    # T x S must stay below 2^31 samples
    widths = (ctypes.c_int32 * 2)(16, 16)
    assert lib.swarm_ppo_deep_workspace_bytes(1 << 16, 1 << 16, 3, 2,
                                              ctypes.cast(widths, ctypes.c_void_p), 4) == -1
