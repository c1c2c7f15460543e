"""
The ensemble (population) classes without a GPU: the stacked network against
its members, the member round trips, single-member export, copy_member, the
torch path of EnsembleProximalPolicyLoss against ProximalPolicyLoss on each
member's slice, and the argument checks of EnsembleTrainer / EnsembleTraining.
"""

import os

import numpy as np
import pytest
import torch

from swarmrl_amd.losses import EnsembleProximalPolicyLoss, ProximalPolicyLoss
from swarmrl_amd.networks import (ActorCriticMLP, EnsembleActorCriticMLP, EnsembleTorchModel,
                                  TorchModel)
from swarmrl_amd.trainers import EnsembleTrainer
from swarmrl_amd.training_routines import EnsembleTraining

CPU = torch.device("cpu")
M, D, K, H = 3, 3, 4, 16


def test_members_are_initialised_as_networks_constructed_in_order():
    torch.manual_seed(3)
    ens = EnsembleActorCriticMLP(M, D, K, H)
    torch.manual_seed(3)
    nets = [ActorCriticMLP(D, K, H) for _ in range(M)]
    for m, net in enumerate(nets):
        for a, b in zip(ens.ppo_layers(), net.ppo_layers()):
            assert torch.equal(a[m], b)
    assert [tuple(p.shape) for p in ens.ppo_layers()] == [
        (M, H, D), (M, H), (M, K, H), (M, K), (M, 1, H), (M, 1)]


def test_forward_equals_each_members_forward():
    """torch.equal on CPU fp32.  n = 32 rows per member: from about 25 rows
    on every product of this size (contraction x rows x columns >= 400 for
    the one-column value head: 16 n >= 400) runs torch's GEMM in both the
    batched and the single form; below, bmm takes a plain loop whose rounding
    differs, which the second half covers at fp32 rounding."""
    torch.manual_seed(0)
    ens = EnsembleActorCriticMLP(M, D, K, H)
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
    nets = [ActorCriticMLP(D, K, H) for _ in range(M)]
    ens = EnsembleActorCriticMLP.from_members(nets)
    assert ens.n_members == M and (ens.input_dim, ens.n_actions, ens.hidden_units) == (D, K, H)
    for m, net in enumerate(nets):
        copy = ens.member(m)
        for a, b in zip(copy.ppo_layers(), net.ppo_layers()):
            assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    fresh = ActorCriticMLP(D, K, H)
    ens.set_member(1, fresh)
    for a, b, c in zip(ens.member(1).ppo_layers(), fresh.ppo_layers(), nets[1].ppo_layers()):
        assert torch.equal(a, b) and not torch.equal(a, c)
    for a, b in zip(ens.member(0).ppo_layers(), nets[0].ppo_layers()):
        assert torch.equal(a, b)  # the other members are untouched
    with pytest.raises(ValueError):
        EnsembleActorCriticMLP.from_members([nets[0], ActorCriticMLP(D, K, H + 1)])


def _trained_model(steps=2):
    torch.manual_seed(2)
    model = EnsembleTorchModel(EnsembleActorCriticMLP(M, D, K, H), device=CPU)
    x = torch.randn(M, 8, D)
    for _ in range(steps):
        logits, values = model.model(x)
        model.update_model((logits ** 2).sum() + values.sum())
    return model


def test_export_member_is_restored_by_a_stock_model(tmp_path):
    model = _trained_model()
    for m in range(M):
        model.export_member(m, filename=f"m{m}", directory=os.fspath(tmp_path))
        stock = TorchModel(ActorCriticMLP(D, K, H), device=CPU)
        stock.restore_model_state(f"m{m}", os.fspath(tmp_path))
        for a, b in zip(model.model.ppo_layers(), stock.model.ppo_layers()):
            assert torch.equal(a[m], b)
        assert stock.epoch_count == model.epoch_count == 2
        for p, q in zip(model.model.ppo_layers(), stock.model.ppo_layers()):  # Adam moments too
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(model.optimizer.state[p][key][m], stock.optimizer.state[q][key])
            assert float(stock.optimizer.state[q]["step"]) == 2.0
    # the stacked state round-trips through export_model / restore_model_state
    model.export_model("all", os.fspath(tmp_path))
    other = EnsembleTorchModel(EnsembleActorCriticMLP(M, D, K, H), device=CPU)
    other.restore_model_state("all", os.fspath(tmp_path))
    for a, b in zip(model.model.ppo_layers(), other.model.ppo_layers()):
        assert torch.equal(a, b)


def test_copy_member_copies_weights_and_adam_state():
    model = _trained_model()
    layers = model.model.ppo_layers()
    before = [p.detach().clone() for p in layers]
    model.copy_member(0, 2)
    for p, b in zip(layers, before):
        st = model.optimizer.state[p]
        assert torch.equal(p[2], b[0]) and torch.equal(p[0], b[0]) and torch.equal(p[1], b[1])
        assert torch.equal(st["exp_avg"][2], st["exp_avg"][0])
        assert torch.equal(st["exp_avg_sq"][2], st["exp_avg_sq"][0])
    w1_moment = model.optimizer.state[layers[0]]["exp_avg"]
    assert not torch.equal(w1_moment[1], w1_moment[0])  # member 1 keeps its own
    moments = [model.optimizer.state[p]["exp_avg"].clone() for p in layers]
    model.copy_member(1, 0, with_optimizer_state=False)
    for p, b, mom in zip(layers, before, moments):
        assert torch.equal(p[0], b[1])
        assert torch.equal(model.optimizer.state[p]["exp_avg"], mom)


def test_compute_action_fused_rejects_a_batch_that_does_not_divide():
    model = EnsembleTorchModel(EnsembleActorCriticMLP(M, D, K, H), device=CPU)
    tab = torch.zeros(K)
    with pytest.raises(ValueError):
        model.compute_action_fused(torch.zeros(M * 4 + 1, D), tab, tab)
    with pytest.raises(ValueError):
        model.compute_action(torch.zeros(M * 4 + 1, D))
    idx, logp = model.compute_action(torch.randn(M * 4, D))
    assert idx.shape == (M * 4,) and logp.shape == (M * 4,)
    assert model.accepts_engine is False and model.fused_policy_args(12, D, K, CPU) is None
    assert not model.fused_sampling_ok(torch.zeros(M * 4, D))  # CPU tensors: the torch path


class _Wrap:
    def __init__(self, net):
        self.net = net

    def __call__(self, features, obs_ndim=1):
        lead = features.shape[: features.ndim - obs_ndim]
        return self.net(features.reshape(*lead, -1))


def test_torch_path_gives_each_member_its_own_ppo_gradient():
    """M = 2, T = 4, S = 6 on the CPU: the gradient of the ensemble loss (the
    sum over members) on member m's slices of the stacked parameters is the
    gradient ProximalPolicyLoss._calculate_loss gives a stock network on
    member m's slice, at the criteria of tests/test_gpu_ppo.py::_check."""
    members, T, S, d, k, hidden = 2, 4, 6, 3, 4, 16
    g = torch.Generator().manual_seed(7)
    torch.manual_seed(7)
    ens = EnsembleActorCriticMLP(members, d, k, hidden)
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
        for name, p, q in zip(("W1", "b1", "Wa", "ba", "Wc", "bc"), ens.ppo_layers(),
                              net.ppo_layers()):
            a, b = p.grad[m], q.grad
            err = (a - b).norm().item()
            assert err <= 2e-4 * b.norm().item() + 1e-6, (m, name, err, b.norm().item())
            assert (a - b).abs().max().item() <= 2e-3 * b.abs().max().item() + 1e-6, (m, name)


def test_compute_loss_repacks_the_episode_member_major():
    """[T, E, A, ...] -> [M, T, (E / M) A, ...]: member m learns from envs
    [m E / M, (m + 1) E / M) only."""
    members, T, E, A, d = 2, 4, 4, 3, 3
    g = torch.Generator().manual_seed(9)
    torch.manual_seed(9)

    class Episode:
        features = list(torch.randn(T, E, A, d, generator=g))
        actions = list(torch.randint(0, 4, (T, E, A), generator=g))
        rewards = list(torch.randn(T, E, A, generator=g))
        log_probs = list(-1.386 + 0.3 * torch.randn(T, E, A, generator=g))

    model = EnsembleTorchModel(EnsembleActorCriticMLP(members, d, 4, 16), device=CPU,
                               optimizer=lambda ps: torch.optim.SGD(ps, lr=1e-3))
    loss = EnsembleProximalPolicyLoss(n_epochs=1)
    f, a, lp, r = loss.member_major(model, Episode())
    assert f.shape == (members, T, 2 * A, d) and a.shape == r.shape == lp.shape == (members, T, 6)
    feats = torch.stack(Episode.features)
    assert torch.equal(f[1], feats[:, 2:4].reshape(T, 2 * A, d))
    assert torch.equal(a[0], torch.stack(Episode.actions)[:, 0:2].reshape(T, 2 * A))
    # one SGD step of compute_loss = each member's own step on its envs
    stocks = [TorchModel(model.model.member(m), device=CPU,
                         optimizer=lambda ps: torch.optim.SGD(ps, lr=1e-3)) for m in range(members)]
    loss.compute_loss(model, Episode())
    for m, stock in enumerate(stocks):
        class Mine:
            features = [x[2 * m:2 * m + 2] for x in Episode.features]
            actions = [x[2 * m:2 * m + 2] for x in Episode.actions]
            rewards = [x[2 * m:2 * m + 2] for x in Episode.rewards]
            log_probs = [x[2 * m:2 * m + 2] for x in Episode.log_probs]
        ProximalPolicyLoss(n_epochs=1).compute_loss(stock, Mine())
        for p, q in zip(model.model.ppo_layers(), stock.model.ppo_layers()):
            torch.testing.assert_close(p[m], q, rtol=1e-4, atol=1e-6)


class _Engine:
    def __init__(self, n_envs):
        self.n_envs = n_envs


def _agent(members, intrinsic_reward=None):
    from swarmrl_amd.agents import ActorCriticAgent

    net = EnsembleTorchModel(EnsembleActorCriticMLP(members, 1, 4, 8), device=CPU)
    return ActorCriticAgent(0, net, task=None, observable=None, actions={},
                            loss=EnsembleProximalPolicyLoss(), intrinsic_reward=intrinsic_reward)


def test_trainer_rejects_bad_env_counts_and_intrinsic_rewards():
    trainer = EnsembleTrainer([_agent(3)])
    assert trainer.n_members == 3
    with pytest.raises(ValueError):
        trainer.perform_rl_training(_Engine(4), n_episodes=1, episode_length=1, load_bar=False)
    with pytest.raises(ValueError):
        EnsembleTrainer([_agent(3, intrinsic_reward=object())])


def test_trainer_reduces_rewards_per_member():
    from swarmrl_amd.trainers.ensemble_trainer import member_mean_rewards

    r = [torch.arange(8.0).reshape(4, 2), torch.arange(8.0).reshape(4, 2) + 10]  # T=2, E=4, A=2
    got = member_mean_rewards(r, 2)
    np.testing.assert_allclose(got, [1.5 + 5.0, 5.5 + 5.0])


def test_ensemble_training_rejects_a_cluster(tmp_path):
    trainer = EnsembleTrainer([_agent(2)])
    with pytest.raises(ValueError):
        EnsembleTraining(trainer, lambda: _Engine(4), 2, 3, 1, cluster=object(),
                         output_dir=tmp_path / "out")
    routine = EnsembleTraining(trainer, lambda: _Engine(3), 2, 3, 1, n_parallel_jobs=7,
                               output_dir=tmp_path / "out")
    with pytest.raises(ValueError):  # 3 envs, 2 members
        routine.train_ensemble()
