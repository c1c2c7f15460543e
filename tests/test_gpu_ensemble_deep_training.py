"""
Deep ensemble training end to end: the set-up of
tests/test_gpu_ensemble_training.py (an engine of 4 envs x 32 colloids, 2-D,
ConcentrationField + GradientSensing, M = 2 members, episodes of 3 slices, two
episodes, 3 PPO epochs each -- the first update eager, the second the captured
graph) with EnsembleDeepActorCriticMLP(2, 1, 4, (16, 16)):

  rollout  each member's recorded actions and log-probs are what the
           single-model kernel (ops.policy_deep_sample) gives on the member's
           recorded features with its weights of that episode, its seed and
           counters starting from zero -- bit for bit.
  update   a stock TorchModel(DeepActorCriticMLP) with the member's pre-update
           weights and Adam state, trained by ProximalPolicyLoss.compute_loss
           on the member's slice of the episode, ends on the member's
           post-update parameters -- bit for bit.

And a genetic run (GeneticTraining: population 4 with one env each, two
generations of one episode of 3 slices, 2 parents, a fixed rng): generation
1 starts from the gather of generation 0's final weights and Adam moments by
the parent map, every child is on disk, and the returned path is the last
generation's best child, restorable into a stock model.
"""

import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
M, E, N, T, EPISODES, EPOCHS = 2, 4, 32, 3, 2, 3
HIDDEN = (16, 16)
NAME = "ActorCriticAgent_0"
NAMES = ("W1", "b1", "W2", "b2", "Wa", "ba", "Wc", "bc")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from swarmrl_amd import _capi

    _capi.require_gpu()
    torch.cuda.set_device(0)


def _engine(out_folder, seed=42):
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    L = 2.0 * math.sqrt(N * 1.0 ** 2 / 0.1)
    ureg = UnitRegistry()
    params = MDParams(
        ureg=ureg,
        box_length=ureg.Quantity([L, L, L], "micrometer"),
        time_step=ureg.Quantity(1e-3, "second"),
        time_slice=ureg.Quantity(0.1, "second"),
        write_interval=ureg.Quantity(1.0, "second"),
    )
    eng = SwarmEngine(params, n_dims=2, seed=seed, n_envs=E, out_folder=os.fspath(out_folder))
    eng.add_colloids(N, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(np.array([L / 2, L / 2, 0.0]), "micrometer"),
                     ureg.Quantity(L / 2, "micrometer"))
    return eng, L


def _agent(L, members, seed=42):
    from swarmrl_amd.actions import Action
    from swarmrl_amd.agents import ActorCriticAgent
    from swarmrl_amd.losses import EnsembleProximalPolicyLoss
    from swarmrl_amd.networks import EnsembleDeepActorCriticMLP, EnsembleTorchModel
    from swarmrl_amd.observables import ConcentrationField
    from swarmrl_amd.tasks.searching import GradientSensing

    box = np.array([L, L, L])
    src = np.array([L / 2, L / 2, 0.0])
    obs = ConcentrationField(src, lambda d: 1 - d, box, scale_factor=10000)
    task = GradientSensing(source=src, decay_function=lambda d: 1 - d, box_length=box,
                           reward_scale_factor=10)
    torch.manual_seed(seed)
    net = EnsembleTorchModel(EnsembleDeepActorCriticMLP(members, 1, 4, HIDDEN),
                             input_shape=(1,), device=DEV)
    actions = {
        "RotateClockwise": Action(torque=np.array([0.0, 0.0, 10.0])),
        "Translate": Action(force=10.0),
        "RotateCounterClockwise": Action(torque=np.array([0.0, 0.0, -10.0])),
        "DoNothing": Action(),
    }
    return ActorCriticAgent(0, net, task, obs, actions, train=True,
                            loss=EnsembleProximalPolicyLoss(n_epochs=EPOCHS))


def _flat_layers(net):
    ws, bs, wa, ba, wc, bc = net.deep_layers()
    return (*(t for pair in zip(ws, bs) for t in pair), wa, ba, wc, bc)


def _train(tmp_path):
    """Two recorded episodes: per episode the trajectory, every member
    exported before the update (weights + Adam state) and the stacked
    parameters after it."""
    from swarmrl_amd.trainers import EnsembleTrainer

    eng, L = _engine(tmp_path / "engine")
    agent = _agent(L, M)
    net = agent.network
    recorded = []
    update = agent.update_agent

    def recording_update():
        tr = agent.trajectory
        rec = {k: [torch.as_tensor(x).clone() for x in getattr(tr, k)]
               for k in ("features", "actions", "log_probs", "rewards")}
        rec["pre"] = tmp_path / f"pre_{len(recorded)}"
        for m in range(M):
            net.export_member(m, filename=f"member_{m}", directory=os.fspath(rec["pre"]))
        out = update()
        torch.cuda.synchronize()
        rec["post"] = [p.detach().clone() for p in net.model.ppo_layers()]
        rec["graph"] = getattr(agent.loss, "_ppo_graph", None) is not None
        recorded.append(rec)
        return out

    agent.update_agent = recording_update
    trainer = EnsembleTrainer([agent])
    rewards = trainer.perform_rl_training(eng, n_episodes=EPISODES, episode_length=T,
                                          load_bar=False)
    return trainer, agent, recorded, rewards


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return _train(tmp_path_factory.mktemp("deep_ensemble"))


def _member(t, m):
    """Member m's envs of an [E, A, ...] slice."""
    per = E // M
    return t[m * per:(m + 1) * per]


def _stock(directory, name):
    from swarmrl_amd.networks import DeepActorCriticMLP, TorchModel

    model = TorchModel(DeepActorCriticMLP(1, 4, HIDDEN), input_shape=(1,), device=DEV)
    model.restore_model_state(name, os.fspath(directory))
    return model


def test_rollout_is_the_members_own_deep_policy(run):
    from swarmrl_amd.engine import ops

    _, agent, recorded, rewards = run
    net = agent.network
    assert rewards.shape == (EPISODES + 1, M) and np.all(np.isfinite(rewards))
    assert [rec["graph"] for rec in recorded] == [False, True]  # eager, then captured
    _, ftab, ttab, _ = agent._action_tables(DEV)
    n_per = (E // M) * N
    counters = [torch.zeros((n_per + 63) // 64, dtype=torch.int64, device=DEV) for _ in range(M)]
    for rec in recorded:
        assert len(rec["actions"]) == T
        for m in range(M):
            ws, bs, wa, ba, _, _ = _stock(rec["pre"], f"member_{m}").model.deep_layers()
            for s in range(T):
                obs = _member(rec["features"][s], m).reshape(n_per, -1).float()
                idx, logp, _, _ = ops.policy_deep_sample(obs, ws, bs, wa, ba,
                                                         net.member_seeds[m], counters[m], 0.0,
                                                         ftab, ttab)
                assert torch.equal(idx, _member(rec["actions"][s], m).reshape(-1)), (m, s)
                assert torch.equal(logp, _member(rec["log_probs"][s], m).reshape(-1)), (m, s)
    assert torch.equal(net._fused_state, torch.stack(counters))
    assert int(net._fused_state[0, 0]) == EPISODES * T


def test_update_is_the_members_own_deep_ppo(run):
    from swarmrl_amd.losses import ProximalPolicyLoss

    _, _, recorded, _ = run
    for ep, rec in enumerate(recorded):
        for m in range(M):
            stock = _stock(rec["pre"], f"member_{m}")
            assert stock.ppo_layers(1) is not None  # the fused deep kernels, not autograd

            class Episode:
                features = [_member(x, m) for x in rec["features"]]
                actions = [_member(x, m) for x in rec["actions"]]
                log_probs = [_member(x, m) for x in rec["log_probs"]]
                rewards = [_member(x, m) for x in rec["rewards"]]

            ProximalPolicyLoss(n_epochs=EPOCHS).compute_loss(stock, Episode())
            torch.cuda.synchronize()
            for name, a, b in zip(NAMES, rec["post"], _flat_layers(stock.model)):
                assert torch.equal(a[m], b), (ep, m, name, (a[m] - b).abs().max().item())
    # and the updates moved the members, each its own way
    assert not torch.equal(recorded[0]["post"][0], recorded[1]["post"][0])
    assert not torch.equal(recorded[1]["post"][0][0], recorded[1]["post"][0][1])


def _snapshot(net):
    layers = net.model.ppo_layers()
    torch.cuda.synchronize()
    state = net.optimizer.state
    return {"w": [p.detach().clone() for p in layers],
            "m": [state[p]["exp_avg"].clone() if p in state else None for p in layers],
            "v": [state[p]["exp_avg_sq"].clone() if p in state else None for p in layers]}


def test_genetic_run_inherits_by_gather_and_exports_every_child(tmp_path):
    from swarmrl_amd.trainers import EnsembleTrainer
    from swarmrl_amd.training_routines import GeneticTraining

    population, generations = 4, 2
    made = []

    def generator():
        eng, _ = _engine(tmp_path / f"engine_{len(made)}", seed=42 + len(made))
        made.append(eng)
        return eng

    L = 2.0 * math.sqrt(N * 1.0 ** 2 / 0.1)
    agent = _agent(L, population, seed=5)
    net = agent.network
    trainer = EnsembleTrainer([agent])
    routine = GeneticTraining(trainer, generator, n_episodes=1, episode_length=T,
                              number_of_generations=generations, population_size=population,
                              number_of_parents=2, output_directory=os.fspath(tmp_path),
                              rng=3)
    before, after, selected, scores = [], [], [], []
    train, select = trainer.perform_rl_training, routine._select_parents

    def recording_training(*args, **kwargs):
        before.append(_snapshot(net))
        rewards = train(*args, **kwargs)
        after.append(_snapshot(net))
        return rewards

    def recording_select(s):
        scores.append(np.array(s))
        selected.append(select(s))
        return selected[-1]

    trainer.perform_rl_training = recording_training
    routine._select_parents = recording_select
    seeds = list(net.member_seeds)
    best = routine.train_model()

    assert len(made) == generations and len(before) == len(after) == generations
    assert net.member_seeds == seeds
    # the selection: the argmax first, then the draw of default_rng(3)
    rng = np.random.default_rng(3)
    for (parents, reward), s in zip(selected, scores):
        assert s.shape == (population,) and np.all(np.isfinite(s))
        assert parents[0] == int(np.argmax(s)) and reward == float(s.max())
        assert parents[1:] == [int(i) for i in rng.choice(list(range(population)), size=1,
                                                          replace=False)]
    # generation 1 starts from the gather of generation 0's final state
    parents = selected[0][0]
    parent_of = [parents[0], parents[0], parents[1], parents[1]]
    assert routine._parent_of(parents) == parent_of
    assert all(m is not None for m in after[0]["m"])  # Adam state exists after generation 0
    for key in ("w", "m", "v"):
        for name, a, b in zip(NAMES, before[1][key], after[0][key]):
            assert torch.equal(a, b[parent_of]), (key, name)
    assert not torch.equal(after[1]["w"][0], before[1]["w"][0])  # and trains on from there
    # every child of every generation is on disk
    root = tmp_path / "genetic_algorithm"
    for g in range(generations):
        for m in range(population):
            assert (root / f"_generation_{g}" / f"_child_{m}" / "Models" / f"{NAME}.pt").is_file()
    # the best child of the last generation, as a stock model
    assert best == root / f"_generation_{generations - 1}" / f"_child_{selected[-1][0][0]}"
    stock = _stock(best / "Models", NAME)
    m = selected[-1][0][0]
    for a, b in zip(after[-1]["w"], _flat_layers(stock.model)):
        assert torch.equal(a[m], b)
    assert stock.epoch_count == generations * EPOCHS
