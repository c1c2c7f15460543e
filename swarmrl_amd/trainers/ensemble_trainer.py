"""
Train an ensemble of independent policies on one batched engine.

The reference's EnsembleTraining (swarmrl/training_routines/
ensemble_submit.py:17-176) runs one process, engine and trainer per model.
Here one engine steps E envs, member m of every agent's EnsembleTorchModel
owns envs [m E/M, (m + 1) E/M) and learns from them alone: one launch samples
every member's actions, one set of launches computes every member's PPO
gradient, one optimizer step updates all members.  This is unlike the
episode-parallel trainers, whose workers pool their experience into ONE
model (trainers/episode_parallel.py).
"""

from __future__ import annotations

import os

import numpy as np
import torch

from swarmrl_amd.agents.actor_critic import ActorCriticAgent
from swarmrl_amd.force_functions.force_fn import ForceFunction
from swarmrl_amd.trainers.continuous_trainer import ContinuousTrainer
from swarmrl_amd.trainers.trainer import _is_killed


def member_mean_rewards(rewards, n_members: int) -> np.ndarray:
    """[M] mean episode reward per member: over the member's envs, agents
    and chunks of a list of [E, A] per-chunk rewards (device tensors or
    arrays; one host sync per episode)."""
    if rewards is None or len(rewards) == 0:
        return np.zeros(n_members)
    r = torch.stack([torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
                     for x in rewards]).double()
    if r.ndim == 2:  # [T, A]: one env
        r = r.unsqueeze(1)
    T, E = int(r.shape[0]), int(r.shape[1])
    if E % n_members != 0:
        raise ValueError(f"{E} envs do not divide among {n_members} ensemble members")
    per = r.reshape(T, n_members, -1).mean(dim=(0, 2))
    return per.cpu().numpy()


class EnsembleTrainer(ContinuousTrainer):
    """ContinuousTrainer for agents whose networks are EnsembleTorchModels of
    n_members members each.  A task's kill switch is one flag of the shared
    engine: when any member's envs raise it, training stops for ALL members
    (the reference would stop that member's process only)."""

    def __init__(self, agents, n_members: int = None):
        super().__init__(agents)
        learners = [a for a in self.agents.values() if isinstance(a, ActorCriticAgent)]
        for agent in learners:
            if getattr(agent, "intrinsic_reward", None) is not None:
                raise ValueError("EnsembleTrainer does not support an intrinsic reward "
                                 "(a per-member RND is out of scope)")
            if not hasattr(agent.network, "n_members"):
                raise ValueError("EnsembleTrainer needs agents with an EnsembleTorchModel")
        counts = {int(a.network.n_members) for a in learners}
        if n_members is not None:
            counts.add(int(n_members))
        if len(counts) != 1:
            raise ValueError(f"the agents' ensembles must have one size, got {sorted(counts)}")
        self.n_members = counts.pop()

    def _check_engine(self, engine):
        n_envs = int(getattr(engine, "n_envs", 1))
        if n_envs % self.n_members != 0:
            raise ValueError(f"engine.n_envs = {n_envs} is not a multiple of the "
                             f"{self.n_members} ensemble members")

    def update_rl(self):
        """Update every learning agent after an episode.  Returns the next
        force function, the [M] per-member rewards (summed over the learning
        agents; each the mean over the member's envs, agents and chunks) and
        whether any task asked to stop."""
        total = np.zeros(self.n_members)
        stop = False
        for agent in self.agents.values():
            if not isinstance(agent, ActorCriticAgent):
                continue
            # (GeneticTraining's generations run through here as well)
            self._refuse_dones(agent, type(self).__name__)
            rewards, killed = self._update_agent(agent)
            total += member_mean_rewards(rewards, self.n_members)
            stop = stop or _is_killed(killed)
        return ForceFunction(agents=self.agents), total, stop

    def perform_rl_training(self, system_runner, n_episodes: int, episode_length: int,
                            load_bar: bool = True) -> np.ndarray:
        """Train for `n_episodes` episodes; returns [n_episodes + 1, M]: a
        leading zero row, then every member's reward per episode (the scalar
        history of ContinuousTrainer, per member).  A kill switch ends the
        training of all members; that episode is not recorded."""
        self._check_engine(system_runner)
        self.engine = system_runner
        history = [np.zeros(self.n_members)]
        force_fn = self.initialize_training()
        for agent in self.agents.values():
            agent.reset_agent(self.engine.colloids)
        bar, task = self._progress("Ensemble RL Training", n_episodes, load_bar)
        with bar:
            for episode in range(1, n_episodes + 1):
                self.engine.integrate(episode_length, force_fn)
                force_fn, reward, stop = self.update_rl()
                if stop:
                    print("Simulation has been ended by the task, ending training.")
                    system_runner.finalize()
                    break
                history.append(np.asarray(reward, dtype=float))
                self._advance(bar, task, episode, [float(h.mean()) for h in history])
        return np.stack(history)

    def export_models(self, directory: str = "."):
        """Write every member on its own, in the reference's on-disk layout:
        directory/ensemble_{m}/Models/ActorCriticAgent_{type}.pt, each a file
        a stock TorchModel(ActorCriticMLP(...)) restores."""
        for m in range(self.n_members):
            models = os.path.join(os.fspath(directory), f"ensemble_{m}", "Models")
            for agent in self.agents.values():
                if isinstance(agent, ActorCriticAgent):
                    agent.network.export_member(
                        m, filename=f"{agent.__name__()}_{agent.particle_type}",
                        directory=models)
