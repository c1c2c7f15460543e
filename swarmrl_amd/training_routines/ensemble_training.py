"""
Ensemble training (reference: swarmrl/training_routines/ensemble_submit.py:
17-176), in one process on one batched engine.

The reference submits one job per model to a dask cluster, each with an
engine and a trainer of its own, and returns {model_id: rewards}.  Here the
models are the members of the trainer's EnsembleTorchModels and the engines
the env blocks of one engine (trainers/ensemble_trainer.py): same
constructor, same return value, same files on disk
(output_dir/ensemble_{m}/Models/...).
"""

from __future__ import annotations

import os
from pathlib import Path

from swarmrl_amd.trainers.ensemble_trainer import EnsembleTrainer


class EnsembleTraining:
    """Train `number_of_ensembles` independent models at once."""

    def __init__(
        self,
        trainer: EnsembleTrainer,
        simulation_runner_generator: callable,
        number_of_ensembles: int,
        episode_length: int,
        n_episodes: int,
        n_parallel_jobs: int = None,
        load_path: Path = None,
        cluster=None,
        output_dir: Path = Path("./ensembled-training"),
    ) -> None:
        """
        trainer: an EnsembleTrainer whose agents hold number_of_ensembles
        members.  simulation_runner_generator: called once; returns one
        engine whose n_envs is a multiple of number_of_ensembles (member m
        trains on envs [m n_envs / M, (m + 1) n_envs / M)).  n_parallel_jobs
        is accepted for the reference's signature and ignored: every member
        runs in the same launches.  cluster must be None: there are no jobs
        to submit.  load_path: a directory to restore the (stacked) models
        from, else they are re-initialised.
        """
        if cluster is not None:
            raise ValueError("EnsembleTraining runs in one process on one engine; "
                             "a cluster is not supported")
        if int(getattr(trainer, "n_members", number_of_ensembles)) != int(number_of_ensembles):
            raise ValueError(f"the trainer's ensembles have {trainer.n_members} members, "
                             f"number_of_ensembles is {number_of_ensembles}")
        self.trainer = trainer
        self.simulation_runner_generator = simulation_runner_generator
        self.number_of_ensembles = int(number_of_ensembles)
        self.episode_length = episode_length
        self.n_episodes = n_episodes
        self.n_parallel_jobs = n_parallel_jobs
        self.load_path = load_path
        self.output_dir = Path(output_dir)
        os.makedirs(self.output_dir, exist_ok=True)

    def train_ensemble(self) -> dict:
        """Train the ensemble; returns {model_id: rewards} with model_id =
        str(m) and rewards member m's history [0.0, episode 1, ...]."""
        system_runner = self.simulation_runner_generator()
        n_envs = int(getattr(system_runner, "n_envs", 1))
        if n_envs % self.number_of_ensembles != 0:
            raise ValueError(f"the engine's n_envs = {n_envs} is not a multiple of "
                             f"number_of_ensembles = {self.number_of_ensembles}")
        if self.load_path is not None:
            self.trainer.restore_models(directory=os.fspath(self.load_path))
        else:
            self.trainer.initialize_models()
        rewards = self.trainer.perform_rl_training(
            system_runner, n_episodes=self.n_episodes, episode_length=self.episode_length,
            load_bar=False)
        self.trainer.export_models(self.output_dir)
        return {str(m): rewards[:, m] for m in range(self.number_of_ensembles)}
