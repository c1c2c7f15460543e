"""
Episodic training with engine resets (reference: swarmrl/trainers/
episodic_trainer.py:17-130): every `reset_frequency` episodes -- or after a
task raised the kill switch -- a fresh engine comes from ``get_engine``; with
``save_episodic_data`` it receives the cycle index as its ``h5_group_tag``
so each reset writes its own trajectory group.  With ``reset_in_place`` the
engine is built once and every later reset is ``SwarmEngine.reset_envs`` on
the live engine.
"""

from __future__ import annotations

import numpy as np

from swarmrl_amd.trainers.trainer import Trainer


class EpisodicTrainer(Trainer):
    """Training over engines that are rebuilt between episodes."""

    def _fresh_engine(self, get_engine, system, save_episodic_data: bool, cycle: int):
        if not save_episodic_data:
            return get_engine(system)
        try:
            return get_engine(system, f"{cycle}")
        except TypeError as err:
            raise ValueError(
                "The system runner does not support episodic data saving. Your "
                "get_engine function should take a system and a str(cycle_index) as "
                "arguments. The cycle_index is passed to the engine as 'h5_group_tag'."
            ) from err

    def perform_rl_training(self, get_engine, system, n_episodes: int, episode_length: int,
                            reset_frequency: int = 1, load_bar: bool = True,
                            save_episodic_data: bool = True,
                            reset_in_place: bool = False) -> np.ndarray:
        """Train for `n_episodes` episodes; returns [0.0, reward of episode
        1, ...].  The engine is finalized after every episode
        (episodic_trainer.py:127).  reset_in_place: `get_engine` is called
        once; later resets put every env of that engine back to a fresh random
        start on the device (SwarmEngine.reset_envs) and re-initialise the
        agents' observables and tasks as a rebuild does."""
        history = [0.0]
        force_fn = self.initialize_training()
        cycle = 0
        stop = False
        built = False  # reset_in_place: get_engine has been called
        bar, task = self._progress("Episodic Training", n_episodes, load_bar)
        with bar:
            for episode in range(n_episodes):
                if stop or episode % reset_frequency == 0:
                    print(f"Resetting the system at episode {episode}")
                    if reset_in_place and built:
                        self.engine.reset_envs(
                            h5_group_tag=f"{cycle}" if save_episodic_data else None)
                    else:
                        self.engine = None
                        self.engine = self._fresh_engine(get_engine, system,
                                                         save_episodic_data, cycle)
                        built = True
                    cycle += 1 if save_episodic_data else 0
                    for agent in self.agents.values():
                        agent.reset_agent(self.engine.colloids)
                self.engine.integrate(episode_length, force_fn)
                force_fn, reward, stop = self.update_rl()
                history.append(float(reward))
                self._advance(bar, task, episode + 1, history)
                self.engine.finalize()
        return np.array(history)
