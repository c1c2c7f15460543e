"""Training routines over the trainers (reference: swarmrl/training_routines/)."""

from swarmrl_amd.training_routines.ensemble_training import EnsembleTraining

__all__ = ["EnsembleTraining"]
