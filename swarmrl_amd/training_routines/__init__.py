"""Training routines over the trainers (reference: swarmrl/training_routines/)."""

from swarmrl_amd.training_routines.ensemble_training import EnsembleTraining
from swarmrl_amd.training_routines.genetic import GeneticTraining

__all__ = ["EnsembleTraining", "GeneticTraining"]
