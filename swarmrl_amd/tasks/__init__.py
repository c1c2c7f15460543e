from swarmrl_amd.tasks import object_movement, searching
from swarmrl_amd.tasks.multi_tasking import MultiTasking
from swarmrl_amd.tasks.object_movement import RotateRod
from swarmrl_amd.tasks.task import Task

__all__ = ["Task", "MultiTasking", "RotateRod", "object_movement", "searching"]
