from swarmrl_amd.tasks.object_movement.rod_rotation import RotateRod

__all__ = ["RotateRod"]
