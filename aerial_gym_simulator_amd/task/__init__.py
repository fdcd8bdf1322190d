"""Task registration (aerial_gym/task/__init__.py)."""
from ..config.task_config import (
    fully_actuated_lidar_navigation_task_config,
    lidar_navigation_task_config,
    navigation_task_config,
    position_setpoint_task_acceleration_sim2real_config,
    position_setpoint_task_config,
    position_setpoint_task_sim2real_end_to_end_config,
    position_setpoint_task_sim2real_config,
    radar_navigation_task_config,
)
from ..registry.task_registry import task_registry
from .lidar_navigation_task import LiDARNavigationTask
from .navigation_task import NavigationTask
from .position_setpoint_task import PositionSetpointTask
from .position_setpoint_task_sim2real_end_to_end import PositionSetpointTaskSim2RealEndToEnd
from .position_setpoint_task_sim2real import PositionSetpointTaskAccelerationSim2Real, PositionSetpointTaskSim2Real
from .radar_navigation_task import RadarNavigationTask

task_registry.register_task("position_setpoint_task", PositionSetpointTask, position_setpoint_task_config)
task_registry.register_task("navigation_task", NavigationTask, navigation_task_config)
task_registry.register_task("lidar_navigation_task", LiDARNavigationTask, lidar_navigation_task_config)
# the LiDAR recipe on lmf2 + a forward-looking radar (task/__init__.py:122-132 of the reference)
task_registry.register_task("radar_navigation_task", RadarNavigationTask, radar_navigation_task_config)
# BASELINE configs[3] as written (fully-actuated octarotor + 32 x 512 LiDAR): the reference's NavigationTask on that robot
task_registry.register_task("navigation_task_fully_actuated_lidar", NavigationTask, fully_actuated_lidar_navigation_task_config)
# the two networks the reference flies on the real lmf2 (task/__init__.py of the reference, same names)
task_registry.register_task("position_setpoint_task_sim2real", PositionSetpointTaskSim2Real, position_setpoint_task_sim2real_config)
task_registry.register_task("position_setpoint_task_acceleration_sim2real", PositionSetpointTaskAccelerationSim2Real,
                            position_setpoint_task_acceleration_sim2real_config)
# ... and the one whose policy commands the motor thrusts of the tinyprop directly
task_registry.register_task("position_setpoint_task_sim2real_end_to_end", PositionSetpointTaskSim2RealEndToEnd,
                            position_setpoint_task_sim2real_end_to_end_config)
