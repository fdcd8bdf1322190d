"""Robot registration (names of aerial_gym/robots/__init__.py:37-66 that are in scope)."""
from ..config.robot_config import (
    BaseOctarotorCfg,
    BaseOctarotorWithLidar32x512Cfg,
    BaseQuadCfg,
    BaseRandCfg,
    BaseROVCfg,
    BaseQuadRootLinkControlCfg,
    BaseQuadWithCamera64x48Cfg,
    BaseQuadWithCameraCfg,
    BaseQuadWithCameraImuCfg,
    BaseQuadWithImuCfg,
    BaseQuadWithFaceIDNormalCameraCfg,
    BaseQuadWithLidarCfg,
    BaseQuadWithStereoCameraCfg,
    LMF1Cfg,
    LMF2Cfg,
    LMF2RadarCfg,
    LMF2With64x48CameraCfg,
    MagpieCfg,
    TinyPropCfg,
)
from ..registry.robot_registry import robot_registry
from .base_multirotor import BaseMultirotor
from .base_rov import BaseROV

robot_registry.register("base_quadrotor", BaseMultirotor, BaseQuadCfg)
robot_registry.register("base_octarotor", BaseMultirotor, BaseOctarotorCfg)
robot_registry.register("base_quadrotor_with_camera", BaseMultirotor, BaseQuadWithCameraCfg)
robot_registry.register("base_quadrotor_with_camera_64x48", BaseMultirotor, BaseQuadWithCamera64x48Cfg)
robot_registry.register("base_quadrotor_with_lidar", BaseMultirotor, BaseQuadWithLidarCfg)
robot_registry.register("base_octarotor_with_lidar_32x512", BaseMultirotor, BaseOctarotorWithLidar32x512Cfg)
robot_registry.register("base_quadrotor_with_faceid_normal_camera", BaseMultirotor, BaseQuadWithFaceIDNormalCameraCfg)
robot_registry.register("base_quadrotor_with_stereo_camera", BaseMultirotor, BaseQuadWithStereoCameraCfg)
robot_registry.register("magpie", BaseMultirotor, MagpieCfg)
robot_registry.register("base_quadrotor_with_imu", BaseMultirotor, BaseQuadWithImuCfg)
robot_registry.register("base_quadrotor_with_camera_imu", BaseMultirotor, BaseQuadWithCameraImuCfg)
robot_registry.register("lmf2", BaseMultirotor, LMF2Cfg)
robot_registry.register("lmf2_with_camera_64x48", BaseMultirotor, LMF2With64x48CameraCfg)
robot_registry.register("lmf2_radar", BaseMultirotor, LMF2RadarCfg)  # robots/__init__.py:52 of the reference: the radar task's robot
robot_registry.register("base_quad_root_link_control", BaseMultirotor, BaseQuadRootLinkControlCfg)
robot_registry.register("tinyprop", BaseMultirotor, TinyPropCfg)  # robots/__init__.py of the reference: the end-to-end task's airframe
robot_registry.register("base_rov", BaseROV, BaseROVCfg)  # robots/__init__.py:41 of the reference: the fully actuated ROV (BlueROV airframe)
robot_registry.register("base_random", BaseMultirotor, BaseRandCfg)  # robots/__init__.py:40 of the reference: eight motors at arbitrary poses, centre of mass off the base link
robot_registry.register("lmf1", BaseMultirotor, LMF1Cfg)  # robots/__init__.py:50 of the reference
