"""Robot configs: base_quadrotor and base_octarotor
(aerial_gym/config/robot_config/base_quad_config.py, base_octarotor_config.py) plus the URDF
constants of resources/robots/{quad,octarotor}/*.urdf as data (``robot_model``); magpie, lmf2, tinyprop, base_rov the same way."""
import numpy as np

from .sensor_config import (
    BaseDepthCameraConfig,
    BaseImuConfig,
    BaseLidarConfig,
    BaseNormalFaceIDCameraConfig,
    DepthCamera64x48Config,
    Lidar32x512Config,
    RSLidar_Airy_Config,
    StereoCameraConfig,
    fake_radar_config,
)

_PI = float(np.pi)


def _state_ratio(lo_xyz, hi_xyz, yaw):
    lo = list(lo_xyz) + [0, 0, -yaw, 1.0] + [0] * 6
    hi = list(hi_xyz) + [0, 0, yaw, 1.0] + [0] * 6
    return lo, hi


class _CommonAsset:
    base_link_name = "base_link"
    disable_gravity = False
    collapse_fixed_joints = False
    fix_base_link = False
    collision_mask = 0
    density = 0.000001
    max_angular_velocity = 100.0
    max_linear_velocity = 100.0
    armature = 0.001
    semantic_id = 0
    per_link_semantic = False
    min_state_ratio, max_state_ratio = _state_ratio([0.1, 0.1, 0.1], [0.3, 0.9, 0.9], _PI)
    max_force_and_torque_disturbance = [0.1, 0.1, 0.1, 0.05, 0.05, 0.05]
    keep_in_env = True
    min_euler_angles, max_euler_angles = [-_PI] * 3, [_PI] * 3


class BaseQuadCfg:
    class init_config:  # [ratio xyz, roll, pitch, yaw, 1.0, v xyz, w xyz]
        min_init_state = [0.1, 0.15, 0.15, 0, 0, -_PI / 6, 1.0, -0.2, -0.2, -0.2, -0.2, -0.2, -0.2]
        max_init_state = [0.2, 0.85, 0.85, 0, 0, _PI / 6, 1.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2]

    class sensor_config:
        enable_camera = False
        camera_config = BaseDepthCameraConfig
        enable_lidar = False
        lidar_config = BaseLidarConfig
        enable_imu = False
        imu_config = None

    class disturbance:
        enable_disturbance = False
        prob_apply_disturbance = 0.02
        max_force_and_torque_disturbance = [0.75, 0.75, 0.75, 0.004, 0.004, 0.004]

    class damping:  # body-frame drag coefficients, all zero for the base quad
        linvel_linear_damping_coefficient = [0.0, 0.0, 0.0]
        linvel_quadratic_damping_coefficient = [0.0, 0.0, 0.0]
        angular_linear_damping_coefficient = [0.0, 0.0, 0.0]
        angular_quadratic_damping_coefficient = [0.0, 0.0, 0.0]

    class robot_asset(_CommonAsset):
        file = "quad.urdf"
        name = "base_quadrotor"
        angular_damping = 0.01
        linear_damping = 0.01

    class robot_model:  # resources/robots/quad/quad.urdf
        base_mass = 0.225
        base_inertia = [[4.225e-4, 0, 0], [0, 4.225e-4, 0], [0, 0, 8.45e-4]]
        collision_sphere_radius = 0.18384776310850237
        motor_mass = 0.00625
        motor_xyz = [[0.13, -0.13, 0.0], [-0.13, -0.13, 0.0], [-0.13, 0.13, 0.0], [0.13, 0.13, 0.0]]
        motor_rpy = [[0.0, 0.0, 0.0]] * 4

    class control_allocator_config:
        num_motors = 4
        force_application_level = "motor_link"
        application_mask = [1 + 4 + i for i in range(4)]
        motor_directions = [1, -1, 1, -1]
        allocation_matrix = [
            [0.0, 0.0, 0.0, 0.0],
            [0.0, 0.0, 0.0, 0.0],
            [1.0, 1.0, 1.0, 1.0],
            [-0.13, -0.13, 0.13, 0.13],
            [-0.13, 0.13, 0.13, -0.13],
            [-0.01, 0.01, -0.01, 0.01],
        ]

        class motor_model_config:
            use_rps = True
            motor_thrust_constant_min, motor_thrust_constant_max = 0.00000926312, 0.00001826312
            motor_time_constant_increasing_min = motor_time_constant_increasing_max = 0.04
            motor_time_constant_decreasing_min = motor_time_constant_decreasing_max = 0.04
            max_thrust, min_thrust = 2, 0
            max_thrust_rate = 100000.0
            thrust_to_torque_ratio = 0.01
            use_discrete_approximation = True


class BaseQuadWithCameraCfg(BaseQuadCfg):
    class sensor_config(BaseQuadCfg.sensor_config):
        enable_camera = True
        camera_config = BaseDepthCameraConfig


class BaseQuadWithCamera64x48Cfg(BaseQuadCfg):
    class sensor_config(BaseQuadCfg.sensor_config):
        enable_camera = True
        camera_config = DepthCamera64x48Config


class BaseQuadWithImuCfg(BaseQuadCfg):  # base_quad_config.py:196-199
    class sensor_config(BaseQuadCfg.sensor_config):
        enable_imu = True
        imu_config = BaseImuConfig


class BaseQuadWithCameraImuCfg(BaseQuadCfg):  # base_quad_config.py:207-213
    class sensor_config(BaseQuadCfg.sensor_config):
        enable_camera = True
        camera_config = BaseDepthCameraConfig
        enable_imu = True
        imu_config = BaseImuConfig


class BaseQuadWithLidarCfg(BaseQuadCfg):
    class sensor_config(BaseQuadCfg.sensor_config):
        enable_lidar = True
        lidar_config = BaseLidarConfig


class BaseQuadWithFaceIDNormalCameraCfg(BaseQuadCfg):  # base_quad_config.py:220-223
    class sensor_config(BaseQuadCfg.sensor_config):
        enable_camera = True
        camera_config = BaseNormalFaceIDCameraConfig


class BaseQuadWithStereoCameraCfg(BaseQuadCfg):  # base_quad_config.py:225-228
    class sensor_config(BaseQuadCfg.sensor_config):
        enable_camera = True
        camera_config = StereoCameraConfig


_S = 0.17320508075688776
_OCTA_RPY = [
    [0.5369911762672153, 0.8339952782025826, -2.726309414768267],
    [-2.191861365711223, -0.12515405937833668, -0.17271936472604107],
    [2.191861365711223, 0.1251540593783369, -0.17271936472604107],
    [-0.5369911762672153, -0.8339952782025827, -2.726309414768267],
]


class BaseOctarotorCfg:
    class init_config:
        min_init_state = [0.0, 0.0, 0.0, 0, 0, -_PI, 1.0, -0.2, -0.2, -0.2, -0.2, -0.2, -0.2]
        max_init_state = [1.0, 1.0, 1.0, 0, 0, _PI, 1.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2]

    class sensor_config(BaseQuadCfg.sensor_config):
        pass

    class disturbance:
        enable_disturbance = True
        prob_apply_disturbance = 0.05
        max_force_and_torque_disturbance = [1.5, 1.5, 1.5, 0.25, 0.25, 0.25]

    class damping(BaseQuadCfg.damping):
        pass

    class robot_asset(_CommonAsset):
        file = "octarotor.urdf"
        name = "base_octarotor"
        angular_damping = 0.0000001
        linear_damping = 0.0000001

    class robot_model:  # resources/robots/octarotor/octarotor.urdf
        base_mass = 0.3
        base_inertia = [[0.048000000000000015, 0, 0], [0, 0.048000000000000015, 0], [0, 0, 0.048000000000000015]]
        collision_sphere_radius = 0.30000000000000004
        motor_mass = 0.1
        motor_xyz = [[sx * _S, sy * _S, sz * _S] for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)]
        motor_rpy = _OCTA_RPY + _OCTA_RPY[::-1]

    class control_allocator_config:
        num_motors = 8
        force_application_level = "motor_link"
        application_mask = [1 + 8 + i for i in range(8)]
        motor_directions = [1, -1, 1, -1, 1, -1, 1, -1]
        _a, _b, _c = 0.78867513, 0.21132487, 0.57735027
        _d, _e, _f, _g = 0.14226497, 0.21547005, 0.25773503, 0.01547005
        _h, _i = 0.11547005, 0.23094011
        allocation_matrix = [
            [-_a, _b, -_b, _a, _a, -_b, _b, -_a],
            [_b, _a, -_a, -_b, -_b, -_a, _a, _b],
            [_c, -_c, -_c, _c, _c, -_c, -_c, _c],
            [_d, -_e, _f, _g, -_g, -_f, _e, -_d],
            [-_f, _g, _d, _e, -_e, -_d, -_g, _f],
            [_h, -_i, -_h, _i, -_i, _h, _i, -_h],
        ]

        class motor_model_config:
            use_rps = False
            motor_thrust_constant_min, motor_thrust_constant_max = 0.00000926312, 0.00001826312
            motor_time_constant_increasing_min, motor_time_constant_increasing_max = 0.01, 0.03
            motor_time_constant_decreasing_min = motor_time_constant_decreasing_max = 0.005
            max_thrust, min_thrust = 6.25, -6.25
            max_thrust_rate = 100000.0
            thrust_to_torque_ratio = 0.01
            use_discrete_approximation = True


class BaseOctarotorWithLidar32x512Cfg(BaseOctarotorCfg):
    class sensor_config(BaseOctarotorCfg.sensor_config):
        enable_lidar = True
        lidar_config = Lidar32x512Config


class BaseROVCfg:  # base_rov_config.py:14-241, resources/robots/BlueROV/rov.urdf -- the robot of examples/position_control_example_rov.py
    """The reference's fully actuated ROV (robots/base_rov.py: BaseROV).  Its URDF is the octarotor's with another visual mesh: a
    0.3 kg base link, eight massless arm links half way out and eight 0.1 kg thruster links at (+-s, +-s, +-s), s = 0.1732 m,
    posed with xyz AND rpy -- a thruster pushes along its link's z axis, at the link's position.  All four drag coefficient
    triples are zero as in the reference; the class that reads them (BaseROV) applies the quadratic linear term per axis.
    Pinned by tests/golden/robot_base_rov.npz (composite of the reference's URDF)."""

    class init_config:
        min_init_state = [0.0, 0.0, 0.0, 0, 0, -_PI, 1.0, -0.2, -0.2, -0.2, -0.2, -0.2, -0.2]
        max_init_state = [1.0, 1.0, 1.0, 0, 0, _PI, 1.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2]

    class sensor_config:
        enable_camera = False
        camera_config = BaseDepthCameraConfig
        enable_lidar = False
        lidar_config = BaseLidarConfig
        enable_imu = False
        imu_config = BaseImuConfig

    class damping:  # along the body x, y, z axes
        linvel_linear_damping_coefficient = [0.0, 0.0, 0.0]
        linvel_quadratic_damping_coefficient = [0.0, 0.0, 0.0]
        angular_linear_damping_coefficient = [0.0, 0.0, 0.0]
        angular_quadratic_damping_coefficient = [0.0, 0.0, 0.0]

    class disturbance:
        enable_disturbance = True
        prob_apply_disturbance = 0.05
        max_force_and_torque_disturbance = [1.5, 1.5, 1.5, 0.25, 0.25, 0.25]

    class robot_asset(_CommonAsset):
        file = "rov.urdf"
        name = "base_rov"
        angular_damping = 0.0000001
        linear_damping = 0.0000001

    class robot_model:  # resources/robots/BlueROV/rov.urdf
        base_mass = 0.3
        base_inertia = [[0.048000000000000015, 0, 0], [0, 0.048000000000000015, 0], [0, 0, 0.048000000000000015]]
        collision_sphere_radius = 0.30000000000000004
        motor_mass = 0.1
        motor_xyz = [[sx * _S, sy * _S, sz * _S] for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)]
        motor_rpy = _OCTA_RPY + _OCTA_RPY[::-1]

    class control_allocator_config:
        num_motors = 8
        force_application_level = "motor_link"
        application_mask = [1 + 8 + i for i in range(8)]
        motor_directions = [1, -1, 1, -1, 1, -1, 1, -1]
        allocation_matrix = [
            [-0.78867513, 0.21132487, -0.21132487, 0.78867513, 0.78867513, -0.21132487, 0.21132487, -0.78867513],
            [0.21132487, 0.78867513, -0.78867513, -0.21132487, -0.21132487, -0.78867513, 0.78867513, 0.21132487],
            [0.57735027, -0.57735027, -0.57735027, 0.57735027, 0.57735027, -0.57735027, -0.57735027, 0.57735027],
            [0.14226497, -0.21547005, 0.25773503, 0.01547005, -0.01547005, -0.25773503, 0.21547005, -0.14226497],
            [-0.25773503, 0.01547005, 0.14226497, 0.21547005, -0.21547005, -0.14226497, -0.01547005, 0.25773503],
            [0.11547005, -0.23094011, -0.11547005, 0.23094011, -0.23094011, 0.11547005, 0.23094011, -0.11547005],
        ]

        class motor_model_config:
            use_rps = False
            motor_thrust_constant_min, motor_thrust_constant_max = 0.00000926312, 0.00001826312
            motor_time_constant_increasing_min, motor_time_constant_increasing_max = 0.01, 0.03
            motor_time_constant_decreasing_min = motor_time_constant_decreasing_max = 0.005
            max_thrust, min_thrust = 6.25, -6.25
            max_thrust_rate = 100000.0
            thrust_to_torque_ratio = 0.01
            use_discrete_approximation = True


class MagpieCfg:  # magpie_config.py:15-176, resources/robots/magpie/model.urdf
    class init_config:
        min_init_state = [0.1, 0.15, 0.15, 0, 0, -_PI, 1.0, -0.2, -0.2, -0.2, -0.2, -0.2, -0.2]
        max_init_state = [0.2, 0.85, 0.85, 0, 0, _PI, 1.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2]

    class sensor_config:
        enable_camera = False
        camera_config = BaseDepthCameraConfig
        enable_lidar = True
        lidar_config = RSLidar_Airy_Config
        enable_imu = False
        imu_config = None

    class disturbance:
        enable_disturbance = True
        prob_apply_disturbance = 0.05
        max_force_and_torque_disturbance = [4.75, 4.75, 4.75, 0.03, 0.03, 0.03]

    class damping:
        linvel_linear_damping_coefficient = [0.0, 0.0, 0.0]
        linvel_quadratic_damping_coefficient = [0.0, 0.0, 0.0]
        angular_linear_damping_coefficient = [0.0, 0.0, 0.0]
        angular_quadratic_damping_coefficient = [0.0, 0.0, 0.0]

    class robot_asset(_CommonAsset):
        file = "model.urdf"
        name = "base_quadrotor"
        collapse_fixed_joints = True  # the prop joints carry dont_collapse="true": 5 bodies remain
        angular_damping = 0.01
        linear_damping = 0.01
        min_state_ratio, max_state_ratio = _state_ratio([0.1, 0.1, 0.1], [0.9, 0.9, 0.9], _PI)

    class robot_model:  # model.urdf: base 1.2 kg + 4 props of 10 g at (+-0.1, +-0.1, 0)
        base_mass = 1.2
        base_inertia = [[0.013, 0, 0], [0, 0.014, 0], [0, 0, 0.013]]
        # the URDF collision shape is a 0.7 x 0.7 x 0.5 box; the collision model here is a sphere (DESIGN.md
        # "Collision"): radius = half the box width
        collision_sphere_radius = 0.35
        motor_mass = 0.01
        motor_inertia = 0.000001
        motor_xyz = [[0.1, 0.1, 0.0], [0.1, -0.1, 0.0], [-0.1, -0.1, 0.0], [-0.1, 0.1, 0.0]]
        motor_rpy = [[0.0, 0.0, 0.0]] * 4

    class control_allocator_config:
        num_motors = 4
        force_application_level = "base_link"  # not "motor_link": the combined wrench A u acts on the root link
        application_mask = [1 + 4 + i for i in range(4)]
        motor_directions = [1, -1, 1, -1]
        allocation_matrix = [
            [0.0, 0.0, 0.0, 0.0],
            [0.0, 0.0, 0.0, 0.0],
            [1.0, 1.0, 1.0, 1.0],
            [-0.13, -0.13, 0.13, 0.13],
            [-0.13, 0.13, 0.13, -0.13],
            [-0.02, 0.02, -0.02, 0.02],
        ]

        class motor_model_config:
            use_rps = True
            motor_thrust_constant_min, motor_thrust_constant_max = 0.00000926312, 0.00001826312
            motor_time_constant_increasing_min, motor_time_constant_increasing_max = 0.01, 0.02
            motor_time_constant_decreasing_min, motor_time_constant_decreasing_max = 0.005, 0.015
            max_thrust, min_thrust = 12.0, 0.1
            max_thrust_rate = 1000000.0
            thrust_to_torque_ratio = 0.02
            use_discrete_approximation = True


class LMF2Cfg(MagpieCfg):  # lmf2_config.py:18-180, resources/robots/lmf2/model.urdf -- the robot of the reference's default navigation recipe
    """The reference's `navigation_task` default (navigation_task_config.py:9-10: lmf2 + lmf2_velocity_control).  Same airframe
    layout as magpie in the URDF (base 1.2 kg + four 10 g props at (+-0.1, +-0.1, 0), fixed joints kept: 5 bodies); the
    allocator applies the combined wrench at the root body (force_application_level "base_link": anything but "motor_link",
    control_allocation.py:53-65).  Pinned by tests/golden/robot_lmf2.npz (composite of the reference's URDF)."""

    class init_config:
        min_init_state = [0.1, 0.15, 0.15, 0, 0, -_PI / 6, 1.0, -0.2, -0.2, -0.2, -0.2, -0.2, -0.2]
        max_init_state = [0.2, 0.85, 0.85, 0, 0, _PI / 6, 1.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2]

    class sensor_config:
        enable_camera = True
        camera_config = BaseDepthCameraConfig  # 135 x 240 depth + segmentation
        enable_lidar = False
        lidar_config = BaseLidarConfig
        enable_imu = False
        imu_config = None

    class robot_model(MagpieCfg.robot_model):
        # the URDF collision shape is a 0.5 m cube; the collision model here is a sphere of half its width (DESIGN.md "Collision")
        collision_sphere_radius = 0.25

    class control_allocator_config:
        num_motors = 4
        force_application_level = "base_link"
        application_mask = [1 + 4 + i for i in range(4)]
        motor_directions = [1, -1, 1, -1]
        allocation_matrix = [
            [0.0, 0.0, 0.0, 0.0],
            [0.0, 0.0, 0.0, 0.0],
            [1.0, 1.0, 1.0, 1.0],
            [-0.13, -0.13, 0.13, 0.13],
            [-0.13, 0.13, 0.13, -0.13],
            [-0.07, 0.07, -0.07, 0.07],
        ]

        class motor_model_config:
            use_rps = True
            motor_thrust_constant_min, motor_thrust_constant_max = 0.00000926312, 0.00001826312
            motor_time_constant_increasing_min, motor_time_constant_increasing_max = 0.05, 0.08
            motor_time_constant_decreasing_min, motor_time_constant_decreasing_max = 0.005, 0.005
            max_thrust, min_thrust = 10.0, 0.1
            max_thrust_rate = 100000.0
            thrust_to_torque_ratio = 0.07
            use_discrete_approximation = True


class LMF2With64x48CameraCfg(LMF2Cfg):
    """lmf2 with the 64 x 48 camera of BASELINE configs[2] instead of its 135 x 240 one"""

    class sensor_config(LMF2Cfg.sensor_config):
        camera_config = DepthCamera64x48Config


class LMF2RadarCfg(LMF2Cfg):  # lmf2_radar_config.py:18-180: lmf2_config.py with the camera off and the fake radar on, nothing else
    """The robot of the reference's `radar_navigation_task` (radar_navigation_task_config.py:9-11)."""

    class sensor_config(LMF2Cfg.sensor_config):
        enable_camera = False
        enable_lidar = True
        lidar_config = fake_radar_config


class BaseQuadRootLinkControlCfg(BaseQuadCfg):  # base_quad_root_link_control_config.py:18-53
    """base_quadrotor with the allocator's wrench applied at the root link.  (The reference points this config at
    resources/robots/quad/model.urdf -- the lmf2-style 1.2 kg body; the rigid-body constants here are that URDF's.)"""

    class robot_asset(BaseQuadCfg.robot_asset):
        file = "model.urdf"
        collapse_fixed_joints = False

    class robot_model(MagpieCfg.robot_model):
        collision_sphere_radius = 0.2  # the URDF collision shape is a 0.4 m cube

    class control_allocator_config(BaseQuadCfg.control_allocator_config):
        force_application_level = "root_link"

        class motor_model_config(BaseQuadCfg.control_allocator_config.motor_model_config):
            motor_thrust_constant_min, motor_thrust_constant_max = 0.00001826312, 0.00001826312
            motor_time_constant_increasing_min, motor_time_constant_increasing_max = 0.01, 0.03
            motor_time_constant_decreasing_min, motor_time_constant_decreasing_max = 0.005, 0.005
            max_thrust, min_thrust = 10, 0


_TINYPROP_ARM_RPY = [  # joints base_link_to_arm_motor_0..3 of tinyprop.urdf
    [-1.5707963267948968, 2.220446049250313e-16, -2.3561944901923453],
    [1.5707963267948968, 2.220446049250313e-16, -0.7853981633974482],
    [1.5707963267948968, 0.0, -2.3561944901923453],
    [-1.5707963267948968, 0.0, -0.7853981633974482],
]
_TINYPROP_ARM_XYZ = [[0.08, -0.08, 0.0], [-0.08, -0.08, 0.0], [-0.08, 0.08, 0.0], [0.08, 0.08, 0.0]]


class TinyPropCfg:  # tinyprop_config.py:15-166, resources/robots/tinyprop/tinyprop.urdf -- the airframe of the end-to-end task
    """The robot the reference trains motor-command policies for (position_setpoint_task_sim2real_end_to_end, `no_control`: the
    action IS the four thrusts, clamped to 0.2 .. 1.2 N by the motor model).  The first airframe here with products of inertia:
    the base link's tensor is full, the arm links are rotated and the prop links carry full tensors.  Pinned by
    tests/golden/robot_tinyprop.npz (composite of the reference's URDF)."""

    class init_config:
        min_init_state = [-0.7, -0.7, -0.7, -_PI / 6, -_PI / 6, -_PI, 1.0, -0.5, -0.5, -0.5, -0.5, -0.5, -0.5]
        max_init_state = [0.7, 0.7, 0.7, _PI / 6, _PI / 6, _PI, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]

    class sensor_config:
        enable_camera = False
        camera_config = BaseDepthCameraConfig
        enable_lidar = False
        lidar_config = BaseLidarConfig
        enable_imu = False
        imu_config = BaseImuConfig

    class disturbance:
        enable_disturbance = False
        prob_apply_disturbance = 0.02
        max_force_and_torque_disturbance = [0.001, 0.001, 0.001, 0.00004, 0.00004, 0.00004]

    class damping:
        linvel_linear_damping_coefficient = [0.0, 0.0, 0.0]
        linvel_quadratic_damping_coefficient = [0.0, 0.0, 0.0]
        angular_linear_damping_coefficient = [0.0, 0.0, 0.0]
        angular_quadratic_damping_coefficient = [0.0, 0.0, 0.0]

    class robot_asset(_CommonAsset):
        file = "tinyprop.urdf"
        name = "tinyprop"
        angular_damping = 0.01
        linear_damping = 0.01

    class robot_model:  # tinyprop.urdf: base 0.321 kg, four 13 g props at (+-0.16, +-0.16, 0), four 1 mg arm links half way out
        base_mass = 0.321
        base_inertia = [[0.0015914, -0.0000044, 0.0000001], [-0.0000044, 0.0015312, 0.0000031], [0.0000001, 0.0000031, 0.0025329]]
        # the URDF collision shape is a 0.11 m cube; the collision model here is a sphere of half its width (DESIGN.md "Collision")
        collision_sphere_radius = 0.055
        motor_mass = 0.013
        motor_inertia = [[2e-6, 1e-9, 1e-9], [1e-9, 2e-6, 1e-9], [1e-9, 1e-9, 3e-6]]
        motor_xyz = [[0.16, -0.16, 0.0], [-0.16, -0.16, 0.0], [-0.16, 0.16, 0.0], [0.16, 0.16, 0.0]]
        motor_rpy = [[0.0, 0.0, 0.0]] * 4
        # every joint of this URDF hangs off base_link; `parent` is what composite_body follows
        links = [dict(name="arm_motor_%d" % j, parent="base_link", mass=0.000001, xyz=_TINYPROP_ARM_XYZ[j], rpy=_TINYPROP_ARM_RPY[j],
                      inertia=[[1e-9] * 3] * 3) for j in range(4)]

    class control_allocator_config:
        num_motors = 4
        force_application_level = "motor_link"
        application_mask = [5, 6, 7, 8]
        motor_directions = [1, -1, 1, -1]
        allocation_matrix = [
            [0.0, 0.0, 0.0, 0.0],
            [0.0, 0.0, 0.0, 0.0],
            [1.0, 1.0, 1.0, 1.0],
            [-0.16, -0.16, 0.16, 0.16],
            [-0.16, 0.16, 0.16, -0.16],
            [-0.01, 0.01, -0.01, 0.01],
        ]

        class motor_model_config:
            use_rps = True
            motor_thrust_constant_min = motor_thrust_constant_max = 0.00001286412
            motor_time_constant_increasing_min = motor_time_constant_increasing_max = 0.047
            motor_time_constant_decreasing_min = motor_time_constant_decreasing_max = 0.047
            max_thrust, min_thrust = 1.2, 0.2
            max_thrust_rate = 100000.0
            thrust_to_torque_ratio = 0.01
            use_discrete_approximation = True
            integration_scheme = "rk4"


class LMF1Cfg(MagpieCfg):  # lmf1_config.py:15-176, resources/robots/lmf1/model.urdf
    """lmf2's predecessor: the same airframe layout with a 1.195 kg base link, forces applied at the four prop links, no sensors
    and no disturbance.  The URDF's fixed joints are kept (5 bodies, ordered by link name: back_left, back_right, front_left,
    front_right), so allocator column j is body application_mask[j] -- front right, back left, front left, back right.  Its
    centre of mass is the base-link origin.  Pinned by tests/golden/robot_lmf1.npz (composite of the reference's URDF)."""

    class init_config:
        min_init_state = [0.0, 0.0, 0.0, -_PI / 6, -_PI / 6, -_PI, 1.0, -0.5, -0.5, -0.5, -0.2, -0.2, -0.2]
        max_init_state = [1.0, 1.0, 1.0, _PI / 6, _PI / 6, _PI, 1.0, 0.5, 0.5, 0.5, 0.2, 0.2, 0.2]

    class sensor_config:
        enable_camera = False
        camera_config = BaseDepthCameraConfig
        enable_lidar = False
        lidar_config = BaseLidarConfig
        enable_imu = False
        imu_config = BaseImuConfig

    class disturbance:
        enable_disturbance = False
        prob_apply_disturbance = 0.0
        max_force_and_torque_disturbance = [0, 0, 0, 0, 0, 0]

    class robot_asset(_CommonAsset):
        file = "model.urdf"
        name = "base_quadrotor"
        collision_mask = 1
        angular_damping = 0.02
        linear_damping = 0.02
        armature = 0.00001
        min_state_ratio = [0.1, 0.1, 0.1, 0, 0, -_PI, 1.0, 0, 0, 0, 0, 0, 0]
        max_state_ratio = [0.9, 0.9, 0.9, 0, 0, _PI, 1.0, 0, 0, 0, 0, 0, 0]

    class robot_model(MagpieCfg.robot_model):  # model.urdf: base 1.195 kg + 4 props of 10 g at (+-0.1, +-0.1, 0)
        base_mass = 1.195
        # the URDF collision shape is a 0.5 m cube; the collision model here is a sphere of half its width (DESIGN.md "Collision")
        collision_sphere_radius = 0.25
        motor_xyz = [[0.1, -0.1, 0.0], [-0.1, 0.1, 0.0], [0.1, 0.1, 0.0], [-0.1, -0.1, 0.0]]  # in allocator-column order

    class control_allocator_config:
        num_motors = 4
        force_application_level = "motor_link"
        application_mask = [4, 1, 3, 2]  # front right, back left, front left, back right
        motor_directions = [1, 1, -1, -1]
        allocation_matrix = [
            [0.0, 0.0, 0.0, 0.0],
            [0.0, 0.0, 0.0, 0.0],
            [1.0, 1.0, 1.0, 1.0],
            [-0.13, 0.13, 0.13, -0.13],
            [-0.13, 0.13, -0.13, 0.13],
            [-0.05, 0.05, -0.05, 0.05],
        ]

        class motor_model_config:
            use_rps = True
            motor_thrust_constant_min = motor_thrust_constant_max = 5.487e-6
            motor_time_constant_increasing_min = motor_time_constant_increasing_max = 0.025
            motor_time_constant_decreasing_min = motor_time_constant_decreasing_max = 0.025
            max_thrust, min_thrust = 20.0, 0.0
            max_thrust_rate = 100000.0
            thrust_to_torque_ratio = 0.05
            use_discrete_approximation = False


class BaseRandCfg:  # base_random_config.py:14-227, resources/robots/random/random.urdf
    """The reference's showcase of an arbitrary configuration: eight motors at arbitrary poses around a base link with a full
    inertia tensor.  The composite's centre of mass lies at (22.44, 1.75, -2.63) mm from the base-link origin, so this airframe
    flies through agx_env_step_com (DESIGN.md "integrator").  `allocation_matrix` is the reference's, which it computed about the
    base-link ORIGIN: the controller is slightly wrong about the airframe it flies, as on the reference.  motor_j is URDF link
    motor_j and allocator column j; the eight massless arm_motor_j links carry nothing and are left out.  Pinned by
    tests/golden/robot_base_random.npz (composite of the reference's URDF)."""

    class init_config:
        min_init_state = [0.0, 0.0, 0.0, 0, 0, -_PI, 1.0, -0.2, -0.2, -0.2, -0.2, -0.2, -0.2]
        max_init_state = [1.0, 1.0, 1.0, 0, 0, _PI, 1.0, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2]

    class sensor_config:
        enable_camera = False
        camera_config = BaseDepthCameraConfig
        enable_lidar = False
        lidar_config = BaseLidarConfig
        enable_imu = False
        imu_config = BaseImuConfig

    class disturbance:
        enable_disturbance = True
        prob_apply_disturbance = 0.05
        max_force_and_torque_disturbance = [1.5, 1.5, 1.5, 0.25, 0.25, 0.25]

    class damping:
        linvel_linear_damping_coefficient = [0.0, 0.0, 0.0]
        linvel_quadratic_damping_coefficient = [0.0, 0.0, 0.0]
        angular_linear_damping_coefficient = [0.0, 0.0, 0.0]
        angular_quadratic_damping_coefficient = [0.0, 0.0, 0.0]

    class robot_asset(_CommonAsset):
        file = "random.urdf"
        name = "base_random"
        angular_damping = 0.0000001
        linear_damping = 0.0000001
        min_state_ratio = [0.1, 0.1, 0.1, 0, 0, -_PI, 1.0, -0.5, -0.5, -0.5, -0.2, -0.2, -0.2]
        max_state_ratio = [0.3, 0.9, 0.9, 0, 0, _PI, 1.0, 0.5, 0.5, 0.5, 0.2, 0.2, 0.2]

    class robot_model:  # random.urdf: base 0.225 kg with a full tensor, eight 3.125 g motor links without inertia of their own
        base_mass = 0.225
        base_inertia = [[0.001425189394784859, -0.00026658913320567757, 0.00039128491940189244],
                        [-0.00026658913320567757, 0.0022903263103270237, -0.00025018840733648744],
                        [0.00039128491940189244, -0.00025018840733648744, 0.0021842657051118833]]
        collision_sphere_radius = 0.47291274518274684
        motor_mass = 0.0031249999999999993
        motor_xyz = [
            [0.2824873734152916, -0.0724873734152916, -0.175],
            [0.21, -0.24499999999999997, -0.27999999999999997],
            [0.03748737341529165, -0.1424873734152916, 0.034999999999999996],
            [0.315, 0.13999999999999999, -0.06999999999999999],
            [0.3524873734152916, 0.28248737341529156, -0.13999999999999999],
            [0.13999999999999999, 0.13999999999999999, 0.27999999999999997],
            [0.14248737341529163, 0.0724873734152916, 0.175],
            [0.315, -0.034999999999999996, -0.034999999999999996],
        ]
        motor_rpy = [
            [-1.5707963267948961, 0.8726646259971647, 1.7272004125383903e-16],
            [-2.792526803190927, -0.34906585039886595, -3.141592653589793],
            [0.7853981633974484, -0.6981317007977318, -3.623233072825522e-17],
            [0.0, -0.34906585039886573, 0.0],
            [0.1745329251994329, 1.3962634015954642, 0.0],
            [-1.2217304763960306, 1.5707963267948966, 0.0],
            [-0.5235987755982989, 1.5707963267948966, 0.0],
            [0.17453292519943295, -0.8726646259971649, 0.0],
        ]

    class control_allocator_config:
        num_motors = 8
        force_application_level = "motor_link"
        application_mask = [1 + 8 + i for i in range(8)]
        motor_directions = [-1, 1, -1, 1, -1, 1, -1, 1]
        allocation_matrix = [
            [5.55111512e-17, -3.21393805e-01, -4.54519478e-01, -3.42020143e-01, 9.69846310e-01, 3.42020143e-01, 8.66025404e-01, -7.54406507e-01],
            [1.00000000e00, -3.42020143e-01, -7.07106781e-01, 0.00000000e00, -1.73648178e-01, 9.39692621e-01, 5.00000000e-01, -1.73648178e-01],
            [1.66533454e-16, -8.83022222e-01, 5.41675220e-01, 9.39692621e-01, 1.71010072e-01, 1.11022302e-16, 1.11022302e-16, 6.33022222e-01],
            [1.75000000e-01, 1.23788742e-01, -5.69783368e-02, 1.34977168e-01, 3.36959042e-02, -2.66534135e-01, -7.88397460e-02, -2.06893989e-02],
            [1.00000000e-02, 2.78845133e-01, -4.32852308e-02, -2.72061766e-01, -1.97793856e-01, 8.63687139e-02, 1.56554446e-01, -1.71261290e-01],
            [2.82487373e-01, -1.41735490e-01, -8.58541103e-02, 3.84858939e-02, -3.33468026e-01, 8.36741468e-02, 8.46777988e-03, -8.74336259e-02],
        ]

        class motor_model_config:
            use_rps = False
            motor_thrust_constant_min, motor_thrust_constant_max = 0.00000926312, 0.00001826312
            motor_time_constant_increasing_min, motor_time_constant_increasing_max = 0.01, 0.03
            motor_time_constant_decreasing_min, motor_time_constant_decreasing_max = 0.005, 0.005
            max_thrust, min_thrust = 5.0, -5.0
            max_thrust_rate = 100000.0
            thrust_to_torque_ratio = 0.01
            use_discrete_approximation = True
