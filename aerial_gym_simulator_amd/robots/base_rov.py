"""Host mirror of aerial_gym/robots/base_rov.py: the fully actuated ROV, a rigid body with eight fixed thruster links.

It differs from BaseMultirotor in three places, all of them in the kernels (AGX_LAUNCH_ROV, include/aerial_gym_hip.h):
  * simulate_drag (base_rov.py:260-285): the quadratic drag on the linear velocity is per axis, -c_q[k] |v_body[k]| v_body[k];
  * update_states (base_rov.py:251-258): robot_euler_angles holds get_euler_xyz_tensor(q) as it is, in [0, 2 pi), without ssa();
  * reset_idx (base_rov.py:171-198): the control allocator is not reset -- motor thrusts and motor constants of a resetting env
    stay as they are and no motor draws are consumed.
Everything else, the plug-in contract included (a registered subclass that overrides step() is called once per physics sub-step
and reaches the built-in step through super().step(action)), is BaseMultirotor's.
"""
import torch

from .._lib import LAUNCH_ROV
from ..utils.logging import CustomLogger
from .base_multirotor import BaseMultirotor

logger = CustomLogger("base_rov")

_ROV_LAWS = ("fully_actuated", "none", "wrench")  # the laws that read no Euler angles


class BaseROV(BaseMultirotor):
    LAUNCH_FLAGS = LAUNCH_ROV  # EnvManager ORs this into AgxEnvBuffers.launch_flags of every launch

    def __init__(self, robot_config, controller_name, env_config, device):
        super().__init__(robot_config, controller_name, env_config, device)
        logger.warning(f"Creating {self.num_envs} ROVs.")
        self.output_forces = None
        self.output_torques = None

    def init_tensors(self, global_tensor_dict):
        super().init_tensors(global_tensor_dict)
        g, dev = global_tensor_dict, self.device
        kind = self.params_dict["controller"]
        if kind not in _ROV_LAWS or self.params_dict["num_motors"] != 8:
            raise ValueError(
                f"BaseROV with controller '{self.controller_name}' ({self.params_dict['num_motors']} motors): the ROV kernels are built "
                "for eight thrusters under the fully actuated law, no_control or an external controller class -- its Euler angles "
                "are not wrapped to (-pi, pi], which the Lee controllers with Euler-angle feedback assume")
        if self.com_offset is not None:
            raise ValueError(f"BaseROV with a centre of mass at {self.params_dict['com']} m from the base-link origin: the ROV kernels "
                             "(AGX_LAUNCH_ROV) carry no centre-of-mass offset")
        d = self.cfg.damping
        self.body_vel_linear_damping_coefficient = torch.tensor(d.linvel_linear_damping_coefficient, device=dev)
        self.body_vel_quadratic_damping_coefficient = torch.tensor(d.linvel_quadratic_damping_coefficient, device=dev)
        self.angvel_linear_damping_coefficient = torch.tensor(d.angular_linear_damping_coefficient, device=dev)
        self.angvel_quadratic_damping_coefficient = torch.tensor(d.angular_quadratic_damping_coefficient, device=dev)
        ca = self.cfg.control_allocator_config
        mask = ca.application_mask if self.force_application_level == "motor_link" else [0]
        self.application_mask = torch.tensor(mask, device=dev)
        self.motor_directions = torch.tensor(ca.motor_directions, device=dev)
        # what the reference's control_allocation() fills before it copies them into robot_force_tensors / robot_torque_tensors
        # (base_rov.py:229-249); agx_robot_step writes the per-body tensors themselves, these stay the zero-initialised scratch
        self.output_forces = torch.zeros_like(g["robot_force_tensor"])
        self.output_torques = torch.zeros_like(g["robot_torque_tensor"])
