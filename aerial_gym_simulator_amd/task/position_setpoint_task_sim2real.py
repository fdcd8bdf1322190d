"""The two set-point tasks the reference trains for the real lmf2, with the reference's API, attributes and step ordering:
PositionSetpointTaskSim2Real (aerial_gym/task/position_setpoint_task_sim2real/position_setpoint_task_sim2real.py:20-259,
velocity commands) and PositionSetpointTaskAccelerationSim2Real (aerial_gym/task/
position_setpoint_task_acceleration_sim2real/position_setpoint_task_acceleration_sim2real.py:20-273, acceleration commands,
doubled in the caller's tensor).  Per step() the task side is agx_sim2real_pre_step, agx_sim2real_reward, one normal fill
and agx_sim2real_obs (csrc/agx_sim2real.hip) around EnvManager.step and the reset launch."""
import torch

from .. import _lib
from ..utils.logging import CustomLogger
from ..utils import roctx
from .setpoint_task_base import SetpointTaskBase

logger = CustomLogger("position_setpoint_task")

NOISE_TAGS = ("sim2real_obs_noise_euler", "sim2real_obs_noise_pos", "sim2real_obs_noise_linvel", "sim2real_obs_noise_angvel")


class PositionSetpointTaskSim2Real(SetpointTaskBase):
    KIND = _lib.SIM2REAL_VELOCITY
    OBSERVATION_SPACE_SHAPE = (13,)  # (sic: :95-97)

    def __init__(self, task_config, seed=None, num_envs=None, headless=None, device=None, use_warp=None):
        logger.info("Building environment for position setpoint task.")
        super().__init__(task_config, seed, num_envs, headless, device, use_warp)
        cfg, N, dev = self.task_config, self.num_envs, self.device
        for key in cfg.reward_parameters.keys():
            cfg.reward_parameters[key] = torch.tensor(cfg.reward_parameters[key], device=dev)
        if cfg.action_space_dim != 4 or cfg.observation_space_dim != 17 or self.sim_env.num_robot_actions != 4:
            raise ValueError("the sim2real set-point tasks have 4-D actions and 17-D observations (task_config.action_space_dim, "
                             "observation_space_dim, the controller's num_actions)")
        self.prev_actions_vehicle_frame = torch.zeros_like(self.actions)  # (read and written by the acceleration task only)
        self.actions_vehicle_frame = torch.zeros_like(self.actions)
        self.prev_dist = torch.zeros(N, device=dev)
        # standard normals of the observation noise, [4][N][3] in the reference's randn_like order (:209-222)
        self.obs_noise = torch.zeros((4, N, 3), device=dev)

    def _check_actions(self, actions):
        """The tasks keep the caller's tensor (`self.actions = actions`) and the acceleration task doubles it in place: it has to
        be the device tensor the kernels can take as it is."""
        if not (isinstance(actions, torch.Tensor) and actions.dtype is torch.float32 and actions.is_contiguous()
                and tuple(actions.shape) == (self.num_envs, 4) and actions.device == self.actions.device):
            raise ValueError(f"actions must be a contiguous float32 tensor of shape ({self.num_envs}, 4) on {self.actions.device}: "
                             "the task keeps a reference to it and reads it again at the next step")

    @roctx.ranged("PositionSetpointTaskSim2Real.step")
    def step(self, actions):
        env = self.sim_env
        env._require_device()
        self._check_actions(actions)
        self.counter += 1
        # prev_actions[:] = actions (as that tensor reads now); prev_dist on the pre-step position; acceleration: previous action
        # in the vehicle frame, incoming action doubled in the caller's tensor
        _lib.check(
            env._lib.agx_sim2real_pre_step(self.KIND, env._buffers, env.num_envs, _lib.dptr(self.target_soa), _lib.dptr(self.actions),
                                           _lib.dptr(actions), _lib.dptr(self.prev_actions), _lib.dptr(self.prev_dist),
                                           _lib.dptr(self.prev_actions_vehicle_frame), env._stream()),
            "agx_sim2real_pre_step",
        )
        self.actions = actions
        return self._step_env_and_return()

    def _draw_obs_noise(self):
        env, z = self.sim_env, self.obs_noise
        if env.strict_rng:  # four randn_like calls on [N, 3], in the reference's order: the torch stream is consumed as there
            for k, tag in enumerate(NOISE_TAGS):
                env.random_source.normal_into(z[k], tag=tag)
        else:
            env.random_source.normal_into(z, tag="sim2real_obs_noise")

    def process_obs_for_task(self):
        env = self.sim_env
        env._require_device()
        self._draw_obs_noise()
        _lib.check(
            env._lib.agx_sim2real_obs(env._buffers, env.num_envs, _lib.dptr(self.target_soa), _lib.dptr(self.obs_noise),
                                      _lib.dptr(self.task_obs["observations"]), env._stream()),
            "agx_sim2real_obs",
        )
        self._publish_step_flags()

    def compute_rewards_and_crashes(self, obs_dict):
        """compute_reward, the distance crash, `truncations = sim_steps > episode_len_steps` and the step's reset set"""
        env = self.sim_env
        env._require_device()
        _lib.check(
            env._lib.agx_sim2real_reward(self.KIND, env._buffers, env.num_envs, _lib.dptr(self.target_soa), _lib.dptr(self.actions),
                                         _lib.dptr(self.prev_actions), _lib.dptr(self.prev_dist),
                                         _lib.dptr(self.actions_vehicle_frame), _lib.dptr(self.prev_actions_vehicle_frame),
                                         int(self.task_config.episode_len_steps), int(env.cfg.env.reset_on_collision),
                                         _lib.dptr(self.rewards), env._stream()),
            "agx_sim2real_reward",
        )
        env.mark_produced(env.RESET_SET)  # the reward kernel wrote this step's reset set
        return self.rewards, self.terminations


class PositionSetpointTaskAccelerationSim2Real(PositionSetpointTaskSim2Real):
    KIND = _lib.SIM2REAL_ACCELERATION
