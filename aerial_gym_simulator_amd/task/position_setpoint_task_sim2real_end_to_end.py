"""The set-point task whose policy commands the four motor thrusts directly, with the reference's API, attributes and step ordering:
PositionSetpointTaskSim2RealEndToEnd (aerial_gym/task/position_setpoint_task_sim2real_end_to_end/
position_setpoint_task_sim2real_end_to_end.py:20-252; tinyprop + no_control, 15-D observation with a 6-D rotation).

Per step(), default mode, four launches and no host synchronisation: agx_end_to_end_pre_step (action rescale, prev_position), the env
step, agx_end_to_end_reward (reward, flags, reset set) and agx_post_step_end_to_end (masked reset + observation with device-generator
noise + prev_actions / prev_pos_error), csrc/agx_dyn_end_to_end.h.  `return_state_before_reset`, an explicit reset() and
get_return_tuple() by hand take the general path: agx_end_to_end_obs on its own and the env manager's own reset."""
import torch

from .. import _lib
from ..config import task_config as task_config_module
from ..tensors import aos_view, soa
from ..utils.logging import CustomLogger
from ..utils import roctx
from .setpoint_task_base import SetpointTaskBase

logger = CustomLogger("position_setpoint_task")

# the four torch.normal draws of process_obs_for_task, in its order (:207-218)
NOISE_TAGS = ("end_to_end_obs_noise_pos", "end_to_end_obs_noise_orientation", "end_to_end_obs_noise_linvel", "end_to_end_obs_noise_angvel")

# compute_reward's constants (:267-309), one table per task of this family: the px4 sibling is another entry
REWARD_CONSTANTS = {
    "end_to_end": dict(z_error_weight=11.0, pos_gain=(10.0, 2.0), pos_exp=(10.0, 2.0), upright_gain=2.5, upright_exp=5.0,
                       alignment_gain=6.0, alignment_exp=5.0, angvel_gain=0.3, angvel_exp=10.0, vel_gain=1.0, vel_exp=5.0,
                       hover_thrust=9.81 * 0.372 / 4, action_gain=0.01, action_exp=10.0, closer_gain=10.0, farther_gain=15.0,
                       diff_gain=1.3, diff_exp=6.0, divisor=100.0),
}


def reward_constants(name):
    K = _lib.AgxEndToEndReward()
    for key, value in REWARD_CONSTANTS[name].items():
        if isinstance(value, tuple):
            for j, v in enumerate(value):
                getattr(K, key)[j] = v
        else:
            setattr(K, key, value)
    return K


class PositionSetpointTaskSim2RealEndToEnd(SetpointTaskBase):
    REWARD = "end_to_end"
    # (obs_noise holds draws that are taken anew before every read: not state)
    SNAPSHOT_TENSORS = (("target_soa", "soa"), ("rewards", "soa"), ("task_obs[observations]", "aos"), ("task_obs[collisions]", "aos"),
                        ("actions", "aos"), ("prev_actions", "aos"), ("action_history", "aos"), ("prev_position_soa", "soa"),
                        ("prev_pos_error_soa", "soa"))
    SNAPSHOT_HOST = ("counter",)

    def __init__(self, task_config, seed=None, num_envs=None, headless=None, device=None, use_warp=None):
        logger.info("Building environment for position setpoint task.")
        super().__init__(task_config, seed, num_envs, headless, device, use_warp)
        cfg, env, N, dev = self.task_config, self.sim_env, self.num_envs, self.device
        for key in cfg.reward_parameters.keys():
            cfg.reward_parameters[key] = torch.tensor(cfg.reward_parameters[key], device=dev)
        if cfg.action_space_dim != 4 or cfg.observation_space_dim != 15 or env.num_robot_actions != 4:
            raise ValueError("the end-to-end set-point task has 4-D actions (one per motor) and 15-D observations "
                             "(task_config.action_space_dim, observation_space_dim, the robot's num_motors)")
        # the config builds the limits on the CPU at import (the reference: on cuda:0); they live on the task's device from here
        lo, hi = (torch.as_tensor(x, dtype=torch.float32).cpu() for x in (cfg.action_limit_min, cfg.action_limit_max))
        self.action_limit_min, self.action_limit_max = lo.to(dev), hi.to(dev)
        self._limits = _lib.AgxEndToEndLimits()
        for j in range(4):
            self._limits.min[j], self._limits.max[j] = float(lo[j]), float(hi[j])
        self._reward_constants = reward_constants(self.REWARD)
        # never written except to zero on reset (:78-80, :152, handle_action_history has no caller): kept as an attribute, no launch
        self.action_history = torch.zeros((N, cfg.action_space_dim * 10), device=dev)
        self.prev_position_soa, self.prev_pos_error_soa = soa(3, N, dev), soa(3, N, dev)
        self.prev_position = aos_view(self.prev_position_soa)
        self.prev_pos_error = aos_view(self.prev_pos_error_soa)
        # strict_rng: standard normals of the observation noise, [4][N][3] in the reference's draw order (:207-218)
        self.obs_noise = torch.zeros((4, N, 3), device=dev)
        self._bookkeeping_done = False
        # The reference's step resets every finished env twice: post_reward_calculation_step resets them, then its own
        # reset_idx(reset_envs) calls sim_env.reset_idx again (:180-182) -- a second full set of draws, whose outcome is the
        # final state.  strict_rng consumes both sets from the torch generator and resets once with the second: exact, because
        # the second reset overwrites every field the first would have written (state, bounds, motor constants, thrusts,
        # sim_steps) for the same envs, and nothing reads those fields in between.
        env.reset_draw_sets = 2

    def reset_idx(self, env_ids):
        super().reset_idx(env_ids)
        self.action_history[env_ids] = 0.0

    def _check_actions(self, actions):
        """The rescaled command goes into the task's own tensor: the caller's is read once and not kept, so a strided one is copied."""
        if not (isinstance(actions, torch.Tensor) and actions.dtype is torch.float32 and tuple(actions.shape) == (self.num_envs, 4)
                and actions.device == self.actions.device):
            raise ValueError(f"actions must be a float32 tensor of shape ({self.num_envs}, 4) on {self.actions.device}")
        return actions if actions.is_contiguous() else actions.contiguous()

    @roctx.ranged("PositionSetpointTaskSim2RealEndToEnd.step")
    def step(self, actions):
        env, cfg = self.sim_env, self.task_config
        env._require_device()
        actions = self._check_actions(actions)
        self.counter += 1
        if cfg.process_actions_for_task is task_config_module.end_to_end_process_actions:
            # actions <- clamp(actions, -1, 1) * (max - min) / 2 + (max + min) / 2; prev_position[:] = robot_position
            _lib.check(
                env._lib.agx_end_to_end_pre_step(env._buffers, env.num_envs, _lib.dptr(actions), self._limits, _lib.dptr(self.actions),
                                                 _lib.dptr(self.prev_position_soa), env._stream()),
                "agx_end_to_end_pre_step",
            )
        else:  # a rescale the user put into the config runs as the torch code it is
            self.actions = cfg.process_actions_for_task(actions, self.action_limit_min, self.action_limit_max).to(torch.float32).contiguous()
            self.prev_position[:] = self.obs_dict["robot_position"]
        # the tail of this step in one launch, unless the observation is wanted of the state before the reset
        env.post_step_launch = None if cfg.return_state_before_reset else self._launch_post_step
        self._bookkeeping_done = False
        try:
            env.step(actions=self.actions)
            self.compute_rewards_and_crashes(self.obs_dict)  # writes self.rewards and self.terminations (the dict's crashes) in place
            if cfg.return_state_before_reset:
                return_tuple = self.get_return_tuple()
            # (truncations = sim_steps > episode_len_steps: written by the reward launch together with the reset set)
            env.post_reward_calculation_step()
        finally:
            env.post_step_launch = None
        if not self._bookkeeping_done:
            # the reference's own reset_idx(reset_envs) (:181-182): when some env resets, the target of EVERY env goes back to zero
            # (the fused tail does this itself).  On the device: the step's reset flag stays set until the step after next.
            any_reset = self.obs_dict["reset_flag"][env._parity] != 0
            torch.where(any_reset, torch.zeros_like(self.target_soa), self.target_soa, out=self.target_soa)
        self.infos = {}
        if not cfg.return_state_before_reset:
            return_tuple = self.get_return_tuple()
        if not self._bookkeeping_done:  # :189-190, on the post-reset position
            self.prev_actions.copy_(self.actions)
            torch.sub(self.target_soa, self.obs_dict["robot_state_soa"][0:3], out=self.prev_pos_error_soa)
        return return_tuple

    def _launch_post_step(self):
        """EnvManager._launch_reset's stand-in for this step: reset + observation + bookkeeping (called behind the strict draws)"""
        env = self.sim_env
        noise = None
        if env.strict_rng:
            self._draw_obs_noise()
            noise = _lib.dptr(self.obs_noise)
        _lib.check(
            env._lib.agx_post_step_end_to_end(env._params, env._buffers, env.num_envs, env._reset_args, _lib.dptr(self.target_soa), noise,
                                              _lib.dptr(self.task_obs["observations"]), _lib.dptr(self.actions),
                                              _lib.dptr(self.prev_actions), _lib.dptr(self.prev_pos_error_soa), env._stream()),
            "agx_post_step_end_to_end",
        )
        self._bookkeeping_done = True

    def _draw_obs_noise(self):
        """four normal fills of [N, 3], in the reference's order: the torch stream is consumed as there"""
        for k, tag in enumerate(NOISE_TAGS):
            self.sim_env.random_source.normal_into(self.obs_noise[k], tag=tag)

    def process_obs_for_task(self):
        env = self.sim_env
        env._require_device()
        if not env.take_produced(env.OBSERVATION):  # (by agx_post_step_end_to_end: neither launched twice nor served stale)
            noise = None
            if env.strict_rng:
                self._draw_obs_noise()
                noise = _lib.dptr(self.obs_noise)
            _lib.check(
                env._lib.agx_end_to_end_obs(env._buffers, env.num_envs, _lib.dptr(self.target_soa), noise,
                                            _lib.dptr(self.task_obs["observations"]), env._stream()),
                "agx_end_to_end_obs",
            )
        self._publish_step_flags()

    def compute_rewards_and_crashes(self, obs_dict):
        """compute_reward, the distance crash, `truncations = sim_steps > episode_len_steps` and the step's reset set"""
        env = self.sim_env
        env._require_device()
        _lib.check(
            env._lib.agx_end_to_end_reward(env._buffers, env.num_envs, _lib.dptr(self.target_soa), _lib.dptr(self.actions),
                                           _lib.dptr(self.prev_actions), _lib.dptr(self.prev_pos_error_soa), self._reward_constants,
                                           float(self.task_config.crash_dist), int(self.task_config.episode_len_steps),
                                           int(env.cfg.env.reset_on_collision), _lib.dptr(self.rewards), env._stream()),
            "agx_end_to_end_reward",
        )
        env.mark_produced(env.RESET_SET)  # the reward kernel wrote this step's reset set
        return self.rewards, self.terminations
