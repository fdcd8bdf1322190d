"""What the set-point tasks share, between BaseTask (the reference's interface) and PositionSetpointTask, the two sim2real tasks and
the end-to-end task: the constructor's overrides, the env, the tensors every one of them allocates, reset / reset_idx / render /
close / get_return_tuple, the publication of the step's flags into task_obs and the general step tail."""
import numpy as np
import torch

from ..sim.sim_builder import SimBuilder
from ..tensors import aos_view, soa
from ..utils.spaces import Box, Dict
from .base_task import BaseTask


def apply_overrides(task_config, seed=None, num_envs=None, headless=None, device=None, use_warp=None):
    """the constructor arguments every task takes: what is not None replaces the config's value"""
    for name, val in (("seed", seed), ("num_envs", num_envs), ("headless", headless), ("device", device), ("use_warp", use_warp)):
        if val is not None:
            setattr(task_config, name, val)


def build_env(cfg, args):
    return SimBuilder().build_env(
        sim_name=cfg.sim_name, env_name=cfg.env_name, robot_name=cfg.robot_name, controller_name=cfg.controller_name,
        args=args, device=cfg.device, num_envs=cfg.num_envs, use_warp=cfg.use_warp, headless=cfg.headless,
    )


class SetpointTaskBase(BaseTask):
    OBSERVATION_SPACE_SHAPE = None  # None: (task_config.observation_space_dim,)

    def __init__(self, task_config, seed=None, num_envs=None, headless=None, device=None, use_warp=None, env_args=None):
        """env_args: what the env is built with instead of task_config.args"""
        apply_overrides(task_config, seed, num_envs, headless, device, use_warp)
        super().__init__(task_config)
        cfg = self.task_config
        self.device = cfg.device
        self.sim_env = build_env(cfg, cfg.args if env_args is None else env_args)
        self._own_env_state()
        N, dev = self.sim_env.num_envs, self.device
        self.num_envs = N
        self.actions = torch.zeros((N, cfg.action_space_dim), device=dev)
        self.prev_actions = torch.zeros_like(self.actions)
        self.counter = 0
        self.target_soa = soa(3, N, dev)
        self.target_position = aos_view(self.target_soa)
        self.obs_dict = self.sim_env.get_obs()
        self.obs_dict["num_obstacles_in_env"] = 1
        self.terminations = self.obs_dict["crashes"]
        self.truncations = self.obs_dict["truncations"]
        self.rewards = torch.zeros(N, device=dev)
        shape = self.OBSERVATION_SPACE_SHAPE or (cfg.observation_space_dim,)
        self.observation_space = Dict({"observations": Box(low=-1.0, high=1.0, shape=shape, dtype=np.float32)})
        self.action_space = Box(low=-1.0, high=1.0, shape=(cfg.action_space_dim,), dtype=np.float32)
        self.task_obs = {
            "observations": torch.zeros((N, cfg.observation_space_dim), device=dev),
            "priviliged_obs": torch.zeros((N, cfg.privileged_observation_space_dim), device=dev),
            "collisions": torch.zeros((N, 1), device=dev),
            "rewards": torch.zeros((N, 1), device=dev),
        }
        self.infos = {}

    def close(self):
        self.sim_env.delete_env()

    def reset(self):
        self.target_position[:, 0:3] = 0.0
        self.infos = {}
        self.sim_env.reset()
        return self.get_return_tuple()

    def reset_idx(self, env_ids):
        self.target_position[:, 0:3] = 0.0
        self.infos = {}
        self.sim_env.reset_idx(env_ids)

    def render(self):
        return None

    def get_return_tuple(self):
        self.process_obs_for_task()
        return (self.task_obs, self.rewards, self.terminations, self.truncations, self.infos)

    def _publish_step_flags(self):
        self.task_obs["rewards"] = self.rewards
        self.task_obs["terminations"] = self.terminations
        self.task_obs["truncations"] = self.truncations

    def _step_env_and_return(self):
        """the general path of step() from sim_env.step on: the return tuple is taken before or after the reset, as
        return_state_before_reset says.  compute_rewards_and_crashes writes self.rewards and self.terminations (the dict's crashes) in
        place, and `truncations = sim_steps > episode_len_steps` together with the reset set."""
        env = self.sim_env
        env.step(actions=self.actions)
        self.compute_rewards_and_crashes(self.obs_dict)
        if self.task_config.return_state_before_reset:
            return_tuple = self.get_return_tuple()
        env.post_reward_calculation_step()
        self.infos = {}
        if not self.task_config.return_state_before_reset:
            return_tuple = self.get_return_tuple()
        return return_tuple
