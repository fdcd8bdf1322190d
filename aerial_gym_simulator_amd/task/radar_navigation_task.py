"""RadarNavigationTask with the reference's API and step ordering
(aerial_gym/task/radar_navigation_task/radar_navigation_task.py:4-157): the LiDAR-navigation recipe on
`lmf2_radar` (lmf2 + acceleration control + a 48 x 120 radar of +-60 degrees) in env_with_obstacles -> 337-D observation.

A subclass of LiDARNavigationTask, like the reference's: step, reset, reset_idx, process_obs_for_task and the curriculum are
the parent's.  Three things differ: the noise on the min-pooled image (:6-21: 3 % of the cells += U(0.2, 10), then 80 % of the
cells = -1; no max-range mask, no low-row mask), so the image post-processing is agx_radar_image_obs; and the reward
(:179-342: backward instead of forward vehicle-frame x velocity is penalised, :242-246), agx_reward_radar_navigation.
Per task.step() the launches are the parent's with these two names in place of agx_lidar_image_obs / agx_reward_lidar_navigation."""
import torch

from .. import _lib
from ..utils.logging import CustomLogger
from .lidar_navigation_task import LiDARNavigationTask

logger = CustomLogger("radar_navigation_task")


class RadarNavigationTask(LiDARNavigationTask):
    def compute_rewards_and_crashes(self, obs_dict):
        env = self.sim_env
        env._require_device()
        p = _lib.dptr
        _lib.check(
            env._lib.agx_reward_radar_navigation(env._buffers, env.num_envs, p(self.target_soa), p(self.target_yaw),
                                                 p(self.current_action), p(self.prev_action), p(self.time_to_collision), self._rp,
                                                 float(self.curriculum_progress_fraction), p(self.pos_err_soa),
                                                 p(self.prev_pos_err_soa), int(self.task_config.episode_len_steps),
                                                 int(env.cfg.env.reset_on_collision), p(self.rewards), env._stream()),
            "agx_reward_radar_navigation",
        )
        env.mark_produced(env.RESET_SET)  # the reward kernel wrote this step's reset set
        return self.rewards, self.terminations

    def _draw_lidar_noise(self):
        """strict mode: the draws of add_noise_to_downsampled_lidar_data (:6-21) in the reference's order (incl. its
        data-dependent draw count, i.e. one host sync)."""
        rs, N, dev = self.obs_dict["random_source"], self.num_envs, self.device
        oh, ow = self._H // self._ph, self._W // self._pw
        noise_mask = rs.bernoulli(0.03, N, oh, ow, tag="radar_noise_mask")
        k = int((noise_mask == 1).sum())
        noise_val = torch.zeros(N, oh, ow, device=dev)
        noise_val[noise_mask == 1] = (10.0 - 0.2) * rs.rand(k, tag="radar_noise_val") + 0.2
        invalid_mask = rs.bernoulli(0.8, N, oh, ow, tag="radar_invalid_mask")
        self._noise = (noise_mask, noise_val, invalid_mask)
        return [_lib.dptr(t) for t in self._noise]

    def process_image_observation(self):
        env = self.sim_env
        p = _lib.dptr
        noise = self._draw_lidar_noise() if env.strict_rng else [None] * 3
        _lib.check(
            env._lib.agx_radar_image_obs(env._buffers, env.num_envs, self._H, self._W, self._ph, self._pw,
                                         p(self.obs_dict["depth_range_pixels"]), *noise, int(not env.strict_rng),
                                         p(self.time_to_collision), p(self.downsampled_lidar_data), env._stream()),
            "agx_radar_image_obs",
        )
