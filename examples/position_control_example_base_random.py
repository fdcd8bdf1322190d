"""Lee position control of 64 `base_random` airframes -- eight motors at arbitrary poses, the centre of mass 22.6 mm off the base
link -- towards random set-points (written against the `aerial_gym` alias, as code for the reference is; the reference names this
robot as a drop-in `robot_name` of its position task).

The command is 4-D: a world-frame position set-point and a yaw set-point.  The config's disturbance is on, and the controller's
allocation matrix is the reference's, computed about the base-link origin: the airframe is flown slightly wrong, on purpose."""
import os

import torch

from aerial_gym.sim.sim_builder import SimBuilder

if __name__ == "__main__":
    env = SimBuilder().build_env(sim_name="base_sim", env_name="empty_env", robot_name="base_random", controller_name="lee_position_control",
                                 args=None, device="cuda:0", num_envs=64, headless=True, use_warp=False)
    n = env.num_envs
    actions = torch.zeros((n, 4), device="cuda:0")
    env.reset()
    g = env.get_obs()
    for i in range(int(os.environ.get("AGX_EXAMPLE_STEPS", 2000))):
        if i % 500 == 0:  # a new set-point for every robot (it flies there from where it is): inside the env, any heading
            actions[:, 0:3] = 0.6 * (torch.rand(n, 3, device="cuda:0") * 2 - 1)
            actions[:, 3] = torch.pi * (torch.rand(n, device="cuda:0") * 2 - 1)
        env.step(actions=actions)
        if i % 250 == 249:
            err = (g["robot_position"] - actions[:, 0:3]).norm(dim=1)
            print(f"step {i + 1}: mean position error {float(err.mean()):.3f} m, max {float(err.max()):.3f} m; "
                  f"mean speed of the mass centre {float(g['robot_linvel'].norm(dim=1).mean()):.3f} m/s")
