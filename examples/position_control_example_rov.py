"""Fully actuated control of 64 ROVs (the BlueROV airframe, eight fixed thrusters) towards random poses in a world without gravity
(reference: examples/position_control_example_rov.py; written against the `aerial_gym` alias, as code for the reference is).

The command is 7-D: a world-frame position set-point and an attitude set-point as a quaternion (x, y, z, w)."""
import os

import torch

from aerial_gym.sim.sim_builder import SimBuilder

if __name__ == "__main__":
    env = SimBuilder().build_env(sim_name="base_sim_no_gravity", env_name="empty_env", robot_name="base_rov",
                                 controller_name="fully_actuated_control", args=None, device="cuda:0", num_envs=64, headless=True,
                                 use_warp=False)
    n = env.num_envs
    actions = torch.zeros((n, 7), device="cuda:0")
    actions[:, 6] = 1.0  # level, heading along x
    env.reset()
    g = env.get_obs()
    for i in range(int(os.environ.get("AGX_EXAMPLE_STEPS", 2000))):
        if i % 500 == 0:  # a new set-point for every ROV (it travels there from where it is): inside the +-1 m env, any heading
            actions[:, 0:3] = 0.6 * (torch.rand(n, 3, device="cuda:0") * 2 - 1)
            yaw = torch.pi * (torch.rand(n, device="cuda:0") * 2 - 1)
            actions[:, 3:5] = 0.0
            actions[:, 5], actions[:, 6] = torch.sin(yaw / 2), torch.cos(yaw / 2)
        env.step(actions=actions)
        if i % 250 == 249:
            err = (g["robot_position"] - actions[:, 0:3]).norm(dim=1)
            # |<q, q_sp>| = cos(half the angle between the two attitudes)
            ang = 2 * torch.acos((g["robot_orientation"] * actions[:, 3:7]).sum(dim=1).abs().clamp(max=1.0))
            print(f"step {i + 1}: mean position error {float(err.mean()):.3f} m, max {float(err.max()):.3f} m; "
                  f"mean attitude error {float(ang.mean()):.3f} rad")
