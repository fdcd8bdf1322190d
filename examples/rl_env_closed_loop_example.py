"""A trained policy closes the loop (reference: examples/rl_games_example/rl_env_closed_loop_example.py): position_setpoint_task
with base_quadrotor under lee_attitude_control, flown by the attitude actor the reference trained.  The actor runs as one launch
of the HIP library between two task.step() calls.

    python examples/rl_env_closed_loop_example.py [checkpoint.pth]

With a path: an rl_games checkpoint, loaded through the reference's MLP class under its own import path.  Without: the actor is
built from tests/golden/policy_attitude_actor.npz (the same network as the reference's networks/attitude_policy.pth)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aerial_gym  # noqa: E402,F401  (the reference's import paths)
from aerial_gym.examples.rl_games_example.rl_games_inference import MLP  # noqa: E402
from aerial_gym.registry.task_registry import task_registry  # noqa: E402
from aerial_gym.utils.policy import ActorMLP  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "policy_attitude_actor.npz")

if __name__ == "__main__":
    device = os.environ.get("AGX_EXAMPLE_DEVICE", "cuda:0")
    steps = int(os.environ.get("AGX_EXAMPLE_STEPS", 1000))
    cfg = task_registry.get_task_config("position_setpoint_task")
    cfg.device, cfg.controller_name, cfg.robot_name = device, "lee_attitude_control", "base_quadrotor"
    rl_task_env = task_registry.make_task("position_setpoint_task", seed=42, headless=True, num_envs=24)
    obs = rl_task_env.reset()[0]
    if len(sys.argv) > 1:
        model = MLP(rl_task_env.task_config.observation_space_dim, rl_task_env.task_config.action_space_dim, sys.argv[1]).to(device).eval()
    else:
        g = np.load(FIXTURE)
        model = ActorMLP.from_arrays([g[f"w{i}"] for i in range(4)], [g[f"b{i}"] for i in range(4)], logstd=g["logstd"], device=device,
                                     task=rl_task_env)
    actions = torch.zeros((rl_task_env.sim_env.num_envs, rl_task_env.task_config.action_space_dim), device=device)
    start = time.time()
    with torch.no_grad():
        for i in range(steps):
            actions[:] = model(obs["observations"]).clamp(-1.0, 1.0)
            obs, reward, terminated, truncated, info = rl_task_env.step(actions=actions)
            if i % 100 == 99:  # obs[:, 0:3] = set-point - position
                dist = obs["observations"][:, 0:3].norm(dim=1)
                print(f"step {i + 1}: distance to the set-point {float(dist.mean()):.3f} m mean, {float(dist.max()):.3f} m max; "
                      f"mean reward {float(reward.mean()):.3f}")
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    print(f"{steps} steps of {rl_task_env.sim_env.num_envs} envs in {time.time() - start:.2f} s")
