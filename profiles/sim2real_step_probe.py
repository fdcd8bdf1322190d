"""Times task.step() of position_setpoint_task_sim2real (the reference's default rl_games recipe: lmf2, velocity commands, noisy
17-D observation) and counts what it launches.

    python profiles/sim2real_step_probe.py [--task NAME] [--envs 8192] [--steps 2000] [--warmup 200] [--out FILE.json]

The time is a host clock around `steps` calls that end in a device synchronise; the launch list comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python profiles/sim2real_step_probe.py --steps 200 --warmup 20` (tracing slows the host)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="position_setpoint_task_sim2real")
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    if not torch.cuda.is_available():
        raise SystemExit("sim2real_step_probe needs a HIP device: a time taken anywhere else says nothing")
    task = task_registry.make_task(a.task, seed=1, num_envs=a.envs, headless=True)
    task.reset()
    actions = torch.zeros(a.envs, 4, device=task.device)
    policy = (torch.rand(a.envs, 4, device=task.device) * 2.0 - 1.0) * 0.3
    for _ in range(a.warmup):
        actions.copy_(policy)
        task.step(actions)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            actions.copy_(policy)  # the caller's buffer, rewritten every step like a policy's output
            task.step(actions)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / a.steps)
    best = min(times)
    result = {"task": a.task, "num_envs": a.envs, "steps": a.steps, "warmup": a.warmup,
              "step_us": [round(t * 1e6, 2) for t in times], "best_step_us": round(best * 1e6, 2),
              "env_steps_per_s": round(a.envs / best), "includes": "one [N, 4] copy into the caller's action buffer per step",
              "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id()}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
