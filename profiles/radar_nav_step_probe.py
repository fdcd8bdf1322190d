"""Times task.step() of radar_navigation_task (lmf2_radar, acceleration commands, 48 x 120 radar, 337-D observation) next to
lidar_navigation_task, whose launches it runs with two entry points exchanged, at 512 envs (the reference's num_envs) and at 8192 envs,
and lists what each step launches.

    python profiles/radar_nav_step_probe.py [--envs 512 8192] [--steps 300] [--warmup 50] [--repeats 3] [--out FILE.json]

The time is a host clock around `steps` calls that end in a device synchronise, both tasks in the same process one after the other.
There is no speed gate on the radar task: the condition is structural (the launch list of tests/test_gpu_radar_nav.py)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TASKS = ("radar_navigation_task", "lidar_navigation_task")


def time_task(name, envs, steps, warmup, repeats):
    import torch

    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    task = task_registry.make_task(name, seed=1, num_envs=envs, headless=True)
    task.reset()
    policy = torch.rand(envs, 4, device=task.device) * 2.0 - 1.0
    for _ in range(warmup):
        task.step(policy)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            task.step(policy)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps)
    calls, real = [], _lib.check

    def check(code, what=""):
        calls.append(what)
        return real(code, what)

    _lib.check = check
    try:
        task.step(policy)
        torch.cuda.synchronize()
    finally:
        _lib.check = real
    task.close()
    best = min(times)
    return {"task": name, "num_envs": envs, "step_us": [round(t * 1e6, 2) for t in times], "best_step_us": round(best * 1e6, 2),
            "env_steps_per_s": round(envs / best), "library_calls_of_a_step": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[512, 8192])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("radar_nav_step_probe needs a HIP device: a time taken anywhere else says nothing")
    rows = [time_task(name, envs, a.steps, a.warmup, a.repeats) for envs in a.envs for name in TASKS]
    result = {"steps": a.steps, "warmup": a.warmup, "rows": rows, "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id()}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
