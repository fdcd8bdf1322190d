"""Times task.step() of position_setpoint_task_sim2real_end_to_end (tinyprop, motor-thrust commands, noisy 15-D observation; 4096 envs
like the reference's config) and counts what it launches.

    python profiles/end_to_end_step_probe.py [--envs 4096] [--steps 2000] [--warmup 200] [--strict] [--out FILE.json]

The time is a host clock around `steps` calls that end in a device synchronise; the launch list comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python profiles/end_to_end_step_probe.py --steps 200 --warmup 20 --repeats 1` (tracing slows the
host).  The structural condition is the launch count: four kernels per step in the default mode (pre-step, env step, reward,
post-step); the library's entry points are counted here as the task calls them."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TASK = "position_setpoint_task_sim2real_end_to_end"


class CountingLib:
    """the loaded library with every agx_* call counted by name"""

    def __init__(self, inner, counts):
        self._inner, self._counts = inner, counts

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        if not name.startswith("agx_"):
            return fn

        def counted(*args):
            self._counts[name] = self._counts.get(name, 0) + 1
            return fn(*args)

        return counted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--strict", action="store_true", help="strict_rng: the torch generator advances as the reference's does")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.registry.task_registry import task_registry

    if not torch.cuda.is_available():
        raise SystemExit("end_to_end_step_probe needs a HIP device: a time taken anywhere else says nothing")
    cfg = task_registry.get_task_config(TASK)
    cfg.args = dict(cfg.args, strict_rng=a.strict)
    task = task_registry.make_task(TASK, seed=1, num_envs=a.envs, headless=True)
    task.reset()
    policy = (torch.rand(a.envs, 4, device=task.device) * 2.0 - 1.0) * 0.3 + 0.4  # around the hover command
    for _ in range(a.warmup):
        task.step(policy)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            task.step(policy)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / a.steps)
    counts = {}
    env = task.sim_env
    real = env._lib
    env._lib = CountingLib(real, counts)
    k = min(a.steps, 100)
    for _ in range(k):
        task.step(policy)
    torch.cuda.synchronize()
    env._lib = real
    best = min(times)
    result = {"task": TASK, "num_envs": a.envs, "steps": a.steps, "warmup": a.warmup, "strict_rng": a.strict,
              "step_us": [round(t * 1e6, 2) for t in times], "best_step_us": round(best * 1e6, 2), "env_steps_per_s": round(a.envs / best),
              "library_calls_per_step": {name: c / k for name, c in sorted(counts.items())},
              "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id()}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
