"""Times EnvManager.step() + post_reward_calculation_step() of a robot under fully_actuated_control in base_sim_no_gravity / empty_env --
base_rov by default, 64 envs like examples/position_control_example_rov.py -- and counts what it launches.

    python profiles/rov_step_probe.py [--robot base_rov] [--envs 64] [--steps 2000] [--warmup 200] [--repeats 3] [--out FILE.json]
                                      [--controller NAME] [--sim NAME] [--one-lane]

`--robot base_random,base_octarotor --controller lee_position_control --sim base_sim --one-lane` is the comparison of DESIGN.md section 8
for the centre-of-mass offset (agx_env_step_com): several robots, one after the other in ONE process, one JSON line each, the
octarotor kept on the one-lane kernel (`env_step_quad` off) that base_random always runs.

The time is a host clock around `steps` steps that end in a device synchronise, once per region; `--repeats 5 --robot base_octarotor
--envs 4096` is the comparison of DESIGN.md section 8 (the octarotor must not pay for the ROV kind: same launches, instruction-identical
kernels).  The launch list comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python profiles/rov_step_probe.py --steps 200 --warmup 20 --repeats 1` (tracing slows the host);
the library's entry points are counted here as the env manager calls them, and the env-step kernel is named by the library."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--robot", default="base_rov")
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--controller", default=None, help="default: fully_actuated_control (7-D pose command); a Lee controller takes a 4-D command")
    ap.add_argument("--sim", default="base_sim_no_gravity")
    ap.add_argument("--one-lane", action="store_true", help="agx_set_option('env_step_quad', 0): no lane-quad kernels")
    a = ap.parse_args()
    import torch

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

    if not torch.cuda.is_available():
        raise SystemExit("rov_step_probe needs a HIP device: a time taken anywhere else says nothing")
    controller = a.controller or ("fully_actuated_control" if "fully_actuated_control" in aerial_gym_simulator_amd.controller_registry.get_controller_names()
                                  else "rov_fully_actuated_control")
    if a.one_lane:
        _lib.set_option("env_step_quad", 0)
    lines = [probe(a, robot, controller, torch, _lib, SimBuilder) for robot in a.robot.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def probe(a, robot_name, controller, torch, _lib, SimBuilder):
    env = SimBuilder().build_env(sim_name=a.sim, env_name="empty_env", robot_name=robot_name, controller_name=controller,
                                 args={"rng_seed": 1}, device="cuda:0", num_envs=a.envs, headless=True, use_warp=False)
    env.reset()
    n = a.envs
    command = torch.zeros(n, env.num_robot_actions, device="cuda:0")
    command[:, 0:3] = 0.6 * (torch.rand(n, 3, device="cuda:0") * 2 - 1)
    if env.num_robot_actions == 7:
        command[:, 6] = 1.0

    def step():
        env.step(command)
        env.post_reward_calculation_step()

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / a.steps)
    counts = {}
    real = env._lib
    env._lib = CountingLib(real, counts)
    k = min(a.steps, 100)
    for _ in range(k):
        step()
    torch.cuda.synchronize()
    env._lib = real
    buf = ctypes.create_string_buffer(128)
    real.agx_env_step_kernel(env._params, env._buffers, n, 1, None, buf, 128)
    times_us = sorted(round(t * 1e6, 2) for t in times)
    kernel = buf.value.decode()
    if env._com is not None:  # agx_env_step_com: the one-lane family's instance of the same arguments, of the kind with the offset
        kernel = kernel.replace("k_env_step<", "k_env_step_com<")
    result = {"robot": robot_name, "controller": controller, "sim": a.sim, "num_envs": n, "steps": a.steps, "warmup": a.warmup,
              "step_us": [round(t * 1e6, 2) for t in times], "best_step_us": times_us[0], "median_step_us": times_us[len(times_us) // 2],
              "env_steps_per_s": round(n / min(times)), "library_calls_per_step": {name: c / k for name, c in sorted(counts.items())},
              "env_step_kernel": kernel, "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id()}
    line = json.dumps(result)
    print(line, flush=True)
    return line


if __name__ == "__main__":
    main()
