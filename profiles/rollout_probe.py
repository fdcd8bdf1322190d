"""Times EnvManager.rollout of T = 500 steps (one launch, csrc/agx_dyn_rollout.h) against 500 eager EnvManager.step calls on the same
build, with and without a record of the state (robot_position, robot_orientation, robot_linvel, robot_angvel: 13 channels).

    python profiles/rollout_probe.py [--steps 500] [--out profiles/rollout_probe.json]

Configurations: base_quadrotor + lee_position_control in empty_env (1 sub-step) at 256 and 8192 envs; base_quadrotor +
lee_velocity_control in env_with_obstacles (10 sub-steps, the collision test every step) at 256 envs.

A sample is a host clock around the whole T steps, the device synchronised at both ends; the figure is the median of 5 samples after
a warm-up, the three forms taking turns sample by sample.  The eager loop's figure is the larger of the host's enqueue and the
device's work, as in any stepping loop.  `eager_one_lane` is the same loop under agx_set_option("env_step_quad", 0): the step then
runs k_env_step, the one-lane-per-env family k_env_step_rollout belongs to, instead of the four-lanes-per-env kernels the default picks
for Lee-controlled airframes without drag (`eager_kernels` names both).  The recording form clones the four dict tensors after every
step, which is what a caller without rollout() has to do.  The rollout with a record reuses one RolloutRecord (out=).  No threshold is set anywhere; the one
expectation is written into the result: `rollout_not_slower` per configuration."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
KEYS = ("robot_position", "robot_orientation", "robot_linvel", "robot_angvel")
CONFIGS = [("base_quadrotor", "lee_position_control", "empty_env", 256), ("base_quadrotor", "lee_position_control", "empty_env", 8192),
           ("base_quadrotor", "lee_velocity_control", "env_with_obstacles", 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "rollout_probe.json"))
    a = ap.parse_args()
    import torch

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

    if not torch.cuda.is_available():
        raise SystemExit("rollout_probe needs a HIP device: a time taken anywhere else says nothing")
    T, sync = a.steps, torch.cuda.synchronize
    results = []
    for robot, controller, env_name, n in CONFIGS:
        env = SimBuilder().build_env(sim_name="base_sim", env_name=env_name, robot_name=robot, controller_name=controller, device=DEV,
                                     args={"rng_seed": 7}, num_envs=n, headless=True, use_warp=False)
        env.reset()
        g = env.global_tensor_dict
        gen = torch.Generator(device=DEV).manual_seed(3)
        held = (torch.rand(n, env.num_robot_actions, device=DEV, generator=gen) * 2 - 1) * 0.5
        snap = env.snapshot()
        rec = env.rollout(held, steps=T, record=KEYS)

        def eager():
            for _ in range(T):
                env.step(held)

        def eager_recording():
            out = []
            for _ in range(T):
                env.step(held)
                out.append([g[k].clone() for k in KEYS])
            return out

        def eager_one_lane():  # the eager loop held to the one-lane kernel family the rollout kernel is of (k_env_step)
            with _lib.option("env_step_quad", 0):
                eager()

        def kernel_name():
            import ctypes

            buf = ctypes.create_string_buffer(128)
            env._lib.agx_env_step_kernel(env._params, env._buffers, n, int(env.cfg.env.num_physics_steps_per_env_step_mean), None, buf, 128)
            return buf.value.decode()

        names = {"eager": kernel_name()}
        with _lib.option("env_step_quad", 0):
            names["eager_one_lane"] = kernel_name()
        forms = {"eager": eager, "eager_one_lane": eager_one_lane, "eager_recording": eager_recording,
                 "rollout": lambda: env.rollout(held, steps=T),
                 "rollout_recording": lambda: env.rollout(held, steps=T, record=KEYS, out=rec)}
        got = {name: [] for name in forms}
        for rnd in range(6):  # round 0 is the warm-up
            for name, fn in forms.items():
                env.restore(snap)  # every sample flies the same 500 steps from the same state
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                if rnd:
                    got[name].append((time.perf_counter() - t0) * 1e3)
        row = {"robot": robot, "controller": controller, "env": env_name, "num_envs": n, "steps": T,
               "substeps_per_step": int(env.cfg.env.num_physics_steps_per_env_step_mean), "eager_kernels": names}
        for name, v in got.items():
            row[name + "_ms"] = round(statistics.median(v), 4)
            row[name + "_samples_ms"] = [round(x, 4) for x in v]
        row["rollout_us_per_step"] = round(row["rollout_ms"] * 1e3 / T, 3)
        row["eager_us_per_step"] = round(row["eager_ms"] * 1e3 / T, 3)
        # (both forms of the rollout against the PLAIN eager loop: the stricter reading)
        row["rollout_not_slower"] = bool(row["rollout_ms"] <= row["eager_ms"] and row["rollout_recording_ms"] <= row["eager_ms"])
        results.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_samples_ms")}), flush=True)
        del env
    doc = {"what": "EnvManager.rollout (one launch) vs the eager EnvManager.step loop, ms per T steps, median of 5 device-synchronised samples",
           "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "results": results}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
