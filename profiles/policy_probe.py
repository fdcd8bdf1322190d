"""Times the actor of a trained policy in the loop: the fused call (utils/policy.py ActorMLP, one launch of csrc/agx_policy.hip)
against the torch module of tests/test_gpu_policy_transfer.py on the same weights (four addmm, three elu, a clamp; sampled: randn,
exp, mul, add on top), at 256 and 8192 envs.

    python profiles/policy_probe.py [--envs 256 8192] [--calls 2000] [--out profiles/policy_probe.json]

(a) the actor call alone, in us per call; (b) the closed loop of position_setpoint_task (base_quadrotor, lee_attitude_control,
the attitude actor): actor call + task.step, in ms per step.  Each in two forms: deterministic + clamp, and sampled + clamp.

A sample is a host clock around `calls` back-to-back calls that end in a device synchronise, divided by `calls`; the figure is the
median of 5 samples after a warm-up, and the two actors alternate sample by sample.  Back-to-back calls overlap the host's enqueue
with the device's work, as a training loop does: the figure is the larger of the two, not a kernel time.  No threshold is set
anywhere."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"


def sample(fn, calls, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) / calls


def alternate(fns, calls, sync, scale):
    """{name: (median, samples)} of 5 samples each, taken in turns"""
    for fn in fns.values():
        sample(fn, max(10, calls // 10), sync)  # warm-up
    got = {name: [] for name in fns}
    for _ in range(5):
        for name, fn in fns.items():
            got[name].append(sample(fn, calls, sync) * scale)
    return {name: (round(statistics.median(v), 5), [round(x, 5) for x in v]) for name, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 8192])
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "policy_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from test_gpu_policy_transfer import GOLDEN, Actor

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.config.task_config import position_setpoint_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry
    from aerial_gym_simulator_amd.utils.policy import ActorMLP

    if not torch.cuda.is_available():
        raise SystemExit("policy_probe needs a HIP device: a time taken anywhere else says nothing")
    g = np.load(GOLDEN)
    ws, bs = [g[f"w{i}"] for i in range(4)], [g[f"b{i}"] for i in range(4)]
    torch_actor = Actor(g).to(DEV).eval()
    sigma = torch.exp(torch_actor.logstd)
    gen = torch.Generator(device=DEV).manual_seed(1)
    cfg.device, cfg.controller_name, cfg.robot_name, cfg.args = DEV, "lee_attitude_control", "base_quadrotor", {}
    sync = torch.cuda.synchronize
    rows = []
    with torch.no_grad():
        for n in a.envs:
            task = task_registry.make_task("position_setpoint_task", seed=1, num_envs=n, headless=True)
            fused = ActorMLP.from_arrays(ws, bs, logstd=g["logstd"], device=DEV, task=task)
            state = {"obs": task.reset()[0]["observations"]}
            obs = state["obs"].clone()

            def torch_det(x):
                return torch_actor(x).clamp(-1.0, 1.0)

            def torch_sampled(x):
                m = torch_actor(x)
                return (m + sigma * torch.randn(m.shape, device=DEV, generator=gen)).clamp(-1.0, 1.0)

            def fused_det(x):
                return fused(x, clamp=True)

            def fused_sampled(x):
                return fused(x, sample=True, clamp=True)

            worst = float((fused_det(obs) - torch_det(obs)).abs().max())  # same net: the two differ by float32 summation order only
            row = {"num_envs": n, "max_abs_difference_fused_vs_torch": worst}
            calls = {"fused_det": lambda: fused_det(obs), "torch_det": lambda: torch_det(obs), "fused_sampled": lambda: fused_sampled(obs),
                     "torch_sampled": lambda: torch_sampled(obs)}
            for name, (med, samples) in alternate(calls, a.calls, sync, 1e6).items():
                row[f"actor_{name}_us"], row[f"actor_{name}_us_samples"] = med, samples

            def loop(actor_fn):
                def one():
                    state["obs"] = task.step(actor_fn(state["obs"]))[0]["observations"]
                return one

            zero = torch.zeros((n, 4), device=DEV)
            loops = {"step_only": lambda: task.step(zero), "fused_det": loop(fused_det), "torch_det": loop(torch_det),
                     "fused_sampled": loop(fused_sampled), "torch_sampled": loop(torch_sampled)}
            for name, (med, samples) in alternate(loops, a.calls, sync, 1e3).items():
                row[f"loop_{name}_ms"], row[f"loop_{name}_ms_samples"] = med, samples
            rows.append(row)
            task.close()
    result = {"probe": "policy_probe", "net": "13-256-128-64-4 ELU (tests/golden/policy_attitude_actor.npz)", "calls_per_sample": a.calls,
              "samples": 5, "rows": rows, "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id()}
    print(json.dumps(result))
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
