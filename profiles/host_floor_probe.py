#!/usr/bin/env python
"""The host's own floor of a position step: bench.py's loop (8192 envs, Lee position control, episodes desynchronised), timed on
the host, minus the time agx_position_task_step spent spinning on the proof record because it was max_lag steps ahead of the
device (AgxPositionStepPlan.lag_wait_ns / lag_waits).  What is left is what the host needs per step when it never has to wait:
the step time below which a faster kernel can no longer show.

    python profiles/host_floor_probe.py [--steps 2000] [--warmup 200] [--repeats 3] [--out FILE]

Prints one JSON object."""
import argparse
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("agx_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    dev = "cuda:0"
    task = bench.make_task("dynamics", 8192, dev, False)
    task.reset()
    bench.desynchronise_episodes(task)
    g = torch.Generator(device=dev).manual_seed(1234)
    actions = [torch.rand(task.num_envs, 4, device=dev, generator=g) * 2 - 1 for _ in range(16)]
    plan = task._plan
    torch.cuda.synchronize()
    for i in range(args.warmup):
        task.step(actions[i % 16])
    torch.cuda.synchronize()
    runs = []
    for _ in range(args.repeats):
        ns0, n0 = int(plan.lag_wait_ns), int(plan.lag_waits)
        t0 = time.perf_counter()
        for i in range(args.steps):
            task.step(actions[i % 16])
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        spin = (int(plan.lag_wait_ns) - ns0) * 1e-9
        runs.append({"step_us": 1e6 * wall / args.steps, "host_enqueue_us": 1e6 * host / args.steps, "lag_wait_us": 1e6 * spin / args.steps,
                     "lag_waits_per_step": (int(plan.lag_waits) - n0) / args.steps,
                     "host_floor_us": 1e6 * (host - spin) / args.steps})
    runs.sort(key=lambda r: r["host_floor_us"])
    out = {"what": "bench.py's loop: host enqueue time per step minus the time spent waiting for the proof record (max_lag)",
           "steps": args.steps, "runs": runs, "host_floor_us_median": runs[len(runs) // 2]["host_floor_us"],
           "modes": task.single_launch_stats()["modes"]}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
