#!/usr/bin/env python
"""Where a wave of the single-launch position step spends its lifetime (k_position_step_fused<AGX_STEP_ANY>, bench.py's plain
workload: 8192 envs, Lee position control, episodes desynchronised).

    python profiles/step_phase_probe.py --stamps [--lib FILE] [--steps 300] [--out FILE]
        builds (or takes: --lib) the library variant with -DAGX_STEP_STAMPS, in which lane 0 of every wave stamps the shader clock
        at six points (csrc/agx_dyn_position_step.h: AGX_STAMP) and the 100 MHz wall clock at its start and end, runs the steps one by
        one and reports, per phase, the median over the waves and the wave that finished LAST, each as the median over the ANY
        launches; and how often the folding workgroup 0 was that last finisher
    python profiles/step_phase_probe.py --workload [--steps 300]
        the same steps on the product library and nothing else: what a counter pass profiles
        (rocprofv3 --pmc ... -- python profiles/step_phase_probe.py --workload; profiles/collect_pmc.py step_counters reads its CSV)

The stamped build waits for its input loads where it stamps their arrival and reads the clock through scalar memory, so its waves
are a little slower than the product's; parent and change are measured the same way.  Prints one JSON object."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANT = os.path.join(ROOT, "aerial_gym_simulator_amd", "lib", "libagx_step_stamps.so")
PHASES = ("start -> arguments there, first input load issued", "-> inputs arrived", "-> barrier reached (step computed)",
          "-> barrier passed", "-> last store issued")
WORDS = 8


def _bench():
    spec = importlib.util.spec_from_file_location("agx_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _task(dev):
    import torch

    bench = _bench()
    task = bench.make_task("dynamics", 8192, dev, False)
    task.reset()
    bench.desynchronise_episodes(task)
    g = torch.Generator(device=dev).manual_seed(1234)
    actions = [torch.rand(task.num_envs, 4, device=dev, generator=g) * 2 - 1 for _ in range(16)]
    return task, actions


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stamps", action="store_true")
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--lib", default=None, help="a library built with -DAGX_STEP_STAMPS (default: built from this tree)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stamps:
        lib = os.path.abspath(args.lib) if args.lib else VARIANT
        if os.environ.get("AGX_LIB_PATH") != lib:
            if not args.lib and not os.path.exists(lib):
                from aerial_gym_simulator_amd import _build

                _build.build_library(extra_flags=["-DAGX_STEP_STAMPS"], lib_path=lib)
            raise SystemExit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=dict(os.environ, AGX_LIB_PATH=lib)))
    import numpy as np
    import torch

    from aerial_gym_simulator_amd import _lib

    dev = "cuda:0"
    task, actions = _task(dev)
    for i in range(args.warmup):
        task.step(actions[i % 16])
    torch.cuda.synchronize()
    if not args.stamps:
        for i in range(args.steps):
            task.step(actions[i % 16])
        torch.cuda.synchronize()
        print(json.dumps({"workload": "plain bench.py steps", "steps": args.steps, "modes": task.single_launch_stats()["modes"],
                          "build_id": _lib.build_id()}))
        return
    raw = C.CDLL(os.environ["AGX_LIB_PATH"])
    any_mode = _lib.STEP_MODES.index("any")
    blocks = (task.num_envs + 15) // 16 + 1  # + the folding workgroup 0
    buf = np.zeros((blocks, 2, WORDS), np.uint64)
    rows = {"step": {"median": [], "last": []}, "helper": {"median": [], "last": []}}
    life = {"step": {"median": [], "last": []}, "helper": {"median": [], "last": []}}
    launch_ticks, last_is, used, cyc, ticks = [], {"step": 0, "helper": 0, "fold": 0}, 0, 0.0, 0.0
    for i in range(args.steps):
        task.step(actions[i % 16])
        torch.cuda.synchronize()
        if int(task._plan.last_mode) != any_mode:
            continue
        assert raw.agx_debug_step_stamps(buf.ctypes.data_as(C.POINTER(C.c_ulonglong)), blocks) == 0
        t = buf.astype(np.int64)
        env = t[1:]  # [env block][wave][word]
        w0 = int(min(t[0, 0, 6], env[:, :, 6].min()))
        if int(env[:, :, 6].max()) - w0 > 5000:  # (50 us: not one launch -- stamps left over from another kernel)
            continue
        used += 1
        ends = {"step": env[:, 0, 7], "helper": env[:, 1, 7], "fold": t[0:1, 0, 7]}
        last_kind = max(ends, key=lambda k: int(ends[k].max()))
        last_is[last_kind] += 1
        launch_ticks.append(int(max(int(e.max()) for e in ends.values())) - w0)
        for wi, kind in enumerate(("step", "helper")):
            x = env[:, wi, :]
            d = np.diff(x[:, 0:6], axis=1)  # [block][5 phases], shader clocks
            tot = x[:, 5] - x[:, 0]
            cyc += float(tot.sum())
            ticks += float((x[:, 7] - x[:, 6]).sum())
            b = int(np.argmax(x[:, 7]))  # the wave of this kind that finished last
            rows[kind]["median"].append(np.median(d, axis=0))
            rows[kind]["last"].append(d[b])
            life[kind]["median"].append(float(np.median(tot)))
            life[kind]["last"].append(float(tot[b]))
    ns_per_clock = (ticks * 10.0 / cyc) if cyc else None
    out = {"what": "phases of the waves of k_position_step_fused<AGX_STEP_ANY>, stamped build, 8192 envs, one synchronised step at a time",
           "library": os.environ["AGX_LIB_PATH"], "build_id": _lib.build_id(), "any_launches_used": used, "steps": args.steps,
           "ns_per_shader_clock": ns_per_clock, "launch_first_start_to_last_end_us_median": med(launch_ticks) / 100.0 if launch_ticks else None,
           "last_finisher_of_the_launch": last_is, "unit": "us (shader clocks x ns_per_shader_clock)"}
    for kind in ("step", "helper"):
        for which in ("median", "last"):
            if not rows[kind][which]:
                continue
            a = np.array(rows[kind][which])
            key = f"{kind}_wave_{'median_wave' if which == 'median' else 'last_finishing_wave'}"
            out[key] = {"lifetime": med(life[kind][which]) * ns_per_clock / 1e3,
                        "phases": {PHASES[k]: float(np.median(a[:, k])) * ns_per_clock / 1e3 for k in range(5)}}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
