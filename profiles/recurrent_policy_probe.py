"""Times a recurrent actor in the loop: the fused call (utils/policy.py RecurrentActor, one launch of csrc/agx_policy.hip
k_recurrent_act) against a torch module on the same weights (nn.Sequential encoder + nn.GRUCell + nn.Linear, the state reset with
`h[ids] = 0` after `nonzero()`, as a user of sample-factory's modules writes it), at 256 / 1024 / 8192 envs.

    python profiles/recurrent_policy_probe.py [--envs 256 1024 8192] [--calls 1000] [--out profiles/recurrent_policy_probe.json]

(a) the actor call alone, in us per call, with the flag tensors of the task as `done`; (b) the closed loop on navigation_task
(actor call + task.step), in ms per step, and task.step alone.  Deterministic actions, clamped.

Sampling as in policy_probe.py: a sample is a host clock around `calls` back-to-back calls that end in a device synchronise, divided
by `calls`; the figure is the median of 5 samples after a warm-up, and the actors alternate sample by sample.  No threshold is set
anywhere."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 1024, 8192])
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--loop-calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "recurrent_policy_probe.json"))
    a = ap.parse_args()
    import recurrent_policy_ref as ref
    import torch
    from policy_probe import alternate

    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd import _lib
    from aerial_gym_simulator_amd.config.task_config import navigation_task_config as cfg
    from aerial_gym_simulator_amd.registry.task_registry import task_registry
    from aerial_gym_simulator_amd.utils.policy import RecurrentActor

    if not torch.cuda.is_available():
        raise SystemExit("recurrent_policy_probe needs a HIP device: a time taken anywhere else says nothing")
    net = ref.load_fixture()
    mean, denom, clip = (torch.as_tensor(v, device=DEV) for v in net["input_norm"])
    layers = []
    for w, b in zip(net["enc_weights"], net["enc_biases"]):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        lin.weight.data.copy_(torch.from_numpy(w))
        lin.bias.data.copy_(torch.from_numpy(b))
        layers += [lin, torch.nn.ELU()]
    encoder = torch.nn.Sequential(*layers).to(DEV).eval()
    cell = torch.nn.GRUCell(64, 64)
    for name, key in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
        getattr(cell, name).data.copy_(torch.from_numpy(net[key]))
    cell = cell.to(DEV).eval()
    head = torch.nn.Linear(64, 8)
    head.weight.data.copy_(torch.from_numpy(net["head_weight"]))
    head.bias.data.copy_(torch.from_numpy(net["head_bias"]))
    head = head.to(DEV).eval()
    cfg.device, cfg.args = DEV, {}
    sync = torch.cuda.synchronize
    rows = []
    with torch.no_grad():
        for n in a.envs:
            task = task_registry.make_task("navigation_task", seed=1, num_envs=n, headless=True)
            fused = RecurrentActor.from_arrays(device=DEV, task=task, **ref.actor_kwargs(net))
            state = {"obs": task.reset()[0]["observations"], "h": torch.zeros((n, 64), device=DEV)}
            obs = state["obs"].clone()

            def torch_actor(x):
                ids = (task.terminations | task.truncations).nonzero().squeeze(-1)  # the host waits here
                state["h"][ids] = 0.0
                x = torch.clamp((x - mean) / denom, -clip, clip)
                state["h"] = cell(encoder(x), state["h"])
                return head(state["h"])[:, :4].clamp(-1.0, 1.0)

            def fused_actor(x):
                return fused(x, done=(task.terminations, task.truncations), clamp=True)

            worst = float((fused_actor(obs) - torch_actor(obs)).abs().max())  # same net, both from a zero state
            row = {"num_envs": n, "max_abs_difference_fused_vs_torch": worst}
            calls = {"fused": lambda: fused_actor(obs), "torch": lambda: torch_actor(obs)}
            for name, (med, samples) in alternate(calls, a.calls, sync, 1e6).items():
                row[f"actor_{name}_us"], row[f"actor_{name}_us_samples"] = med, samples

            def loop(actor_fn):
                def one():
                    state["obs"] = task.step(actor_fn(state["obs"]))[0]["observations"]
                return one

            zero = torch.zeros((n, 4), device=DEV)
            loops = {"step_only": lambda: task.step(zero), "fused": loop(fused_actor), "torch": loop(torch_actor)}
            for name, (med, samples) in alternate(loops, a.loop_calls, sync, 1e3).items():
                row[f"loop_{name}_ms"], row[f"loop_{name}_ms_samples"] = med, samples
            rows.append(row)
            task.close()
    result = {"probe": "recurrent_policy_probe", "net": "81-256-128-64 ELU, GRU 64, head 8 (tests/golden/policy_lmf2_nav_recurrent_actor.npz)",
              "calls_per_sample": a.calls, "loop_calls_per_sample": a.loop_calls, "samples": 5, "rows": rows,
              "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id()}
    print(json.dumps(result))
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
