"""A recurrent navigation policy closes the loop (reference: examples/dce_rl_navigation/dce_nn_navigation.py and
sim2real/sample_factory_inference.py): navigation_task, flown by the sample-factory actor the reference trained for it (encoder
81 -> 256 -> 128 -> 64 ELU, GRU 64, adaptive head) -- encoder, cell, head, the state reset and the clamp as one launch of the HIP
library between two task.step() calls; the task's own flag tensors reset the state, nothing is read back to the host.

    python examples/recurrent_actor_closed_loop_example.py [train_dir experiment]

With a train directory and an experiment name: a sample-factory experiment, loaded through the reference's NN_Inference_Class under
its own import path.  Without: the actor is built from tests/golden/policy_lmf2_nav_recurrent_actor.npz (the arrays of the
reference's sim2real/weights/lmf2_sim2real_241024).

This shows the loop and its speed, not flight quality: the policy was trained on latents of the reference's trained depth-image
VAE, whose weight file is not part of this repository (out of scope), so the latents it sees here are not the ones it
learned."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aerial_gym  # noqa: E402,F401  (the reference's import paths)
from aerial_gym.examples.dce_rl_navigation.sf_inference_class import NN_Inference_Class  # noqa: E402
from aerial_gym.registry.task_registry import task_registry  # noqa: E402
from aerial_gym.utils.policy import SF_NORM_CLIP, SF_NORM_EPSILON, RecurrentActor  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "policy_lmf2_nav_recurrent_actor.npz")

if __name__ == "__main__":
    device = os.environ.get("AGX_EXAMPLE_DEVICE", "cuda:0")
    steps = int(os.environ.get("AGX_EXAMPLE_STEPS", 300))
    num_envs = int(os.environ.get("AGX_EXAMPLE_ENVS", 256))
    cfg = task_registry.get_task_config("navigation_task")
    cfg.device = device
    rl_task_env = task_registry.make_task("navigation_task", seed=42, headless=True, num_envs=num_envs)
    obs = rl_task_env.reset()[0]
    if len(sys.argv) > 2:
        sf_cfg = {"train_dir": sys.argv[1], "experiment": sys.argv[2], "load_checkpoint_kind": "best", "eval_deterministic": True,
                  "device": "cpu" if device == "cpu" else "gpu"}
        actor = NN_Inference_Class(num_envs, cfg.action_space_dim, cfg.observation_space_dim, sf_cfg).actor
    else:
        g = np.load(FIXTURE)
        denom = np.sqrt(g["norm_var"].astype(np.float32) + np.float32(SF_NORM_EPSILON), dtype=np.float32)
        actor = RecurrentActor.from_arrays([g[f"w{i}"] for i in range(3)], [g[f"b{i}"] for i in range(3)], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"],
                                           g["head_weight"], g["head_bias"], input_norm=(g["norm_mean"].astype(np.float32), denom, SF_NORM_CLIP),
                                           device=device, task=rl_task_env)
    resets = torch.zeros((), dtype=torch.int64, device=device)
    start = time.time()
    with torch.no_grad():
        for i in range(steps):
            # the flags of the step that produced `obs` zero the state before this observation is evaluated
            actions = actor(obs["observations"], done=(rl_task_env.terminations, rl_task_env.truncations), clamp=True)
            obs, reward, terminated, truncated, info = rl_task_env.step(actions=actions)
            resets += (terminated | truncated).sum()
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    elapsed = time.time() - start
    print(f"{steps} steps of {num_envs} envs in {elapsed:.2f} s: {steps / elapsed:.1f} steps per second, {steps * num_envs / elapsed:.0f} env steps per "
          f"second; {int(resets)} episodes ended; |h| mean {float(actor.hidden.abs().mean()):.3f}")
