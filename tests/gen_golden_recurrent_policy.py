"""Writes tests/golden/policy_lmf2_nav_recurrent_actor.npz: the actor arrays of the reference's navigation policy
sim2real/weights/lmf2_sim2real_241024 (sample-factory, 81 -> 256 -> 128 -> 64 ELU, GRU 64, adaptive head of 8 = 4 means + 4
log-std) -- weights and the observation normaliser's statistics only, no critic, no optimizer state.  Run once where the
reference tree is at hand:

    python tests/gen_golden_recurrent_policy.py <reference root>

No test reads the reference tree: they read the fixture."""
import glob
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
EXPERIMENT = os.path.join("aerial_gym", "sim2real", "weights", "lmf2_sim2real_241024")


def main(root):
    from aerial_gym_simulator_amd.utils.policy import recurrent_arrays_from_state_dict

    path = sorted(glob.glob(os.path.join(root, EXPERIMENT, "checkpoint_p0", "best_*.pth")))[-1]
    sd = torch.load(path, map_location="cpu", weights_only=False)["model"]
    a = recurrent_arrays_from_state_dict(sd)  # refuses anything that is not this structure
    prefix = f"obs_normalizer.running_mean_std.running_mean_std.{a['obs_key']}."
    arrays = {"obs_key": np.array(a["obs_key"]), "norm_mean": sd[prefix + "running_mean"].numpy(), "norm_var": sd[prefix + "running_var"].numpy()}
    for i, (w, b) in enumerate(zip(a["enc_weights"], a["enc_biases"])):
        arrays[f"w{i}"], arrays[f"b{i}"] = w, b
    for name in ("w_ih", "w_hh", "b_ih", "b_hh", "head_weight", "head_bias"):
        arrays[name] = a[name]
    assert a["logstd"] is None and arrays["norm_mean"].dtype == np.float64
    out = os.path.join(HERE, "golden", "policy_lmf2_nav_recurrent_actor.npz")
    np.savez(out, **arrays)
    print(out, os.path.getsize(out), "bytes;", os.path.basename(path))


if __name__ == "__main__":
    main(sys.argv[1])
