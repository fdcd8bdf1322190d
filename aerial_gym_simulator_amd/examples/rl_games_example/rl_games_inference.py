"""MLP with the reference's surface (aerial_gym/examples/rl_games_example/rl_games_inference.py:7-48): the actor of an rl_games
checkpoint, `MLP(input_dim, output_dim, path).to(device).eval()`, `model.forward(obs)`.  Built on ActorMLP: on a HIP device a
forward is one launch of the library's fused kernel (csrc/agx_policy.hip), not four addmm and three elu.

Differences from the reference's class: the layer widths come from the checkpoint (the reference hard-codes 256-128-64 and fails
in load_state_dict otherwise); a checkpoint with running_mean_std is normalised as rl_games' player does (the reference's strict
load refuses such a file); the result of forward lives in a buffer this object keeps per batch size -- copy it
(`actions[:] = model.forward(obs)`, as the reference's loop does) before the next call."""
from ...utils.policy import ActorMLP


class MLP:
    def __init__(self, input_dim, output_dim, path):
        self.actor = ActorMLP.from_rl_games_checkpoint(path, device="cpu")
        if int(input_dim) != self.actor.obs_dim or int(output_dim) != self.actor.action_dim:
            raise ValueError(f"MLP({input_dim}, {output_dim}, ...): the actor of {path} maps {self.actor.obs_dim} observations to "
                             f"{self.actor.action_dim} actions")
        print("Loaded MLP network from {}".format(path))

    def to(self, device):
        self.actor = self.actor.to(device)
        return self

    def eval(self):
        return self

    def forward(self, x):
        return self.actor(x)

    __call__ = forward
