"""Test helper for the policy actor (csrc/agx_policy.hip, utils/policy.py): the three actors the reference trained
(tests/golden/policy_*_actor.npz), random nets from a seeded CPU generator, the MLP stated in our own words in float64 with the
propagated order-independent error bound, the float32 numpy statements of input normalisation and sampling, the torch module
the tests compare the CPU path with, and a writer of synthetic rl_games checkpoints."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REAL_NETS = ("attitude", "lmf2_acceleration", "lmf2_velocity")
U = 2.0 ** -24  # unit roundoff of float32


def golden_path(name):
    return os.path.join(GOLDEN, f"policy_{name}_actor.npz")


def load_actor(name):
    """(weights, biases, logstd) of a real actor: float32 numpy, torch's [out][in]"""
    g = np.load(golden_path(name))
    count = sum(1 for k in g.files if k.startswith("w") and k[1:].isdigit())
    return [g[f"w{i}"] for i in range(count)], [g[f"b{i}"] for i in range(count)], g["logstd"]


def random_net(dims, gen, scale=1.0):
    """weights and biases uniform in +-scale / sqrt(fan-in), float32 numpy"""
    ws, bs = [], []
    for fin, fout in zip(dims[:-1], dims[1:]):
        bound = scale / np.sqrt(fin)
        ws.append(((torch.rand((fout, fin), generator=gen) * 2 - 1) * bound).float().numpy())
        bs.append(((torch.rand(fout, generator=gen) * 2 - 1) * bound).float().numpy())
    return ws, bs


def act64(x, activation):
    if activation == "elu":
        return torch.where(x > 0, x, torch.expm1(x))
    if activation == "relu":
        return torch.where(x < 0, torch.zeros_like(x), x)
    return x


def linear64(x, err, w, b):
    """y = W x + b in float64 from float32 operands, and the bound of a float32 evaluation in ANY summation order:
    E_y = |W| E_x + (K + 2) u (|W| (|x| + E_x) + |b|) -- the incoming error through |W|, K + 2 rounded additions of partial sums no
    larger than the magnitude sum"""
    w64, b64 = torch.as_tensor(w).double(), torch.as_tensor(b).double()
    y = F.linear(x, w64, b64)
    mag = F.linear(x.abs() + err, w64.abs(), b64.abs())
    return y, F.linear(err, w64.abs()) + (w64.shape[1] + 2) * U * mag


def mlp64(ws, bs, x, activation):
    """the net in float64 from float32 operands, end to end: (mean [N, out], bound [N, out], pre-activations per layer).
    bound: E_0 = 0, E_l = linear64's bound + u |y_l|: the activation is a contraction followed by one rounding."""
    x = torch.as_tensor(x).double()
    err = torch.zeros_like(x)
    pres = []
    for l, (w, b) in enumerate(zip(ws, bs)):
        pre, err = linear64(x, err, w, b)
        y = act64(pre, activation) if l + 1 < len(ws) else pre
        err = err + U * y.abs()
        pres.append(pre)
        x = y
    return x, err, pres


def norm_f32(x, mean, denom, clip):
    """rl_games' normalize_input in numpy float32, every operation rounded"""
    x, mean, denom = np.asarray(x, np.float32), np.asarray(mean, np.float32), np.asarray(denom, np.float32)
    v = ((x - mean).astype(np.float32) / denom).astype(np.float32)
    return np.clip(v, np.float32(-clip), np.float32(clip)).astype(np.float32)


def sample_f32(mu, eps, logstd, clamp=False):
    """a = mu + eps * exp(logstd) in numpy float32, every operation rounded: exp in float64 rounded once"""
    mu, eps = np.asarray(mu, np.float32), np.asarray(eps, np.float32)
    sigma = np.exp(np.asarray(logstd, np.float32).astype(np.float64)).astype(np.float32)
    t = (eps * sigma).astype(np.float32)
    a = (mu + t).astype(np.float32)
    return np.clip(a, np.float32(-1.0), np.float32(1.0)) if clamp else a


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Actor(torch.nn.Module):
    """the actor as tests/test_gpu_policy_transfer.py states it: Linear / ELU ..., Linear"""

    def __init__(self, ws, bs, logstd=None):
        super().__init__()
        self.layers = torch.nn.ModuleList()
        for w, b in zip(ws, bs):
            lin = torch.nn.Linear(w.shape[1], w.shape[0])
            lin.weight.data.copy_(torch.from_numpy(np.asarray(w)))
            lin.bias.data.copy_(torch.from_numpy(np.asarray(b)))
            self.layers.append(lin)
        if logstd is not None:
            self.logstd = torch.nn.Parameter(torch.from_numpy(np.asarray(logstd)), requires_grad=False)

    def forward(self, x):
        for lin in self.layers[:-1]:
            x = F.elu(lin(x))
        return self.layers[-1](x)


def rl_games_state_dict(ws, bs, logstd, running=None):
    """the `model` entry of an rl_games A2C continuous checkpoint around the given actor: the actor's keys, a value head (which a
    loader of the actor ignores) and, with running = (mean, var), the input normaliser"""
    sd = {}
    for i, (w, b) in enumerate(zip(ws[:-1], bs[:-1])):
        sd[f"a2c_network.actor_mlp.{2 * i}.weight"] = torch.from_numpy(np.array(w, np.float32))
        sd[f"a2c_network.actor_mlp.{2 * i}.bias"] = torch.from_numpy(np.array(b, np.float32))
    sd["a2c_network.mu.weight"] = torch.from_numpy(np.array(ws[-1], np.float32))
    sd["a2c_network.mu.bias"] = torch.from_numpy(np.array(bs[-1], np.float32))
    sd["a2c_network.sigma"] = torch.from_numpy(np.array(logstd, np.float32))
    sd["a2c_network.value.weight"] = torch.zeros(1, ws[-1].shape[1])
    sd["a2c_network.value.bias"] = torch.zeros(1)
    sd["value_mean_std.running_mean"] = torch.zeros(1)
    if running is not None:
        sd["running_mean_std.running_mean"] = torch.from_numpy(np.array(running[0], np.float32))
        sd["running_mean_std.running_var"] = torch.from_numpy(np.array(running[1], np.float32))
        sd["running_mean_std.count"] = torch.tensor(1000.0)
    return sd


def write_checkpoint(path, state_dict):
    torch.save({"model": state_dict, "epoch": 1, "frame": 1, "last_mean_rewards": 0.0}, str(path))
    return str(path)
