"""Test helper for the recurrent actor (csrc/agx_policy.hip k_recurrent_act, utils/policy.py RecurrentActor): the navigation actor
the reference trained (tests/golden/policy_lmf2_nav_recurrent_actor.npz), random nets from a seeded CPU generator, one step of the
actor stated in our own words in float64 with a propagated error bound, the gate arithmetic in rounded-operation float32 numpy,
and a writer of synthetic sample-factory experiments (checkpoint files, optionally a config.json).

A net is a dict: enc_weights, enc_biases (lists, torch's [out][in] / [out]), w_ih [3H][I], w_hh [3H][H], b_ih, b_hh [3H] (gate order
r, z, n), head_weight [P][H], head_bias [P], logstd (None: the head is adaptive, P = 2 A), input_norm (None or (mean, denom, clip)),
activation ("elu" / "relu").

The bound (step64).  u = 2^-24.  E_v is a bound on |float32 value - float64 value| of v.
  linear map y = W x + b with K inputs (policy_ref.linear64):  E_y = |W| E_x + (K + 2) u (|W| (|x| + E_x) + |b|): the incoming
    error through |W|, and K + 2 rounded additions of partial sums no larger than the magnitude sum, in ANY summation order.
  a rounded operation (+, -, *) adds u times the magnitude of its result; a product p = a b carries |a| E_b + |b| E_a + E_a E_b.
  an elementary function f with Lipschitz constant c adds c E_in + fn u |f|: c = 1 for ELU / ReLU and tanh, 1/4 for the sigmoid.
    fn = 1 unit (the default): one rounding, what the device's correctly rounded expm1_cw / sigmoid_cw / tanh_cw add.  fn = FN_TORCH
    = 4 units is for torch's float32 CPU functions alone, which the CPU path runs: they compose up to three <= 1-ulp operations
    (exp, add, divide).
  normaliser: d = x - mean, v = d / denom, clamp (a contraction): E_v = u |d| / |denom| + u |v|, and 0 where |v| - E_v >= clip:
    both precisions are clipped to the same value there.
  encoder: the linear map, then the activation, for every layer.
  cell, with the carried E_h of the state the step reads (0 for a state that was reset):
    gi, gh: the linear map from (x, E_x) and (h, E_h) -- E_h enters through |W_hh|.
    s = gi + gh:  E_s = E_gi + E_gh + u |s|;  r, z = sigmoid(s):  E = min(E_s / 4 + fn u, 1): both values lie in [0, 1].
    t = r gh_n:  E_t = |r| E_ghn + |gh_n| E_r + E_r E_ghn + u |t|;  a = gi_n + t:  E_a = E_gin + E_t + u |a|;  n = tanh(a):
      E_n = min(E_a + fn u |n|, 2): both values lie in [-1, 1].
    q = 1 - z: E_q = E_z + u |q|;  b = q n: E_b = |q| E_n + |n| E_q + E_q E_n + u |b|;  c = z h: E_c = |z| E_h + |h| E_z + E_z E_h +
      u |c| -- E_h enters through z, and E_z through |h|;  h' = b + c: E_h' = E_b + E_c + u |h'|.
  head: the linear map from (h', E_h').
Magnitudes are those of the float64 values plus their E where the float32 magnitude matters (the linear map's magnitude sum)."""
import json
import os

import numpy as np
import torch
from policy_ref import U, act64, bits, linear64, norm_f32, sample_f32  # noqa: F401  (the shared statements; tests take them from here too)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "policy_lmf2_nav_recurrent_actor.npz")
FN_TORCH = 4.0  # units of roundoff one of torch's float32 CPU elementary functions may add (docstring); the device's add 1
SF_EPSILON, SF_CLIP = 1e-5, 5.0


def sf_denom(var):
    """sqrt(float32(var) + 1e-5) in float32"""
    return np.sqrt(np.asarray(var).astype(np.float32) + np.float32(SF_EPSILON), dtype=np.float32)


_fixture = None


def load_fixture():
    """the reference's navigation actor as a net (the normaliser included), loaded once"""
    global _fixture
    if _fixture is None:
        g = np.load(FIXTURE)
        count = sum(1 for k in g.files if k.startswith("w") and k[1:].isdigit())
        _fixture = {"enc_weights": [g[f"w{i}"] for i in range(count)], "enc_biases": [g[f"b{i}"] for i in range(count)],
                    "w_ih": g["w_ih"], "w_hh": g["w_hh"], "b_ih": g["b_ih"], "b_hh": g["b_hh"], "head_weight": g["head_weight"],
                    "head_bias": g["head_bias"], "logstd": None, "activation": "elu", "obs_key": str(g["obs_key"]),
                    "running": (g["norm_mean"], g["norm_var"]),
                    "input_norm": (g["norm_mean"].astype(np.float32), sf_denom(g["norm_var"]), SF_CLIP)}
    return _fixture


def _uniform(shape, bound, gen):
    return ((torch.rand(shape, generator=gen) * 2 - 1) * bound).float().numpy()


def random_net(dims, hidden, actions, gen, adaptive=True, activation="elu", scale=1.5):
    """encoder widths dims = [in, ..., cell input], a GRU of `hidden`, a head of 2 * actions (adaptive) or actions outputs with a
    constant log-std; weights and biases uniform in +-scale / sqrt(fan-in)"""
    net = {"enc_weights": [], "enc_biases": [], "activation": activation, "input_norm": None}
    for fin, fout in zip(dims[:-1], dims[1:]):
        net["enc_weights"].append(_uniform((fout, fin), scale / np.sqrt(fin), gen))
        net["enc_biases"].append(_uniform((fout,), scale / np.sqrt(fin), gen))
    k = scale / np.sqrt(hidden)
    net["w_ih"], net["w_hh"] = _uniform((3 * hidden, dims[-1]), k, gen), _uniform((3 * hidden, hidden), k, gen)
    net["b_ih"], net["b_hh"] = _uniform((3 * hidden,), k, gen), _uniform((3 * hidden,), k, gen)
    P = 2 * actions if adaptive else actions
    net["head_weight"], net["head_bias"] = _uniform((P, hidden), k, gen), _uniform((P,), k, gen)
    net["logstd"] = None if adaptive else _uniform((actions,), 1.0, gen)
    return net


def actor_kwargs(net):
    """the keyword arguments of RecurrentActor.from_arrays"""
    keys = ("enc_weights", "enc_biases", "w_ih", "w_hh", "b_ih", "b_hh", "head_weight", "head_bias", "logstd", "activation", "input_norm")
    return {k: net[k] for k in keys}


def num_actions(net):
    P = net["head_weight"].shape[0]
    return P // 2 if net["logstd"] is None else P


# ---- float64 with the bound ------------------------------------------------------------------------------------------------------
def step64(net, obs, h, err_h, flagged=None, reset="before", fn=1.0):
    """one call in float64 from float32 operands.  obs [N, in] float32, h [N, H] float64 (the stored state), err_h its bound,
    flagged: bool [N] or None.  Returns a dict of float64 tensors: mean, logstd, hidden (what is stored), and the bounds err_mean,
    err_logstd, err_hidden (docstring of this module); fn: units of roundoff per elementary function."""
    x = torch.as_tensor(obs).double()
    err = torch.zeros_like(x)
    if net["input_norm"] is not None:
        mean, denom, clip = net["input_norm"]
        d = x - torch.as_tensor(mean).double()
        den = torch.as_tensor(denom).double()
        v = d / den
        err = U * d.abs() / den.abs() + U * v.abs()
        err = torch.where(v.abs() - err >= clip, torch.zeros_like(err), err)  # beyond the clip in both precisions: exact
        x = v.clamp(-clip, clip)
    for w, b in zip(net["enc_weights"], net["enc_biases"]):
        pre, err = linear64(x, err, w, b)
        x = act64(pre, net["activation"])
        err = err + fn * U * x.abs()
    h = torch.as_tensor(h).double()
    err_h = torch.as_tensor(err_h).double()
    if flagged is not None and reset == "before":
        h = torch.where(flagged[:, None], torch.zeros_like(h), h)
        err_h = torch.where(flagged[:, None], torch.zeros_like(err_h), err_h)
    H = h.shape[1]
    gi, e_gi = linear64(x, err, net["w_ih"], net["b_ih"])
    gh, e_gh = linear64(h, err_h, net["w_hh"], net["b_hh"])
    s = gi[:, :2 * H] + gh[:, :2 * H]
    e_s = e_gi[:, :2 * H] + e_gh[:, :2 * H] + U * s.abs()
    rz = torch.sigmoid(s)
    e_rz = (e_s / 4 + fn * U).clamp(max=1.0)  # both values lie in [0, 1]
    r, z, e_r, e_z = rz[:, :H], rz[:, H:], e_rz[:, :H], e_rz[:, H:]
    gin, ghn, e_gin, e_ghn = gi[:, 2 * H:], gh[:, 2 * H:], e_gi[:, 2 * H:], e_gh[:, 2 * H:]
    t = r * ghn
    e_t = r.abs() * e_ghn + ghn.abs() * e_r + e_r * e_ghn + U * t.abs()
    a = gin + t
    e_a = e_gin + e_t + U * a.abs()
    n = torch.tanh(a)
    e_n = (e_a + fn * U * n.abs()).clamp(max=2.0)  # both values lie in [-1, 1]
    q = 1.0 - z
    e_q = e_z + U * q.abs()
    b = q * n
    e_b = q.abs() * e_n + n.abs() * e_q + e_q * e_n + U * b.abs()
    c = z * h
    e_c = z.abs() * err_h + h.abs() * e_z + e_z * err_h + U * c.abs()
    hn = b + c
    e_hn = e_b + e_c + U * hn.abs()
    y, e_y = linear64(hn, e_hn, net["head_weight"], net["head_bias"])
    A = num_actions(net)
    stored, e_stored = hn, e_hn
    if flagged is not None and reset == "after":
        stored = torch.where(flagged[:, None], torch.zeros_like(hn), hn)
        e_stored = torch.where(flagged[:, None], torch.zeros_like(e_hn), e_hn)
    if net["logstd"] is None:
        logstd, e_logstd = y[:, A:], e_y[:, A:]
    else:
        logstd = torch.as_tensor(net["logstd"]).double().expand(y.shape[0], A)
        e_logstd = torch.zeros_like(logstd)
    return {"mean": y[:, :A], "err_mean": e_y[:, :A], "logstd": logstd, "err_logstd": e_logstd, "hidden": stored, "err_hidden": e_stored}


# ---- float32, one rounding per operation -----------------------------------------------------------------------------------------
def sigmoid_f32(x):
    """float64 libm rounded once"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    return (1.0 / (1.0 + np.exp(-x64))).astype(np.float32)


def tanh_f32(x):
    return np.tanh(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def gates_f32(gi, gh, h, sigmoid=sigmoid_f32, tanh=tanh_f32):
    """h' [N, H] of gi, gh [N, 3H] and h [N, H] in numpy float32, every operation rounded once:
    r = sigmoid(gi_r + gh_r); z = sigmoid(gi_z + gh_z); n = tanh(gi_n + r * gh_n); a = 1 - z; b = a * n; c = z * h; h' = b + c"""
    gi, gh, h = (np.asarray(v, np.float32) for v in (gi, gh, h))
    H = h.shape[1]
    r = sigmoid((gi[:, :H] + gh[:, :H]).astype(np.float32))
    z = sigmoid((gi[:, H:2 * H] + gh[:, H:2 * H]).astype(np.float32))
    t = (r * gh[:, 2 * H:]).astype(np.float32)
    n = tanh((gi[:, 2 * H:] + t).astype(np.float32))
    a = (np.float32(1.0) - z).astype(np.float32)
    b = (a * n).astype(np.float32)
    c = (z * h).astype(np.float32)
    return (b + c).astype(np.float32)


# ---- torch's own GRU on the same weights ----------------------------------------------------------------------------------------
class TorchActor(torch.nn.Module):
    """nn.Sequential encoder + nn.GRU + nn.Linear, as sample-factory assembles them"""

    def __init__(self, net):
        super().__init__()
        layers = []
        for w, b in zip(net["enc_weights"], net["enc_biases"]):
            lin = torch.nn.Linear(w.shape[1], w.shape[0])
            lin.weight.data.copy_(torch.from_numpy(np.asarray(w)))
            lin.bias.data.copy_(torch.from_numpy(np.asarray(b)))
            layers += [lin, torch.nn.ELU() if net["activation"] == "elu" else torch.nn.ReLU()]
        self.encoder = torch.nn.Sequential(*layers)
        H = net["w_hh"].shape[1]
        self.core = torch.nn.GRU(net["w_ih"].shape[1], H)
        for name, key in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
            getattr(self.core, name).data.copy_(torch.from_numpy(np.asarray(net[key])))
        self.head = torch.nn.Linear(H, net["head_weight"].shape[0])
        self.head.weight.data.copy_(torch.from_numpy(np.asarray(net["head_weight"])))
        self.head.bias.data.copy_(torch.from_numpy(np.asarray(net["head_bias"])))
        self.norm = net["input_norm"]

    @torch.no_grad()
    def forward(self, obs, h):
        x = obs
        if self.norm is not None:
            mean, denom, clip = self.norm
            x = torch.clamp((x - torch.from_numpy(mean)) / torch.from_numpy(denom), -clip, clip)
        out, hn = self.core(self.encoder(x).unsqueeze(0), h.unsqueeze(0))
        return self.head(out.squeeze(0)), hn.squeeze(0)


# ---- synthetic sample-factory experiments ---------------------------------------------------------------------------------------
def sf_state_dict(net, obs_key="obs", running=None):
    """the `model` entry of a sample-factory checkpoint around the net: the actor's keys, the critic head and the returns
    normaliser (which a loader of the actor ignores) and, with running = (mean, var) in float64, the observation normaliser"""
    t = lambda a: torch.from_numpy(np.array(a))  # noqa: E731
    sd = {}
    if running is not None:
        prefix = f"obs_normalizer.running_mean_std.running_mean_std.{obs_key}."
        sd[prefix + "running_mean"], sd[prefix + "running_var"] = t(np.asarray(running[0], np.float64)), t(np.asarray(running[1], np.float64))
        sd[prefix + "count"] = torch.ones(1, dtype=torch.float64)
    sd["returns_normalizer.running_mean"] = torch.zeros(1, dtype=torch.float64)
    sd["returns_normalizer.running_var"] = torch.ones(1, dtype=torch.float64)
    sd["returns_normalizer.count"] = torch.ones(1, dtype=torch.float64)
    for i, (w, b) in enumerate(zip(net["enc_weights"], net["enc_biases"])):
        sd[f"encoder.encoders.{obs_key}.mlp_head.{2 * i}.weight"], sd[f"encoder.encoders.{obs_key}.mlp_head.{2 * i}.bias"] = t(w), t(b)
    for name, key in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
        sd["core.core." + name] = t(net[key])
    sd["critic_linear.weight"], sd["critic_linear.bias"] = torch.zeros(1, net["w_hh"].shape[1]), torch.zeros(1)
    sd["action_parameterization.distribution_linear.weight"] = t(net["head_weight"])
    sd["action_parameterization.distribution_linear.bias"] = t(net["head_bias"])
    if net["logstd"] is not None:
        sd["action_parameterization.learned_stddev"] = t(net["logstd"])
    return sd


SF_CONFIG = {"rnn_type": "gru", "rnn_num_layers": 1, "nonlinearity": "elu", "decoder_mlp_layers": [], "continuous_tanh_scale": 0.0,
             "obs_subtract_mean": 0.0, "obs_scale": 1.0, "normalize_input": True, "use_rnn": True, "rnn_size": 64}


def write_experiment(train_dir, experiment, files, config=None, policy_index=0):
    """<train_dir>/<experiment>/checkpoint_p<i>/<name> for every (name, state dict) of `files`, and config.json when given;
    returns the checkpoint directory"""
    root = os.path.join(str(train_dir), experiment)
    ckdir = os.path.join(root, f"checkpoint_p{policy_index}")
    os.makedirs(ckdir, exist_ok=True)
    for name, sd in files.items():
        torch.save({"train_step": 1, "env_steps": 1, "best_performance": 0.0, "model": sd, "curr_lr": 1e-4}, os.path.join(ckdir, name))
    if config is not None:
        with open(os.path.join(root, "config.json"), "w") as f:
            json.dump(config, f)
    return ckdir
