"""ActorMLP: a trained actor network in the loop -- observations in, actions out, one launch of the HIP library
(csrc/agx_policy.hip: every layer on the exact-fp32 matrix instruction, activations in LDS, rl_games' input normalisation,
sampling and clamping in the same kernel).  It replaces the torch module the reference puts between two task.step() calls
(examples/rl_games_example/rl_games_inference.py) and what rl_games' player does around it.

On a CPU device the same net is evaluated with torch.nn.functional.linear: the loader, the plumbing and the examples run without
a GPU.  On a HIP device there is no torch path: a missing kernel is an error."""
import ctypes as C
import re

import numpy as np
import torch

from .. import _lib

ACTIVATIONS = {"none": _lib.POLICY_NONE, None: _lib.POLICY_NONE, "elu": _lib.POLICY_ELU, "relu": _lib.POLICY_RELU}
NORM_EPSILON = 1e-5  # rl_games RunningMeanStd: (x - mean) / sqrt(var + epsilon)
NORM_CLIP = 5.0      # ... clamped to +-5
# what a checkpoint of rl_games' A2C continuous model holds besides the actor; not needed to act
_IGNORED_PREFIXES = ("a2c_network.value.", "a2c_network.critic_mlp.", "value_mean_std.", "running_mean_std.count")


def _arr(a):
    return np.ascontiguousarray(np.asarray(a, np.float32))


def _f32(t):
    """a checkpoint's tensor as contiguous float32 numpy"""
    return np.ascontiguousarray(torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous().numpy())


def check_dims(dims):
    """the limits of agx_policy_create for layer widths [in, hidden..., out] (ValueError names the offending number); returns the
    bytes of LDS a workgroup uses.  Host only: works without a GPU."""
    dims = [int(d) for d in dims]
    arr = (C.c_int32 * len(dims))(*dims)
    lds = C.c_size_t(0)
    lib = _lib.load()
    if lib.agx_policy_check(len(dims) - 1, arr, C.byref(lds)) != 0:
        raise ValueError(lib.agx_last_error().decode("utf-8", "replace"))
    return int(lds.value)


def pack_layer(w, pad_rows_to=1):
    """torch's [out][in] -> the kernel's [K8][Cout] (float32 numpy), the rows padded with zeros to a multiple of `pad_rows_to`
    first (32 for the last layer): what agx_policy_create uploads"""
    from .vae.vae_image_encoder import pack_weight

    w = np.asarray(w, np.float32)
    rows = -(-w.shape[0] // pad_rows_to) * pad_rows_to
    padded = np.zeros((rows, w.shape[1]), np.float32)
    padded[:w.shape[0]] = w
    return pack_weight(padded)


def actor_arrays_from_state_dict(sd):
    """(weights, biases, logstd, input_norm) of an rl_games A2C state dict (`torch.load(path)["model"]`): the layers
    a2c_network.actor_mlp.{0,2,4,...} and a2c_network.mu, the per-action a2c_network.sigma, running_mean_std when present.
    KeyError / ValueError name the key or the width that does not fit."""
    layers = {}
    known = set()
    for key in sd:
        m = re.fullmatch(r"a2c_network\.actor_mlp\.(\d+)\.(weight|bias)", str(key))
        if m:
            layers.setdefault(int(m.group(1)), {})[m.group(2)] = key
            known.add(key)
    for key in sd:
        k = str(key)
        if key in known or k in ("a2c_network.mu.weight", "a2c_network.mu.bias", "a2c_network.sigma", "running_mean_std.running_mean",
                                 "running_mean_std.running_var") or k.startswith(_IGNORED_PREFIXES):
            continue
        raise ValueError(f"rl_games checkpoint: key {k!r} is not part of a plain actor MLP with a per-action sigma (separate sigma "
                         "networks, recurrent cores and CNN front ends are not supported)")
    for idx in sorted(layers):
        if idx % 2 != 0:
            raise ValueError(f"rl_games checkpoint: 'a2c_network.actor_mlp.{idx}' holds parameters; Linear layers sit at the even indices")
    count = len(layers)
    weights, biases = [], []
    names = [f"a2c_network.actor_mlp.{2 * i}" for i in range(count)] + ["a2c_network.mu"]
    for i, name in enumerate(names):
        for kind, dst in (("weight", weights), ("bias", biases)):
            key = f"{name}.{kind}"
            if key not in sd:
                raise KeyError(f"rl_games checkpoint has no {key!r} (layers found: {sorted(layers)}, then a2c_network.mu)")
            dst.append(_f32(sd[key]))
    logstd = _f32(sd["a2c_network.sigma"]) if "a2c_network.sigma" in sd else None
    input_norm = None
    if "running_mean_std.running_mean" in sd or "running_mean_std.running_var" in sd:
        for key in ("running_mean_std.running_mean", "running_mean_std.running_var"):
            if key not in sd:
                raise KeyError(f"rl_games checkpoint has no {key!r} next to the other half of running_mean_std")
        mean, var = _f32(sd["running_mean_std.running_mean"]), _f32(sd["running_mean_std.running_var"])
        input_norm = (mean, np.sqrt(var + np.float32(NORM_EPSILON), dtype=np.float32), NORM_CLIP)
    return weights, biases, logstd, input_norm


class _Actor:
    """What ActorMLP and RecurrentActor share: validation, the env-step count of the generator, the buffers kept per batch size,
    the CPU statements of the normaliser and of sampling, and the library entries <_ENTRY>_{create, set_input_norm, set_logstd,
    noise, destroy}.  A subclass sets obs_dim, action_dim and logstd (None: no constant log-std) before _setup."""
    _ENTRY = None  # "agx_policy" / "agx_recurrent"

    @classmethod
    def _check_layers(cls, weights, biases, what):
        """(weights, biases, widths [in, out of layer 0, ...]) of a chain of Linear layers; `what` ("" or "encoder ") names them"""
        name = cls.__name__
        weights, biases = [_arr(w) for w in weights], [_arr(b) for b in biases]
        if len(weights) != len(biases) or not weights:
            raise ValueError(f"{name}: {len(weights)} {what}weights and {len(biases)} biases")
        for l, (w, b) in enumerate(zip(weights, biases)):
            if w.ndim != 2 or b.shape != (w.shape[0],):
                raise ValueError(f"{name}: {what}layer {l}: weight {w.shape} and bias {b.shape} are not [out, in] and [out]")
            if l and w.shape[1] != weights[l - 1].shape[0]:
                raise ValueError(f"{name}: {what}layer {l} reads {w.shape[1]} inputs, layer {l - 1} writes {weights[l - 1].shape[0]}")
        return weights, biases, [weights[0].shape[1]] + [w.shape[0] for w in weights]

    def _setup(self, input_norm, device, task, rng_seed, env_index_base):
        self.input_norm = None
        if input_norm is not None:
            mean, denom, clip = input_norm
            mean, denom = _arr(mean).reshape(-1), _arr(denom).reshape(-1)
            if mean.shape != (self.obs_dim,) or denom.shape != (self.obs_dim,):
                raise ValueError(f"{type(self).__name__}: input_norm of widths {mean.size} / {denom.size}, the net reads {self.obs_dim} inputs")
            self.input_norm = (mean, denom, float(clip))
        self.device = str(device)
        self.task = task
        env = getattr(task, "sim_env", None)
        self.rng_seed = int(rng_seed if rng_seed is not None else getattr(env, "rng_seed", 0)) & 0xFFFFFFFFFFFFFFFF
        self.env_index_base = int(env_index_base if env_index_base is not None else getattr(env, "env_offset", 0))
        self.step = 0  # the env step of the next sampled call without `step=` and without a task
        self.mean = None
        self._out = {}
        self._handle = None
        self._is_cpu = torch.device(self.device).type == "cpu"

    def _create(self, *args):
        """<_ENTRY>_create(*args, &handle) on this actor's device, then the normaliser and the constant log-std"""
        self._lib = _lib.load()
        handle = C.c_void_p()
        with torch.cuda.device(torch.device(self.device)):
            self._entry("create", *args, C.byref(handle))
            self._handle = handle
            if self.input_norm is not None:
                mean, denom, clip = self.input_norm
                self._entry("set_input_norm", handle, mean.ctypes.data, denom.ctypes.data, clip)
            if self.logstd is not None:
                self._entry("set_logstd", handle, self.logstd.ctypes.data)

    def _entry(self, which, *args):
        name = f"{self._ENTRY}_{which}"
        _lib.check(getattr(self._lib, name)(*args), name)

    def __del__(self):
        handle, self._handle = getattr(self, "_handle", None), None
        if handle:
            getattr(self._lib, f"{self._ENTRY}_destroy")(handle)

    def _check_obs(self, obs):
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim or obs.dtype is not torch.float32:
            raise ValueError(f"{type(self).__name__}: observations must be float32 [N, {self.obs_dim}], got {obs.dtype} {tuple(obs.shape)}")
        return obs.shape[0]

    def _check_eps(self, eps, n):
        if eps is not None and (tuple(eps.shape) != (n, self.action_dim) or eps.dtype is not torch.float32):
            raise ValueError(f"{type(self).__name__}: eps must be float32 [{n}, {self.action_dim}]")

    def _buffers(self, n, count):
        """`count` tensors [n, action_dim] kept per batch size: the actions without out=, the mean (and the log-std)"""
        bufs = self._out.get(n)
        if bufs is None:
            bufs = self._out[n] = tuple(torch.empty((n, self.action_dim), dtype=torch.float32, device=self.device) for _ in range(count))
        return bufs

    def _check_out(self, out, buf, n):
        """out= when given, else the kept buffer"""
        if out is None:
            return buf
        if tuple(out.shape) != (n, self.action_dim) or out.dtype is not torch.float32:
            raise ValueError(f"{type(self).__name__}: out must be float32 [{n}, {self.action_dim}]")
        return out

    def _env_step(self, step, sample):
        if step is not None:
            return int(step)
        env = getattr(self.task, "sim_env", None)
        if env is not None:
            return int(env.step_counter)
        s = self.step
        if sample:
            self.step += 1
        return s

    @staticmethod
    def _flag_word(sample, clamp):
        return (_lib.POLICY_SAMPLE if sample else 0) | (_lib.POLICY_CLAMP if clamp else 0)

    def _normalise_cpu(self, x):
        if self.input_norm is None:
            return x
        m, d, clip = self.input_norm
        return torch.clamp((x - torch.from_numpy(m)) / torch.from_numpy(d), -clip, clip)

    def _emit_cpu(self, mean, logstd, out, sample, clamp, eps):
        """out <- mean -> (sample with sigma = exp(logstd)) -> (clamp)"""
        a = mean
        if sample:
            if eps is None:
                raise ValueError(f"{type(self).__name__} on a CPU device has no generator: pass eps= to sample")
            a = mean + eps * torch.exp(logstd)
        if clamp:
            a = a.clamp(-1.0, 1.0)
        out.copy_(a)

    def noise(self, n, step):
        """[n, action_dim]: the normals a sampled call without eps draws at env step `step` (diagnostic; one stream for both actors)"""
        if self._is_cpu:
            raise RuntimeError(f"{type(self).__name__}.noise: the generator lives in the HIP library; this actor is on a CPU device")
        out = torch.empty((n, self.action_dim), dtype=torch.float32, device=self.device)
        self._entry("noise", self._handle, n, self.rng_seed, self.env_index_base, int(step) & 0x7FFFFFFF, _lib.dptr(out), _lib.current_stream(self.device))
        return out


def _pointers(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


class ActorMLP(_Actor):
    """actor(obs) -> actions [N, A].  Build with from_arrays or from_rl_games_checkpoint."""
    _ENTRY = "agx_policy"

    def __init__(self, weights, biases, logstd=None, activation="elu", input_norm=None, device="cuda:0", task=None, rng_seed=None,
                 env_index_base=None):
        if activation not in ACTIVATIONS:
            raise ValueError(f"ActorMLP: activation {activation!r}; supported: 'none', 'elu', 'relu'")
        self.activation = activation if activation is not None else "none"
        self.weights, self.biases, self.dims = self._check_layers(weights, biases, "")
        self.lds_bytes = check_dims(self.dims)
        self.obs_dim, self.action_dim = self.dims[0], self.dims[-1]
        self.logstd = None if logstd is None else _arr(logstd).reshape(-1)
        if self.logstd is not None and self.logstd.shape != (self.action_dim,):
            raise ValueError(f"ActorMLP: logstd has {self.logstd.size} entries, the net has {self.action_dim} actions")
        self._setup(input_norm, device, task, rng_seed, env_index_base)
        if self._is_cpu:
            self._cpu = [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in zip(self.weights, self.biases)]
        else:
            self._create(len(self.weights), (C.c_int32 * len(self.dims))(*self.dims), _pointers(self.weights), _pointers(self.biases),
                         ACTIVATIONS[self.activation])

    # ---- constructors ----------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, weights, biases, logstd=None, activation="elu", input_norm=None, device="cuda:0", **kw):
        return cls(weights, biases, logstd=logstd, activation=activation, input_norm=input_norm, device=device, **kw)

    @classmethod
    def from_rl_games_checkpoint(cls, path, device="cuda:0", activation="elu", **kw):
        """`torch.load(path)["model"]` of an rl_games A2C continuous agent (both recipes of the reference use ELU)"""
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if not isinstance(ck, dict) or "model" not in ck:
            raise KeyError(f"{path}: not an rl_games checkpoint (no 'model' entry)")
        weights, biases, logstd, input_norm = actor_arrays_from_state_dict(ck["model"])
        return cls(weights, biases, logstd=logstd, activation=activation, input_norm=input_norm, device=device, **kw)

    def to(self, device):
        """the same net on another device (a new handle there); self when it already lives on it"""
        if torch.device(device) == torch.device(self.device):
            return self
        return ActorMLP(self.weights, self.biases, logstd=self.logstd, activation=self.activation, input_norm=self.input_norm,
                        device=device, task=self.task, rng_seed=self.rng_seed, env_index_base=self.env_index_base)

    # ---- the call --------------------------------------------------------------------------------------------------------
    def __call__(self, obs, out=None, sample=False, clamp=False, eps=None, step=None):
        """obs [N, obs_dim] float32 -> actions [N, action_dim]; `actor.mean` then holds the mean of this call.  sample: a = mu +
        eps * exp(logstd), eps given ([N, action_dim]) or drawn by the library's generator at (rng_seed, env_index_base + env,
        step, action) -- step: the task's env step, or this object's own count of sampled calls.  clamp: to [-1, 1], last.
        Without out= the result lives in a buffer kept per batch size: the next call of that size overwrites it."""
        n = self._check_obs(obs)
        if sample and self.logstd is None:
            raise ValueError("ActorMLP: sample=True needs a logstd (the checkpoint's a2c_network.sigma)")
        self._check_eps(eps, n)
        buf, mean = self._buffers(n, 2)
        out = self._check_out(out, buf, n)
        env_step = self._env_step(step, sample and eps is None)
        if self._is_cpu:
            return self._call_cpu(obs, out, mean, sample, clamp, eps)
        if not obs.is_contiguous():
            obs = obs.contiguous()
        p = _lib.dptr
        _lib.check(self._lib.agx_policy_act(self._handle, n, p(obs), p(out), p(mean), p(eps) if sample else None, self._flag_word(sample, clamp),
                                            self.rng_seed, self.env_index_base, env_step & 0x7FFFFFFF, _lib.current_stream(self.device)),
                   "agx_policy_act")
        self.mean = mean
        return out

    def _call_cpu(self, obs, out, mean, sample, clamp, eps):
        x = self._normalise_cpu(obs)
        last = len(self._cpu) - 1
        for l, (w, b) in enumerate(self._cpu):
            x = torch.nn.functional.linear(x, w, b)
            if l < last:
                if self.activation == "elu":
                    x = torch.nn.functional.elu(x)
                elif self.activation == "relu":
                    x = torch.relu(x)
        mean.copy_(x)
        self._emit_cpu(mean, torch.from_numpy(self.logstd) if sample else None, out, sample, clamp, eps)
        self.mean = mean
        return out


# ---- recurrent actors: sample-factory's encoder MLP -> GRU -> linear head --------------------------------------------------------
SF_NORM_EPSILON = 1e-5  # sample-factory RunningMeanStdInPlace: (x - mean) / sqrt(var + eps) ...
SF_NORM_CLIP = 5.0      # ... clamped to +-5 (its published defaults: epsilon=1e-5, clip=5.0)
_SF_IGNORED_PREFIXES = ("critic_linear.", "returns_normalizer.")
_SF_NORM = r"obs_normalizer\.running_mean_std\.running_mean_std\.([^.]+)\.(running_mean|running_var|count)"
_SF_ENC = r"encoder\.encoders\.([^.]+)\.mlp_head\.(\d+)\.(weight|bias)"
_SF_CORE = ("core.core.weight_ih_l0", "core.core.weight_hh_l0", "core.core.bias_ih_l0", "core.core.bias_hh_l0")
_SF_HEAD = ("action_parameterization.distribution_linear.weight", "action_parameterization.distribution_linear.bias")
_SF_STDDEV = "action_parameterization.learned_stddev"


def check_recurrent_dims(dims, hidden, head_out):
    """the limits of agx_recurrent_create for encoder widths [in, ..., cell input], the hidden size and the head's width
    (ValueError names the offending number); returns the bytes of LDS a workgroup uses.  Host only."""
    dims = [int(d) for d in dims]
    lds = C.c_size_t(0)
    lib = _lib.load()
    if lib.agx_recurrent_check(len(dims) - 1, (C.c_int32 * len(dims))(*dims), int(hidden), int(head_out), C.byref(lds)) != 0:
        raise ValueError(lib.agx_last_error().decode("utf-8", "replace"))
    return int(lds.value)


def recurrent_arrays_from_state_dict(sd):
    """the arrays of a sample-factory actor-critic state dict (`torch.load(path)["model"]`) with one observation key, an MLP
    encoder, a one-layer GRU core and a linear action head: a dict with obs_key, enc_weights, enc_biases, w_ih, w_hh, b_ih, b_hh,
    head_weight, head_bias, logstd (None when the head is adaptive) and input_norm (None or (mean, denom, clip)).  ValueError /
    KeyError name the key that does not fit."""
    enc, norm, obs_keys = {}, {}, set()
    for key in sd:
        k = str(key)
        m = re.fullmatch(_SF_ENC, k)
        if m:
            obs_keys.add(m.group(1))
            enc.setdefault(int(m.group(2)), {})[m.group(3)] = key
            continue
        m = re.fullmatch(_SF_NORM, k)
        if m:
            obs_keys.add(m.group(1))
            norm[m.group(2)] = key
            continue
        if k in _SF_CORE or k in _SF_HEAD or k == _SF_STDDEV or k.startswith(_SF_IGNORED_PREFIXES) or k.endswith(".count"):
            continue
        if re.fullmatch(r"core\.core\.(weight|bias)_(ih|hh)_l[1-9]\d*(_reverse)?", k) or k.endswith("_reverse"):
            raise ValueError(f"sample-factory checkpoint: key {k!r}: only a one-layer, one-direction core is supported")
        raise ValueError(f"sample-factory checkpoint: key {k!r} is not part of an actor with one MLP encoder, one GRU layer and a linear "
                         "action head (decoder layers, conv encoders, separate actor_encoder / critic_encoder and LSTM cores are not supported)")
    if len(obs_keys) != 1:
        raise ValueError(f"sample-factory checkpoint: observation keys {sorted(obs_keys)}: exactly one is supported")
    obs_key = next(iter(obs_keys))
    if not enc:
        raise KeyError(f"sample-factory checkpoint has no 'encoder.encoders.{obs_key}.mlp_head.0.weight'")
    for idx in sorted(enc):
        if idx % 2 != 0:
            raise ValueError(f"sample-factory checkpoint: 'encoder.encoders.{obs_key}.mlp_head.{idx}' holds parameters; Linear layers sit at "
                             "the even indices")
    out = {"obs_key": obs_key, "enc_weights": [], "enc_biases": []}
    for i in range(len(enc)):
        for kind, dst in (("weight", out["enc_weights"]), ("bias", out["enc_biases"])):
            key = f"encoder.encoders.{obs_key}.mlp_head.{2 * i}.{kind}"
            if key not in sd:
                raise KeyError(f"sample-factory checkpoint has no {key!r} (layers found: {sorted(enc)})")
            dst.append(_f32(sd[key]))
    for key in _SF_CORE + _SF_HEAD:
        if key not in sd:
            raise KeyError(f"sample-factory checkpoint has no {key!r}")
    w_ih, w_hh, b_ih, b_hh = (_f32(sd[k]) for k in _SF_CORE)
    hidden = w_hh.shape[1]
    for name, arr, want in (("core.core.weight_ih_l0", w_ih, (3 * hidden, out["enc_weights"][-1].shape[0])),
                            ("core.core.weight_hh_l0", w_hh, (3 * hidden, hidden)), ("core.core.bias_ih_l0", b_ih, (3 * hidden,)),
                            ("core.core.bias_hh_l0", b_hh, (3 * hidden,))):
        if arr.shape != want:
            kind = " (4 x hidden rows: an LSTM)" if arr.shape[0] == 4 * hidden else ""
            raise ValueError(f"sample-factory checkpoint: {name!r} has shape {arr.shape}{kind}; a GRU of hidden size {hidden} has {want}")
    out.update(w_ih=w_ih, w_hh=w_hh, b_ih=b_ih, b_hh=b_hh, head_weight=_f32(sd[_SF_HEAD[0]]), head_bias=_f32(sd[_SF_HEAD[1]]))
    out["logstd"] = _f32(sd[_SF_STDDEV]).reshape(-1) if _SF_STDDEV in sd else None
    out["input_norm"] = None
    if "running_mean" in norm or "running_var" in norm:
        for kind in ("running_mean", "running_var"):
            if kind not in norm:
                raise KeyError(f"sample-factory checkpoint has no 'obs_normalizer.running_mean_std.running_mean_std.{obs_key}.{kind}' next to "
                               "the other half of the normaliser")
        mean, var = _f32(sd[norm["running_mean"]]), _f32(sd[norm["running_var"]])  # float64 in the file: rounded to float32 first
        out["input_norm"] = (mean, np.sqrt(var + np.float32(SF_NORM_EPSILON), dtype=np.float32), SF_NORM_CLIP)
    return out


def _check_sf_config(cfg, where):
    """the entries of a sample-factory config.json this actor depends on (ValueError names the entry); returns normalize_input"""
    want = (("rnn_type", lambda v: v == "gru", "'gru'"), ("rnn_num_layers", lambda v: v == 1, "1"),
            ("nonlinearity", lambda v: v in ("elu", "relu"), "'elu' or 'relu'"), ("decoder_mlp_layers", lambda v: list(v) == [], "[]"),
            ("continuous_tanh_scale", lambda v: float(v) == 0.0, "0"), ("obs_subtract_mean", lambda v: float(v) == 0.0, "0"),
            ("obs_scale", lambda v: float(v) == 1.0, "1"))
    for name, ok, text in want:
        if name in cfg and not ok(cfg[name]):
            raise ValueError(f"{where}: {name} = {cfg[name]!r}; supported: {text}")
    return bool(cfg.get("normalize_input", True))


def find_sample_factory_checkpoint(path_or_dir, kind="best"):
    """a .pth file as it is; of a checkpoint_p0 directory the newest best_* (kind 'best') or checkpoint_* (kind 'latest')"""
    import glob
    import os

    path = str(path_or_dir)
    if os.path.isfile(path):
        return path
    if kind not in ("best", "latest"):
        raise ValueError(f"load_checkpoint_kind {kind!r}; supported: 'best', 'latest'")
    prefix = {"best": "best", "latest": "checkpoint"}[kind]
    found = sorted(glob.glob(os.path.join(path, f"{prefix}_*")))  # zero-padded train step in the name: sorted = oldest first
    if not found:
        raise FileNotFoundError(f"{path}: no {prefix}_* checkpoint")
    return found[-1]


class RecurrentActor(_Actor):
    """actor(obs, done) -> actions [N, A] of an encoder MLP -> GRU cell -> linear head; the state lives in `actor.hidden` [N, H].
    Build with from_arrays or from_sample_factory_checkpoint."""
    _ENTRY = "agx_recurrent"

    def __init__(self, enc_weights, enc_biases, w_ih, w_hh, b_ih, b_hh, head_weight, head_bias, logstd=None, activation="elu", input_norm=None,
                 device="cuda:0", task=None, rng_seed=None, env_index_base=None):
        if activation not in ("elu", "relu"):
            raise ValueError(f"RecurrentActor: activation {activation!r}; supported: 'elu', 'relu'")
        self.activation = activation
        self.enc_weights, self.enc_biases, self.dims = self._check_layers(enc_weights, enc_biases, "encoder ")
        self.w_ih, self.w_hh, self.b_ih, self.b_hh = _arr(w_ih), _arr(w_hh), _arr(b_ih).reshape(-1), _arr(b_hh).reshape(-1)
        self.head_weight, self.head_bias = _arr(head_weight), _arr(head_bias).reshape(-1)
        if self.w_hh.ndim != 2 or self.w_hh.shape[0] != 3 * self.w_hh.shape[1]:
            raise ValueError(f"RecurrentActor: w_hh {self.w_hh.shape} is not [3 H, H] (a GRU, gates r, z, n)")
        self.hidden_dim = H = self.w_hh.shape[1]
        if self.w_ih.shape != (3 * H, self.dims[-1]) or self.b_ih.shape != (3 * H,) or self.b_hh.shape != (3 * H,):
            raise ValueError(f"RecurrentActor: w_ih {self.w_ih.shape}, b_ih {self.b_ih.shape}, b_hh {self.b_hh.shape} do not fit a GRU of "
                             f"{self.dims[-1]} inputs and hidden size {H}")
        if self.head_weight.ndim != 2 or self.head_weight.shape[1] != H or self.head_bias.shape != (self.head_weight.shape[0],):
            raise ValueError(f"RecurrentActor: head weight {self.head_weight.shape} and bias {self.head_bias.shape} do not read {H} inputs")
        P = self.head_weight.shape[0]
        self.logstd = None if logstd is None else _arr(logstd).reshape(-1)
        self.adaptive = self.logstd is None
        if self.adaptive and P % 2:
            raise ValueError(f"RecurrentActor: an adaptive head emits means and log-std: {P} outputs is odd (pass logstd= for a constant one)")
        self.action_dim = P // 2 if self.adaptive else P
        if not self.adaptive and self.logstd.shape != (self.action_dim,):
            raise ValueError(f"RecurrentActor: logstd has {self.logstd.size} entries, the head has {self.action_dim} actions")
        if not 1 <= self.action_dim <= 64:
            raise ValueError(f"RecurrentActor: {self.action_dim} actions; supported: 1 .. 64")
        self.obs_dim = self.dims[0]
        self.lds_bytes = check_recurrent_dims(self.dims, H, P)
        self._setup(input_norm, device, task, rng_seed, env_index_base)
        self.hidden = None  # [N, H], allocated by the first call
        self.logstd_out = None
        self._may_resize = True
        if self._is_cpu:
            t = torch.from_numpy
            self._cpu = {"enc": [(t(w), t(b)) for w, b in zip(self.enc_weights, self.enc_biases)], "ih": (t(self.w_ih), t(self.b_ih)),
                         "hh": (t(self.w_hh), t(self.b_hh)), "head": (t(self.head_weight), t(self.head_bias))}
        else:
            self._create(len(self.enc_weights), (C.c_int32 * len(self.dims))(*self.dims), H, self.action_dim, int(self.adaptive),
                         _pointers(self.enc_weights), _pointers(self.enc_biases), self.w_ih.ctypes.data, self.w_hh.ctypes.data, self.b_ih.ctypes.data,
                         self.b_hh.ctypes.data, self.head_weight.ctypes.data, self.head_bias.ctypes.data, ACTIVATIONS[activation])

    # ---- constructors ----------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, enc_weights, enc_biases, w_ih, w_hh, b_ih, b_hh, head_weight, head_bias, logstd=None, activation="elu",
                    input_norm=None, device="cuda:0", **kw):
        return cls(enc_weights, enc_biases, w_ih, w_hh, b_ih, b_hh, head_weight, head_bias, logstd=logstd, activation=activation,
                   input_norm=input_norm, device=device, **kw)

    @classmethod
    def from_sample_factory_checkpoint(cls, path_or_dir, device="cuda:0", kind="best", **kw):
        """a .pth file of sample-factory, or its checkpoint_p0 directory (the newest best_* / checkpoint_* by `kind`).  A
        config.json beside checkpoint_p0 is read only to validate what this actor depends on and for the nonlinearity."""
        import json
        import os

        path = find_sample_factory_checkpoint(path_or_dir, kind)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if not isinstance(ck, dict) or "model" not in ck:
            raise KeyError(f"{path}: not a sample-factory checkpoint (no 'model' entry)")
        a = recurrent_arrays_from_state_dict(ck["model"])
        config = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(path))), "config.json")
        activation, normalize = kw.pop("activation", None), True
        if os.path.isfile(config):
            with open(config) as f:
                cfg = json.load(f)
            normalize = _check_sf_config(cfg, config)
            activation = activation or cfg.get("nonlinearity")
        actor = cls(a["enc_weights"], a["enc_biases"], a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"], a["head_weight"], a["head_bias"],
                    logstd=a["logstd"], activation=activation or "elu", input_norm=a["input_norm"] if normalize else None, device=device, **kw)
        actor.obs_key = a["obs_key"]
        return actor

    def to(self, device):
        """the same net on another device (a new handle and a fresh state there); self when it already lives on it"""
        if torch.device(device) == torch.device(self.device):
            return self
        return RecurrentActor(self.enc_weights, self.enc_biases, self.w_ih, self.w_hh, self.b_ih, self.b_hh, self.head_weight, self.head_bias,
                              logstd=self.logstd, activation=self.activation, input_norm=self.input_norm, device=device, task=self.task,
                              rng_seed=self.rng_seed, env_index_base=self.env_index_base)

    # ---- the state -------------------------------------------------------------------------------------------------------
    def allocate(self, n):
        """a zero state for n envs (what the first call does)"""
        self.hidden = torch.zeros((int(n), self.hidden_dim), dtype=torch.float32, device=self.device)
        self._may_resize = False
        return self.hidden

    def reset(self, env_ids=None):
        """zero the state rows `env_ids`; without ids all of them, and the next call may come with another batch size"""
        if env_ids is None:
            self._may_resize = True
            if self.hidden is not None:
                self.hidden.zero_()
        elif self.hidden is not None:
            self.hidden[env_ids] = 0.0

    # ---- the call --------------------------------------------------------------------------------------------------------
    def __call__(self, obs, done=None, reset="before", out=None, sample=False, clamp=False, eps=None, step=None):
        """obs [N, obs_dim] float32 -> actions [N, action_dim]; `actor.hidden` advances in place, `actor.mean` and
        `actor.logstd_out` then hold this call's values.  done: None, one bool / uint8 tensor [N] or a tuple of two (an env with
        either set is reset) -- `(task.terminations, task.truncations)` goes straight in.  reset "before": a flagged env is
        evaluated from a zero state (sample-factory's sampler, with the flags of the step that produced obs); "after": it is
        evaluated with the state it has, and zero is stored (the reference's dce_nn_navigation.py).  sample / clamp / eps / step
        / out as for ActorMLP; sigma = exp(logstd) of the head."""
        n = self._check_obs(obs)
        if reset not in ("before", "after"):
            raise ValueError(f"RecurrentActor: reset {reset!r}; supported: 'before', 'after'")
        self._check_eps(eps, n)
        if sample and eps is None and self._is_cpu:  # refused before the step count or the state moves
            raise ValueError("RecurrentActor on a CPU device has no generator: pass eps= to sample")
        flags = () if done is None else (tuple(done) if isinstance(done, (tuple, list)) else (done,))
        if len(flags) > 2:
            raise ValueError(f"RecurrentActor: done holds {len(flags)} tensors; one or two are supported")
        for f in flags:
            if tuple(f.shape) != (n,) or f.dtype not in (torch.bool, torch.uint8) or not f.is_contiguous():
                raise ValueError(f"RecurrentActor: a done tensor must be contiguous bool or uint8 [{n}], got {f.dtype} {tuple(f.shape)}")
        if self.hidden is None or (self.hidden.shape[0] != n and self._may_resize):
            self.allocate(n)
        elif self.hidden.shape[0] != n:
            raise ValueError(f"RecurrentActor: {n} envs, the state holds {self.hidden.shape[0]}: call reset() before changing the batch size")
        self._may_resize = False
        buf, mean, logstd_out = self._buffers(n, 3)
        out = self._check_out(out, buf, n)
        env_step = self._env_step(step, sample and eps is None)
        if self._is_cpu:
            return self._call_cpu(obs, flags, reset, out, mean, logstd_out, sample, clamp, eps)
        if not obs.is_contiguous():
            obs = obs.contiguous()
        bits = self._flag_word(sample, clamp) | (_lib.POLICY_RESET_AFTER if reset == "after" else 0)
        p = _lib.dptr
        _lib.check(self._lib.agx_recurrent_act(self._handle, n, p(obs), p(self.hidden), p(flags[0]) if flags else None,
                                               p(flags[1]) if len(flags) > 1 else None, p(out), p(mean), p(logstd_out), p(eps) if sample else None,
                                               bits, self.rng_seed, self.env_index_base, env_step & 0x7FFFFFFF, _lib.current_stream(self.device)),
                   "agx_recurrent_act")
        self.mean, self.logstd_out = mean, logstd_out
        return out

    def _call_cpu(self, obs, flags, reset, out, mean, logstd_out, sample, clamp, eps):
        F = torch.nn.functional
        x = self._normalise_cpu(obs)
        for w, b in self._cpu["enc"]:
            x = F.linear(x, w, b)
            x = F.elu(x) if self.activation == "elu" else torch.relu(x)
        flagged = None
        for f in flags:
            flagged = (f != 0) if flagged is None else (flagged | (f != 0))
        h = self.hidden
        if flagged is not None and reset == "before":
            h = torch.where(flagged[:, None], torch.zeros_like(h), h)
        H = self.hidden_dim
        gi, gh = F.linear(x, *self._cpu["ih"]), F.linear(h, *self._cpu["hh"])
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        c = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        hn = (1.0 - z) * c + z * h
        self.hidden.copy_(torch.where(flagged[:, None], torch.zeros_like(hn), hn) if flagged is not None and reset == "after" else hn)
        y = F.linear(hn, *self._cpu["head"])
        A = self.action_dim
        mean.copy_(y[:, :A])
        logstd_out.copy_(y[:, A:] if self.adaptive else torch.from_numpy(self.logstd).expand_as(mean))
        self._emit_cpu(mean, logstd_out, out, sample, clamp, eps)
        self.mean, self.logstd_out = mean, logstd_out
        return out


class SampleFactoryInference:
    """The surface of the reference's two inference classes around RecurrentActor (sim2real/nn_inference_class.py
    Sim2RealInferenceClass, examples/dce_rl_navigation/sf_inference_class.py NN_Inference_Class; they differ in the observation key
    alone): `cls(num_envs, num_actions, num_obs, cfg)`, `get_action(obs_dict)`, `reset(env_ids)`, `rnn_states`.  cfg: an object or
    dict with train_dir and experiment (the checkpoint is <train_dir>/<experiment>/checkpoint_p<policy_index>/), optionally
    load_checkpoint_kind ('latest', sample-factory's default, or 'best'), policy_index, eval_deterministic and device ('cpu', else the
    HIP device)."""

    def __init__(self, num_envs, num_actions, num_obs, cfg):
        import os

        get = cfg.get if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
        for name in ("train_dir", "experiment"):
            if get(name) is None:
                raise ValueError(f"cfg has no {name!r}")
        self.cfg = cfg
        self.num_agents, self.num_actions, self.num_obs = int(num_envs), int(num_actions), int(num_obs)
        self.eval_deterministic = bool(get("eval_deterministic", False))
        self.device = torch.device("cpu" if get("device") == "cpu" else "cuda:0")
        directory = os.path.join(str(get("train_dir")), str(get("experiment")), f"checkpoint_p{int(get('policy_index', 0) or 0)}")
        self.actor = RecurrentActor.from_sample_factory_checkpoint(directory, device=str(self.device), kind=get("load_checkpoint_kind", "latest"))
        if self.actor.obs_dim != self.num_obs or self.actor.action_dim != self.num_actions:
            raise ValueError(f"the actor of {directory} maps {self.actor.obs_dim} observations to {self.actor.action_dim} actions, not "
                             f"{self.num_obs} to {self.num_actions}")
        self.actor.allocate(self.num_agents)

    @property
    def rnn_states(self):
        return self.actor.hidden

    def reset(self, env_ids):
        self.actor.reset(env_ids)

    def get_action(self, obs, get_np=False, get_robot_zero=False):
        x = obs["obs"] if "obs" in obs else obs["observations"]
        x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
        sample = not self.eval_deterministic
        eps = torch.randn((x.shape[0], self.num_actions)) if sample and self.device.type == "cpu" else None
        actions = self.actor(x, sample=sample, eps=eps)
        if get_robot_zero:
            actions = actions[0]
        if get_np:
            return actions.cpu().numpy()
        return actions
