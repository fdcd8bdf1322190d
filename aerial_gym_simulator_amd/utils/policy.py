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
            dst.append(torch.as_tensor(sd[key]).detach().to("cpu", torch.float32).contiguous().numpy())
    logstd = None
    if "a2c_network.sigma" in sd:
        logstd = torch.as_tensor(sd["a2c_network.sigma"]).detach().to("cpu", torch.float32).contiguous().numpy()
    input_norm = None
    if "running_mean_std.running_mean" in sd or "running_mean_std.running_var" in sd:
        for key in ("running_mean_std.running_mean", "running_mean_std.running_var"):
            if key not in sd:
                raise KeyError(f"rl_games checkpoint has no {key!r} next to the other half of running_mean_std")
        mean = torch.as_tensor(sd["running_mean_std.running_mean"]).detach().to("cpu", torch.float32).numpy()
        var = torch.as_tensor(sd["running_mean_std.running_var"]).detach().to("cpu", torch.float32).numpy()
        input_norm = (mean, np.sqrt(var + np.float32(NORM_EPSILON), dtype=np.float32), NORM_CLIP)
    return weights, biases, logstd, input_norm


class ActorMLP:
    """actor(obs) -> actions [N, A].  Build with from_arrays or from_rl_games_checkpoint."""

    def __init__(self, weights, biases, logstd=None, activation="elu", input_norm=None, device="cuda:0", task=None, rng_seed=None,
                 env_index_base=None):
        if activation not in ACTIVATIONS:
            raise ValueError(f"ActorMLP: activation {activation!r}; supported: 'none', 'elu', 'relu'")
        self.activation = activation if activation is not None else "none"
        self.weights = [np.ascontiguousarray(np.asarray(w, np.float32)) for w in weights]
        self.biases = [np.ascontiguousarray(np.asarray(b, np.float32)) for b in biases]
        if len(self.weights) != len(self.biases) or not self.weights:
            raise ValueError(f"ActorMLP: {len(self.weights)} weights and {len(self.biases)} biases")
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.ndim != 2 or b.shape != (w.shape[0],):
                raise ValueError(f"ActorMLP: layer {l}: weight {w.shape} and bias {b.shape} are not [out, in] and [out]")
            if l and w.shape[1] != self.weights[l - 1].shape[0]:
                raise ValueError(f"ActorMLP: layer {l} reads {w.shape[1]} inputs, layer {l - 1} writes {self.weights[l - 1].shape[0]}")
        self.dims = [self.weights[0].shape[1]] + [w.shape[0] for w in self.weights]
        self.lds_bytes = check_dims(self.dims)
        self.obs_dim, self.action_dim = self.dims[0], self.dims[-1]
        self.logstd = None if logstd is None else np.ascontiguousarray(np.asarray(logstd, np.float32)).reshape(-1)
        if self.logstd is not None and self.logstd.shape != (self.action_dim,):
            raise ValueError(f"ActorMLP: logstd has {self.logstd.size} entries, the net has {self.action_dim} actions")
        self.input_norm = None
        if input_norm is not None:
            mean, denom, clip = input_norm
            mean = np.ascontiguousarray(np.asarray(mean, np.float32)).reshape(-1)
            denom = np.ascontiguousarray(np.asarray(denom, np.float32)).reshape(-1)
            if mean.shape != (self.obs_dim,) or denom.shape != (self.obs_dim,):
                raise ValueError(f"ActorMLP: input_norm of widths {mean.size} / {denom.size}, the net reads {self.obs_dim} inputs")
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
        if self._is_cpu:
            self._cpu = [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in zip(self.weights, self.biases)]
        else:
            self._lib = _lib.load()
            n = len(self.weights)
            wp = (C.c_void_p * n)(*[w.ctypes.data for w in self.weights])
            bp = (C.c_void_p * n)(*[b.ctypes.data for b in self.biases])
            handle = C.c_void_p()
            with torch.cuda.device(torch.device(self.device)):
                _lib.check(self._lib.agx_policy_create(n, (C.c_int32 * len(self.dims))(*self.dims), wp, bp, ACTIVATIONS[self.activation],
                                                       C.byref(handle)), "agx_policy_create")
                self._handle = handle
                if self.input_norm is not None:
                    mean, denom, clip = self.input_norm
                    _lib.check(self._lib.agx_policy_set_input_norm(handle, mean.ctypes.data, denom.ctypes.data, clip), "agx_policy_set_input_norm")
                if self.logstd is not None:
                    _lib.check(self._lib.agx_policy_set_logstd(handle, self.logstd.ctypes.data), "agx_policy_set_logstd")

    def __del__(self):
        handle, self._handle = getattr(self, "_handle", None), None
        if handle:
            self._lib.agx_policy_destroy(handle)

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
    def _buffers(self, n):
        bufs = self._out.get(n)
        if bufs is None:
            bufs = self._out[n] = (torch.empty((n, self.action_dim), dtype=torch.float32, device=self.device),
                                   torch.empty((n, self.action_dim), dtype=torch.float32, device=self.device))
        return bufs

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

    def __call__(self, obs, out=None, sample=False, clamp=False, eps=None, step=None):
        """obs [N, obs_dim] float32 -> actions [N, action_dim]; `actor.mean` then holds the mean of this call.  sample: a = mu +
        eps * exp(logstd), eps given ([N, action_dim]) or drawn by the library's generator at (rng_seed, env_index_base + env,
        step, action) -- step: the task's env step, or this object's own count of sampled calls.  clamp: to [-1, 1], last.
        Without out= the result lives in a buffer kept per batch size: the next call of that size overwrites it."""
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim or obs.dtype is not torch.float32:
            raise ValueError(f"ActorMLP: observations must be float32 [N, {self.obs_dim}], got {obs.dtype} {tuple(obs.shape)}")
        n = obs.shape[0]
        if sample and self.logstd is None:
            raise ValueError("ActorMLP: sample=True needs a logstd (the checkpoint's a2c_network.sigma)")
        if eps is not None and (tuple(eps.shape) != (n, self.action_dim) or eps.dtype is not torch.float32):
            raise ValueError(f"ActorMLP: eps must be float32 [{n}, {self.action_dim}]")
        buf, mean = self._buffers(n)
        if out is None:
            out = buf
        elif tuple(out.shape) != (n, self.action_dim) or out.dtype is not torch.float32:
            raise ValueError(f"ActorMLP: out must be float32 [{n}, {self.action_dim}]")
        env_step = self._env_step(step, sample and eps is None)
        if self._is_cpu:
            return self._call_cpu(obs, out, mean, sample, clamp, eps)
        if not obs.is_contiguous():
            obs = obs.contiguous()
        flags = (_lib.POLICY_SAMPLE if sample else 0) | (_lib.POLICY_CLAMP if clamp else 0)
        p = _lib.dptr
        _lib.check(self._lib.agx_policy_act(self._handle, n, p(obs), p(out), p(mean), p(eps) if sample else None, flags, self.rng_seed,
                                            self.env_index_base, env_step & 0x7FFFFFFF, _lib.current_stream(self.device)), "agx_policy_act")
        self.mean = mean
        return out

    def _call_cpu(self, obs, out, mean, sample, clamp, eps):
        x = obs
        if self.input_norm is not None:
            m, d, clip = self.input_norm
            x = torch.clamp((x - torch.from_numpy(m)) / torch.from_numpy(d), -clip, clip)
        last = len(self._cpu) - 1
        for l, (w, b) in enumerate(self._cpu):
            x = torch.nn.functional.linear(x, w, b)
            if l < last:
                if self.activation == "elu":
                    x = torch.nn.functional.elu(x)
                elif self.activation == "relu":
                    x = torch.relu(x)
        mean.copy_(x)
        if sample:
            if eps is None:
                raise ValueError("ActorMLP on a CPU device has no generator: pass eps= to sample")
            x = x + eps * torch.exp(torch.from_numpy(self.logstd))
        if clamp:
            x = x.clamp(-1.0, 1.0)
        out.copy_(x)
        self.mean = mean
        return out

    def noise(self, n, step):
        """[n, action_dim]: the normals a sampled call without eps draws at env step `step` (diagnostic)"""
        if self._is_cpu:
            raise RuntimeError("ActorMLP.noise: the generator lives in the HIP library; this actor is on a CPU device")
        out = torch.empty((n, self.action_dim), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.agx_policy_noise(self._handle, n, self.rng_seed, self.env_index_base, int(step) & 0x7FFFFFFF, _lib.dptr(out),
                                              _lib.current_stream(self.device)), "agx_policy_noise")
        return out
