"""VAEImageEncoder with the reference's surface (aerial_gym/utils/vae/vae_image_encoder.py): the depth image -> 64 latents
of the pre-trained VAE encoder (utils/vae/VAE.py ImgEncoder: nine convolutions, two dense layers) and the reparametrisation.

Everything on the device is the HIP library (csrc/agx_vae.hip: exact-fp32 matrix instructions, one fixed accumulation order per
layer); this module loads and checks the state dict, builds the nearest-neighbour index tables from torch itself, owns the
workspace the encoder runs its env chunks through and draws nothing: eps comes from the caller (`eps=`, the strict-RNG mode of
the tasks) or from the library's counter-based generator.  The decoder is not part of this package."""
import ctypes as C
import os

import numpy as np
import torch

from ... import _lib

LAYER_NAMES = ("conv0", "conv0_1", "conv1_0", "conv1_1", "conv0_jump_2", "conv2_0", "conv2_1", "conv1_jump_3", "conv3_0", "dense0",
               "dense1")  # the order of the library's per-layer arrays (AGX_VAE_LAYERS)
# Cin, Cout, kernel, stride, (pad_h, pad_w) of the convolutions; (in, out) of the dense layers
CONV_LAYERS = {
    "conv0": (1, 32, 5, 2, (2, 2)), "conv0_1": (32, 32, 3, 2, (2, 2)), "conv1_0": (32, 32, 5, 2, (1, 1)),
    "conv1_1": (32, 64, 3, 1, (1, 1)), "conv0_jump_2": (32, 64, 4, 2, (1, 1)), "conv2_0": (64, 64, 5, 2, (2, 2)),
    "conv2_1": (64, 128, 3, 2, (1, 1)), "conv1_jump_3": (64, 128, 5, 4, (2, 1)), "conv3_0": (128, 128, 5, 2, (0, 0)),
}
DENSE_LAYERS = {"dense0": (2304, 512), "dense1": (512, 128)}
LATENT_DIMS = 64
WEIGHTS_HINT = ("The trained weights are not shipped with this package: copy "
                "aerial_gym/utils/vae/weights/ICRA_test_set_more_sim_data_kld_beta_3_LD_64_epoch_49.pth of the upstream "
                "repository (ntnu-arl/aerial_gym_simulator) there, or point vae_config.model_folder / model_file at a state dict "
                "of the same architecture.")


def clean_state_dict(state_dict):
    """the key names a checkpoint of the reference may carry, brought to `encoder.<layer>.<kind>`: a DataParallel `module.` prefix
    dropped, the older `dronet.` name of the encoder mapped to `encoder.`"""
    return {key.replace("module.", "").replace("dronet.", "encoder."): value for key, value in state_dict.items()}


def expected_shapes():
    """{state-dict key: shape} of the 22 encoder tensors"""
    shapes = {}
    for name, (cin, cout, k, _s, _p) in CONV_LAYERS.items():
        shapes[f"encoder.{name}.weight"], shapes[f"encoder.{name}.bias"] = (cout, cin, k, k), (cout,)
    for name, (fin, fout) in DENSE_LAYERS.items():
        shapes[f"encoder.{name}.weight"], shapes[f"encoder.{name}.bias"] = (fout, fin), (fout,)
    return shapes


def select_encoder_tensors(state_dict):
    """the 22 `encoder.*` tensors of a (cleaned) state dict as contiguous float32 CPU tensors, in LAYER_NAMES order:
    (weights, biases).  `img_decoder.*` and anything else is ignored.  KeyError / ValueError name the offending key."""
    shapes = expected_shapes()
    weights, biases = [], []
    for name in LAYER_NAMES:
        for kind, dst in (("weight", weights), ("bias", biases)):
            key = f"encoder.{name}.{kind}"
            if key not in state_dict:
                raise KeyError(f"VAE state dict has no {key!r} (keys are cleaned like the reference: 'module.' stripped, 'dronet.' -> 'encoder.')")
            t = torch.as_tensor(state_dict[key])
            if tuple(t.shape) != shapes[key]:
                raise ValueError(f"VAE state dict: {key!r} has shape {tuple(t.shape)}, the encoder needs {shapes[key]}")
            dst.append(t.detach().to("cpu", torch.float32).contiguous())
    return weights, biases


def load_encoder_state(path):
    if not os.path.exists(path):
        raise FileNotFoundError(f"VAE weight file {path} does not exist. {WEIGHTS_HINT}")
    state = torch.load(path, map_location="cpu")
    if isinstance(state, dict) and "state_dict" in state and not any(str(k).startswith(("encoder.", "module.", "dronet.")) for k in state):
        state = state["state_dict"]
    return select_encoder_tensors(clean_state_dict(state))


def layer_geometry(image_res):
    """{layer name: (out_h, out_w)} for an image_res input; ValueError unless conv3_0 ends in 3 x 6 (what dense0 requires)"""
    lib = _lib.load()
    out = (C.c_int32 * (2 * _lib.VAE_LAYERS))()
    if lib.agx_vae_geometry(int(image_res[0]), int(image_res[1]), out) != 0:
        raise ValueError(lib.agx_last_error().decode("utf-8", "replace"))
    return {name: (out[2 * i], out[2 * i + 1]) for i, name in enumerate(LAYER_NAMES)}


def nearest_index_tables(src_hw, dst_hw):
    """(row_map [dst_h], col_map [dst_w]) int32: F.interpolate(x, dst_hw, mode="nearest")[..., r, c] == x[..., row_map[r], col_map[c]].
    Built from torch itself (an arange image through F.interpolate), so they are torch's rule by construction."""
    (sh, sw), (dh, dw) = src_hw, dst_hw
    rows = torch.arange(sh, dtype=torch.float32).view(1, 1, sh, 1).expand(1, 1, sh, sw)
    cols = torch.arange(sw, dtype=torch.float32).view(1, 1, 1, sw).expand(1, 1, sh, sw)
    row_map = torch.nn.functional.interpolate(rows, (dh, dw), mode="nearest")[0, 0, :, 0]
    col_map = torch.nn.functional.interpolate(cols, (dh, dw), mode="nearest")[0, 0, 0, :]
    return row_map.to(torch.int32).contiguous(), col_map.to(torch.int32).contiguous()


def pack_weight(w):
    """torch layout [Cout, ...] -> the kernels' [K8][Cout] (float32 numpy, host)"""
    w = np.ascontiguousarray(np.asarray(w, np.float32))
    cout, k = w.shape[0], int(np.prod(w.shape[1:]))
    lib = _lib.load()
    packed = np.empty(lib.agx_vae_packed_floats(cout, k), np.float32)
    _lib.check(lib.agx_vae_pack_weight(cout, k, w.ctypes.data, packed.ctypes.data), "agx_vae_pack_weight")
    return packed


def unpack_weight(packed, shape):
    shape = tuple(int(v) for v in shape)
    cout, k = shape[0], int(np.prod(shape[1:]))
    packed = np.ascontiguousarray(packed, np.float32)
    assert packed.size == _lib.load().agx_vae_packed_floats(cout, k), (packed.size, shape)
    w = np.empty(shape, np.float32)
    _lib.check(_lib.load().agx_vae_unpack_weight(cout, k, packed.ctypes.data, w.ctypes.data), "agx_vae_unpack_weight")
    return w


def _bf16_shape(shape):
    """the AgxVaeConv the bf16 pack reads: [Cout, Cin, kh, kw], a dense [out, in] as a 1 x 1 kernel"""
    shape = tuple(int(v) for v in shape)
    cout, cin, kh, kw = shape if len(shape) == 4 else (shape[0], shape[1], 1, 1)
    return _lib.AgxVaeConv(cin=cin, cout=cout, kh=kh, kw=kw)


def pack_weight_bf16(w):
    """torch layout [Cout, Cin, kh, kw] (or [out, in]) -> the bf16 kernels' [Cout][Kp], k = (kh, kw, ci), rounded to nearest even,
    Kp = K rounded up to 16 with a zero tail (uint16 numpy, host).  A dense layer that reads a flattened [H, W, C] activation
    is packed from its weight viewed as [out, C, H, W] (dense0: `w.reshape(512, 128, 3, 6)`)."""
    w = np.ascontiguousarray(np.asarray(w, np.float32))
    S, lib = _bf16_shape(w.shape), _lib.load()
    packed = np.empty(lib.agx_vae_packed_bf16_elems(C.byref(S)), np.uint16)
    _lib.check(lib.agx_vae_pack_weight_bf16(C.byref(S), w.ctypes.data, packed.ctypes.data), "agx_vae_pack_weight_bf16")
    return packed


def unpack_weight_bf16(packed, shape):
    """the rounded values of a pack_weight_bf16 result, float32 in torch's layout `shape`"""
    S, lib = _bf16_shape(shape), _lib.load()
    packed = np.ascontiguousarray(packed, np.uint16)
    assert packed.size == lib.agx_vae_packed_bf16_elems(C.byref(S)), (packed.size, shape)
    w = np.empty(tuple(int(v) for v in shape), np.float32)
    _lib.check(lib.agx_vae_unpack_weight_bf16(C.byref(S), packed.ctypes.data, w.ctypes.data), "agx_vae_unpack_weight_bf16")
    return w


PRECISIONS = {"fp32": _lib.VAE_FP32, "bf16": _lib.VAE_BF16}


class VAEImageEncoder(torch.nn.Module):
    DEFAULT_WORKSPACE_MB = 1024

    def __init__(self, config, device="cuda:0", workspace_mb=None, rng_seed=0):
        super().__init__()
        self.config = config
        self.device = device
        self.precision = getattr(config, "precision", "fp32")
        if self.precision not in PRECISIONS:
            raise ValueError(f"vae_config.precision = {self.precision!r}: this encoder runs in 'fp32' or 'bf16'")
        if int(config.latent_dims) != LATENT_DIMS:
            raise ValueError(f"vae_config.latent_dims = {config.latent_dims}: this encoder has {LATENT_DIMS} latents")
        self.image_res = (int(config.image_res[0]), int(config.image_res[1]))
        self.geometry = layer_geometry(self.image_res)  # ValueError for an image_res that does not end in 3 x 6
        path = os.path.join(config.model_folder, config.model_file)
        weights, biases = load_encoder_state(path)
        self._lib = _lib.load()
        wp = (C.c_void_p * _lib.VAE_LAYERS)(*[w.data_ptr() for w in weights])
        bp = (C.c_void_p * _lib.VAE_LAYERS)(*[b.data_ptr() for b in biases])
        handle = C.c_void_p()
        with torch.cuda.device(torch.device(device)):
            _lib.check(self._lib.agx_vae_create_precision(wp, bp, self.image_res[0], self.image_res[1], LATENT_DIMS,
                                                          PRECISIONS[self.precision], C.byref(handle)), "agx_vae_create_precision")
        self._handle = handle
        self.workspace_bytes_budget = int(workspace_mb if workspace_mb is not None else self.DEFAULT_WORKSPACE_MB) << 20
        self.rng_seed, self.env_index_base, self.env_step = int(rng_seed), 0, 0
        self._workspace = None
        self._tables = {}
        self._resized = None

    def __del__(self):
        handle, self._handle = getattr(self, "_handle", None), None
        if handle:
            self._lib.agx_vae_destroy(handle)

    # ---- chunking ------------------------------------------------------------------------------------------------------
    def bytes_per_env(self):
        return int(self._lib.agx_vae_workspace_bytes(self._handle, 1))

    def envs_per_chunk(self, num_envs):
        """what agx_vae_encode derives from the workspace budget; at least 1 (a budget below one env is raised to one env)"""
        return max(1, int(self._lib.agx_vae_envs_per_chunk(self._handle, self.workspace_bytes_budget, int(num_envs))))

    def _workspace_for(self, num_envs):
        """(workspace, the bytes of it that hold exactly envs_per_chunk(num_envs) envs)"""
        need = int(self._lib.agx_vae_workspace_bytes(self._handle, self.envs_per_chunk(num_envs)))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace, need

    # ---- resizing ------------------------------------------------------------------------------------------------------
    def _source(self, images):
        """(pixels [N, h, w], row_map, col_map): what the first convolution reads"""
        n, h, w = images.shape
        if (h, w) == self.image_res:
            return images, None, None
        if self.config.interpolation_mode == "nearest":
            if (h, w) not in self._tables:
                rm, cm = nearest_index_tables((h, w), self.image_res)
                self._tables[(h, w)] = (rm.to(self.device), cm.to(self.device))
            return (images,) + self._tables[(h, w)]
        if self._resized is None or self._resized.shape[0] != n:
            self._resized = torch.empty((n, 1) + self.image_res, device=self.device)
        self._resized.copy_(torch.nn.functional.interpolate(images.unsqueeze(1), self.image_res, mode=self.config.interpolation_mode))
        return self._resized.view(n, *self.image_res), None, None

    # ---- the reference's surface ---------------------------------------------------------------------------------------
    def encode_all(self, image_tensors, eps=None, out=None):
        """(z_sampled, means, std), each [N, 64].  eps [N, 64]: the normals of the reparametrisation (None: the library's
        generator at (rng_seed, env_index_base + env, env_step)).  out: the tensor z_sampled is written to.  The results are
        fresh [N, 64] tensors per call, like the reference's (callers keep them): three small allocations from torch's caching
        allocator on the host side, none inside the library.  Not capturable into a hipGraph: env_step is a launch argument."""
        x = image_tensors
        if x.dim() == 4:
            if x.shape[1] != 1:
                raise ValueError(f"VAEImageEncoder.encode: one image per env ([N, H, W] or [N, 1, H, W]), got {tuple(x.shape)}")
            x = x[:, 0]
        if x.dim() != 3:
            raise ValueError(f"VAEImageEncoder.encode: [N, H, W] or [N, 1, H, W], got {tuple(image_tensors.shape)}")
        if x.dtype is not torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        n = x.shape[0]
        pixels, row_map, col_map = self._source(x)
        latents = out if out is not None else torch.empty((n, LATENT_DIMS), device=self.device)
        means, std = torch.empty((n, LATENT_DIMS), device=self.device), torch.empty((n, LATENT_DIMS), device=self.device)
        if eps is not None and (tuple(eps.shape) != (n, LATENT_DIMS) or eps.dtype is not torch.float32):
            raise ValueError(f"eps must be float32 [{n}, {LATENT_DIMS}]")
        ws, ws_bytes = self._workspace_for(n)
        p = _lib.dptr
        _lib.check(self._lib.agx_vae_encode(self._handle, n, p(pixels), pixels.shape[1], pixels.shape[2], p(row_map), p(col_map), p(eps),
                                            p(latents), p(means), p(std), p(ws), ws_bytes, self.rng_seed, int(self.env_index_base),
                                            int(self.env_step), _lib.current_stream(self.device)), "agx_vae_encode")
        return latents, means, std

    def encode(self, image_tensors, eps=None):
        z_sampled, means, _std = self.encode_all(image_tensors, eps=eps)
        return z_sampled if self.config.return_sampled_latent else means

    def forward(self, image_tensors):
        return self.encode(image_tensors)

    def decode(self, latent_spaces):
        raise NotImplementedError("the VAE decoder is not part of this package (the reference uses it in commented-out debugging code only)")

    def get_latent_dims_size(self):
        return self.config.latent_dims
