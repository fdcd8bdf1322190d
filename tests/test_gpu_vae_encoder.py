"""GPU: the VAE depth-image encoder (csrc/agx_vae.hip) layer by layer and as a whole against tests/vae_ref.py (float64 on the CPU).

Exact-arithmetic inputs (activations multiples of 1/16, weights and biases multiples of 1/8, all in [-1, 1]: every product and
partial sum is representable, K <= 3200 needs 19 bits) make every summation order give the same floats, so the kernels must equal
float64 BIT FOR BIT: that pins the matrix instruction's lane maps, padding, the asymmetric pad, strides and tile edges.  Random
inputs are held to the order-independent bound |err| <= (K + 2) 2^-24 (|w| (*) |x| + |b|) (vae_ref.bound).  Whole encoder:
agx_vae_encode == the chain of single-layer calls, invariance to chunking and env position, the sampling epilogue and its device
generator."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import vae_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONV_NAMES = list(vae_ref.CONVS)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _lib():
    from aerial_gym_simulator_amd import _lib as L

    return L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _packed(w):
    from aerial_gym_simulator_amd.utils.vae.vae_image_encoder import pack_weight

    return torch.from_numpy(pack_weight(w.numpy())).to(DEV)


def hip_conv(name, x, w, b, add=None, elu=False, maps=None):
    """one agx_vae_conv2d call: x [B, Cin, h, w] float32 CPU (the SOURCE image when maps = (row_map, col_map) is given)"""
    L = _lib()
    cin, cout, k, s, (ph, pw) = vae_ref.CONVS[name]
    B, _, sh, sw = x.shape
    ih, iw = (len(maps[0]), len(maps[1])) if maps else (sh, sw)
    oh, ow = vae_ref.out_hw(name, ih, iw)
    S = L.AgxVaeConv(cin=cin, cout=cout, kh=k, kw=k, stride=s, pad_h=ph, pad_w=pw, in_h=ih, in_w=iw, out_h=oh, out_w=ow, src_h=sh, src_w=sw)
    xd, wd, bd = x.contiguous().to(DEV), _packed(w), b.to(DEV)
    ad = add.contiguous().to(DEV) if add is not None else None
    md = [m.to(torch.int32).to(DEV) for m in maps] if maps else [None, None]
    y = torch.full((B, cout, oh, ow), float("nan"), device=DEV)
    L.check(L.load().agx_vae_conv2d(B, L.dptr(xd), L.dptr(wd), L.dptr(bd), L.dptr(ad), L.dptr(y), C.byref(S), L.VAE_ELU if elu else 0,
                                    L.dptr(md[0]), L.dptr(md[1]), _stream()), "agx_vae_conv2d")
    torch.cuda.synchronize()
    return y.cpu()


def hip_linear(x, w, b, elu=False):
    L = _lib()
    xd, wd, bd = x.contiguous().to(DEV), _packed(w), b.to(DEV)
    y = torch.full((x.shape[0], w.shape[0]), float("nan"), device=DEV)
    L.check(L.load().agx_vae_linear(x.shape[0], L.dptr(xd), L.dptr(wd), L.dptr(bd), L.dptr(y), w.shape[1], w.shape[0], L.VAE_ELU if elu else 0,
                                    _stream()), "agx_vae_linear")
    torch.cuda.synchronize()
    return y.cpu()


def _same_bits(got, ref64):
    ref = ref64.to(torch.float32)  # (exact but for ELU's expm1, which is rounded once)
    return np.array_equal(got.numpy().view(np.uint32), ref.numpy().view(np.uint32))


EPILOGUES = [(False, False), (True, False), (False, True), (True, True)]  # (second tensor, ELU)


@pytest.mark.parametrize("size", [(13, 17), (37, 70)])
@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_layers_exact_inputs_bit_for_bit(name, size):
    cin, cout, k, _s, _p = vae_ref.CONVS[name]
    g = _gen(100 + CONV_NAMES.index(name))
    w, b = vae_ref.exact_grid((cout, cin, k, k), 1 / 8, g), vae_ref.exact_grid((cout,), 1 / 8, g)
    oh, ow = vae_ref.out_hw(name, *size)
    for batch in (1, 3):
        x = vae_ref.exact_grid((batch, cin) + size, 1 / 16, g)
        add = vae_ref.exact_grid((batch, cout, oh, ow), 1 / 16, g)
        for with_add, elu in EPILOGUES:
            ref, _mag, pre = vae_ref.layer64(name, x, w, b, add if with_add else None, elu)
            assert torch.equal(pre.float().double(), pre)  # the premise: the exact result is a float32
            got = hip_conv(name, x, w, b, add if with_add else None, elu)
            assert got.shape == ref.shape and _same_bits(got, ref), (name, size, batch, with_add, elu, float((got.double() - ref).abs().max()))


@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_layers_random_inputs_within_the_order_independent_bound(name):
    cin, cout, k, _s, _p = vae_ref.CONVS[name]
    g = _gen(200 + CONV_NAMES.index(name))
    scale = 1 / np.sqrt(vae_ref.fan_in(name))
    w, b = (torch.rand((cout, cin, k, k), generator=g) * 2 - 1) * scale, (torch.rand(cout, generator=g) * 2 - 1) * scale
    worst = 0.0
    for batch, size in ((1, (13, 17)), (3, (37, 70))):
        x = torch.rand((batch, cin) + size, generator=g) * 2 - 1
        add = torch.rand((batch, cout) + vae_ref.out_hw(name, *size), generator=g) * 2 - 1
        for with_add, elu in ((False, False), (True, True)):
            ref, mag, _pre = vae_ref.layer64(name, x, w, b, add if with_add else None, elu)
            got = hip_conv(name, x, w, b, add if with_add else None, elu)
            ratio = float(((got.double() - ref).abs() / vae_ref.bound(name, mag, ref, elu)).max())
            worst = max(worst, ratio)
    print(f"{name}: max |err| / bound = {worst:.3f}")
    assert worst <= 1.0, (name, worst)


def test_conv0_through_index_tables_equals_resize_then_convolution():
    from aerial_gym_simulator_amd.utils.vae.vae_image_encoder import nearest_index_tables

    g = _gen(300)
    w, b = vae_ref.exact_grid((32, 1, 5, 5), 1 / 8, g), vae_ref.exact_grid((32,), 1 / 8, g)
    for src, dst in (((9, 11), (37, 70)), ((48, 64), (61, 50))):  # up-sampling, and a mix of up and down
        x = vae_ref.exact_grid((3, 1) + src, 1 / 16, g)
        rm, cm = nearest_index_tables(src, dst)
        assert not torch.equal(rm, torch.arange(dst[0], dtype=torch.int32))
        ref, _mag, _pre = vae_ref.layer64("conv0", torch.nn.functional.interpolate(x, dst, mode="nearest"), w, b)
        got = hip_conv("conv0", x, w, b, maps=(rm, cm))
        assert got.shape == ref.shape and _same_bits(got, ref), (src, dst)


@pytest.mark.parametrize("batch", [1, 5, 64, 65])
@pytest.mark.parametrize("name", ["dense0", "dense1"])
def test_dense_layers(name, batch):
    fin, fout = vae_ref.DENSE[name]
    elu = name == "dense0"
    g = _gen(400 + batch)
    w, b, x = vae_ref.exact_grid((fout, fin), 1 / 8, g), vae_ref.exact_grid((fout,), 1 / 8, g), vae_ref.exact_grid((batch, fin), 1 / 16, g)
    ref, _mag, _pre = vae_ref.layer64(name, x, w, b, None, elu)
    assert _same_bits(hip_linear(x, w, b, elu), ref), (name, batch, "exact inputs")
    scale = 1 / np.sqrt(fin)
    w, b, x = (torch.rand((fout, fin), generator=g) * 2 - 1) * scale, (torch.rand(fout, generator=g) * 2 - 1) * scale, torch.rand((batch, fin), generator=g) * 2 - 1
    ref, mag, _pre = vae_ref.layer64(name, x, w, b, None, elu)
    ratio = float(((hip_linear(x, w, b, elu).double() - ref).abs() / vae_ref.bound(name, mag, ref, elu)).max())
    print(f"{name} batch {batch}: max |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_expm1_cw_is_correctly_rounded():
    """in the manner of test_gpu_math.py: float64 expm1 rounded once, over a dense sweep of negative arguments, the interval
    around 0 and the saturation to -1"""
    L = _lib()
    rng = np.random.default_rng(21)
    n = 400_000
    x = np.concatenate([-rng.uniform(0, 20, n), -np.logspace(-40, 1.3, n // 4), rng.uniform(-1e-3, 1e-3, n // 4), rng.uniform(-0.7, 0.7, n // 4),
                        rng.uniform(0, 5, n // 8), -rng.uniform(16, 120, n // 8), np.linspace(-0.3466, -0.3465, 2001),
                        [0.0, -0.0, -1e-45, 1e-45, -1e-8, -17.0, -17.33, -18.0, -87.4, -103.9, -104.1, -1e4, -3e38, 1.0, 88.0]]).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    out = torch.empty_like(xd)
    L.check(L.load().agx_math_eval(L.MATH_EXPM1, xd.numel(), L.dptr(xd), L.dptr(xd), L.dptr(out), _stream()), "agx_math_eval")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    exact = np.expm1(x.astype(np.float64))
    assert np.mean(got == exact.astype(np.float32)) > 0.99999
    ulp = np.maximum(np.spacing(np.abs(exact.astype(np.float32))).astype(np.float64), np.spacing(np.float32(1e-30)))
    assert (np.abs(got.astype(np.float64) - exact) / ulp).max() <= 0.5 + 1e-5
    assert np.all(got[x < -18] == -1.0) and np.all(got[x < 0] >= -1.0) and np.all(got[x < 0] < 0)
    tiny = np.abs(x) < 1e-10
    assert np.array_equal(got[tiny].view(np.uint32), x[tiny].view(np.uint32))  # expm1(x) = x there, signed zeros included


# ---------------------------------------------------------------------------------------------------- the whole encoder
def _vae_cfg(folder, **kw):
    d = dict(use_vae=True, latent_dims=64, model_file="w.pth", model_folder=str(folder), image_res=(270, 480), interpolation_mode="nearest",
             return_sampled_latent=True)
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.fixture(scope="module")
def enc_and_weights(tmp_path_factory):
    from aerial_gym_simulator_amd.utils.vae.vae_image_encoder import VAEImageEncoder

    folder = tmp_path_factory.mktemp("vae")
    sd = vae_ref.random_state_dict(_gen(7), prefix="module.dronet.", scale=1.7)  # (1.7: keeps the activations from shrinking layer by layer)
    sd["module.img_decoder.dense.weight"] = torch.zeros(4, 4)
    torch.save(sd, str(folder / "w.pth"))
    enc = VAEImageEncoder(_vae_cfg(folder), device=DEV, rng_seed=0xABCDEF0123)
    clean = {k.replace("module.dronet.", "encoder."): v for k, v in sd.items()}
    return enc, clean


def _images(n, hw, seed):
    return torch.rand((n,) + hw, generator=_gen(seed)) * 10.0  # depth-like, metres


def _encode_raw(enc, px, eps=None, workspace_bytes=None, env_base=0, step=0):
    """agx_vae_encode on device pixels [n, h, w] -> (latents, means, std) CPU; workspace_bytes forces the chunk size"""
    L = _lib()
    n, h, w = px.shape
    pixels, rm, cm = enc._source(px)
    ws_bytes = workspace_bytes or int(enc._lib.agx_vae_workspace_bytes(enc._handle, n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    lat, mean, std = (torch.full((n, 64), float("nan"), device=DEV) for _ in range(3))
    L.check(enc._lib.agx_vae_encode(enc._handle, n, L.dptr(pixels), h, w, L.dptr(rm), L.dptr(cm), L.dptr(eps), L.dptr(lat), L.dptr(mean),
                                    L.dptr(std), L.dptr(ws), ws_bytes, enc.rng_seed, env_base, step, _stream()), "agx_vae_encode")
    torch.cuda.synchronize()
    return lat.cpu(), mean.cpu(), std.cpu()


def _chain(sd, images, maps):
    """the encoder as single-layer calls: {layer: (output, its HIP input(s))}"""
    g = lambda n: (sd[f"encoder.{n}.weight"], sd[f"encoder.{n}.bias"])  # noqa: E731
    o = {}
    o["conv0"] = hip_conv("conv0", images, *g("conv0"), maps=maps)
    o["conv0_1"] = hip_conv("conv0_1", o["conv0"], *g("conv0_1"), elu=True)
    o["conv1_0"] = hip_conv("conv1_0", o["conv0_1"], *g("conv1_0"))
    o["conv0_jump_2"] = hip_conv("conv0_jump_2", o["conv0_1"], *g("conv0_jump_2"))
    o["conv1_1"] = hip_conv("conv1_1", o["conv1_0"], *g("conv1_1"), add=o["conv0_jump_2"], elu=True)
    o["conv2_0"] = hip_conv("conv2_0", o["conv1_1"], *g("conv2_0"))
    o["conv1_jump_3"] = hip_conv("conv1_jump_3", o["conv1_1"], *g("conv1_jump_3"))
    o["conv2_1"] = hip_conv("conv2_1", o["conv2_0"], *g("conv2_1"), add=o["conv1_jump_3"], elu=True)
    o["conv3_0"] = hip_conv("conv3_0", o["conv2_1"], *g("conv3_0"))
    o["dense0"] = hip_linear(o["conv3_0"].flatten(1), *g("dense0"), elu=True)
    o["dense1"] = hip_linear(o["dense0"], *g("dense1"))
    return o


CHAIN_INPUT = {"conv0_1": "conv0", "conv1_0": "conv0_1", "conv0_jump_2": "conv0_1", "conv1_1": "conv1_0", "conv2_0": "conv1_1",
               "conv1_jump_3": "conv1_1", "conv2_1": "conv2_0", "conv3_0": "conv2_1", "dense0": "conv3_0", "dense1": "dense0"}
CHAIN_ADD = {"conv1_1": "conv0_jump_2", "conv2_1": "conv1_jump_3"}
CHAIN_ELU = ("conv0_1", "conv1_1", "conv2_1", "dense0")


@pytest.mark.parametrize("setup", ["native_n1", "native_n3", "from_48x64_n3"])
def test_encoder_equals_the_layer_chain_and_every_layer_meets_the_bound(enc_and_weights, setup):
    """(a) agx_vae_encode == the chain of single-layer calls bit for bit, (b) each layer of the chain within the bound of float64
    applied to its own HIP input, (d, first half) the sampling epilogue == its numpy float32 restatement, (e) printed"""
    from aerial_gym_simulator_amd.utils.vae.vae_image_encoder import nearest_index_tables

    enc, sd = enc_and_weights
    n = 1 if setup == "native_n1" else 3
    hw = (48, 64) if setup.startswith("from") else (270, 480)
    images = _images(n, hw, 31)
    maps = nearest_index_tables(hw, (270, 480)) if hw != (270, 480) else None
    eps = torch.randn((n, 64), generator=_gen(32))
    lat, mean, std = _encode_raw(enc, images.to(DEV), eps=eps.to(DEV))
    o = _chain(sd, images.unsqueeze(1), maps)
    z = o["dense1"]
    want_lat, want_mean, want_std = vae_ref.sample_f32(z.numpy(), eps.numpy())
    for got, want, what in ((lat, want_lat, "latents"), (mean, want_mean, "means"), (std, want_std, "std")):
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), (setup, what)
    # (b)
    resized = torch.nn.functional.interpolate(images.unsqueeze(1), (270, 480), mode="nearest") if maps else images.unsqueeze(1)
    for name in vae_ref.ORDER:
        x = resized if name == "conv0" else o[CHAIN_INPUT[name]]
        if name == "dense0":
            x = x.flatten(1)
        add = o[CHAIN_ADD[name]] if name in CHAIN_ADD else None
        elu = name in CHAIN_ELU
        ref, mag, _pre = vae_ref.layer64(name, x, sd[f"encoder.{name}.weight"], sd[f"encoder.{name}.bias"], add, elu)
        ratio = float(((o[name].double() - ref).abs() / vae_ref.bound(name, mag, ref, elu)).max())
        assert ratio <= 1.0, (setup, name, ratio)
    # (e) informational: the final 128 outputs against float64 end to end, next to torch's own fp32 on the same inputs
    ref = vae_ref.encoder64(sd, resized)["dense1"]
    sd32 = {k: v.float() for k, v in sd.items()}
    t32 = _torch_fp32(sd32, resized)
    print(f"{setup}: max |HIP - float64| of the 128 outputs = {float((z.double() - ref).abs().max()):.3e}; torch fp32 (CPU): "
          f"{float((t32.double() - ref).abs().max()):.3e}; max |output| = {float(ref.abs().max()):.3f}")


def _torch_fp32(sd, images):
    F = torch.nn.functional
    c = lambda n, x: F.conv2d(x, sd[f"encoder.{n}.weight"], sd[f"encoder.{n}.bias"], stride=vae_ref.CONVS[n][3], padding=vae_ref.CONVS[n][4])  # noqa: E731
    x01 = F.elu(c("conv0_1", c("conv0", images.float())))
    x11 = F.elu(c("conv1_1", c("conv1_0", x01)) + c("conv0_jump_2", x01))
    x21 = F.elu(c("conv2_1", c("conv2_0", x11)) + c("conv1_jump_3", x11))
    d0 = F.elu(F.linear(c("conv3_0", x21).flatten(1), sd["encoder.dense0.weight"], sd["encoder.dense0.bias"]))
    return F.linear(d0, sd["encoder.dense1.weight"], sd["encoder.dense1.bias"])


def test_encoder_is_invariant_to_chunking_and_env_position(enc_and_weights):
    """(c) N = 5 with a workspace that forces chunks of 2 == one chunk == each image encoded alone at env position 0, bit for bit"""
    enc, _sd = enc_and_weights
    px = _images(5, (270, 480), 41).to(DEV)
    eps = torch.randn((5, 64), generator=_gen(42)).to(DEV)
    size = lambda n: int(enc._lib.agx_vae_workspace_bytes(enc._handle, n))  # noqa: E731
    chunk = lambda ws: int(enc._lib.agx_vae_envs_per_chunk(enc._handle, ws, 5))  # noqa: E731  (what agx_vae_encode derives for 5 envs)
    one, two, five = size(1), size(2), size(5)
    # the chunk each workspace really forces: the size is linear in the chunk, so size(n) holds n envs and not one byte fewer does
    assert (two, five) == (2 * one, 5 * one) and one % 256 == 0
    assert [chunk(ws) for ws in (one - 1, one, two - 1, two, size(3) - 1, five - 1, five, 2 * five)] == [0, 1, 1, 2, 2, 4, 5, 5]
    chunked = _encode_raw(enc, px, eps=eps, workspace_bytes=two)  # 2 + 2 + 1
    whole = _encode_raw(enc, px, eps=eps, workspace_bytes=five)  # one chunk of 5
    for a, b in zip(chunked, whole):
        assert np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))
    for i in range(5):
        alone = _encode_raw(enc, px[i:i + 1].contiguous(), eps=eps[i:i + 1].contiguous())
        for a, b in zip(alone, whole):
            assert np.array_equal(a.numpy().view(np.uint32), b[i:i + 1].numpy().view(np.uint32)), i
    assert all(torch.isfinite(t).all() for t in whole)


def _noise(enc, n, base, step):
    L = _lib()
    out = torch.empty((n, 64), device=DEV)
    L.check(enc._lib.agx_vae_noise(n, enc.rng_seed, base, step, L.dptr(out), _stream()), "agx_vae_noise")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_sampling_from_the_device_generator(enc_and_weights):
    """(d, second half) eps = NULL: latents == means + agx_vae_noise * std, each operation rounded; the noise is a function of
    (seed, global env index, step) alone"""
    enc, _sd = enc_and_weights
    px = _images(3, (48, 64), 51).to(DEV)
    two = int(enc._lib.agx_vae_workspace_bytes(enc._handle, 2))
    assert int(enc._lib.agx_vae_envs_per_chunk(enc._handle, two, 3)) == 2  # chunks of 2 + 1: the second starts at env 12
    lat, mean, std = _encode_raw(enc, px, eps=None, workspace_bytes=two, env_base=10, step=7)
    z = _noise(enc, 3, 10, 7)
    want = (mean.numpy() + (z * std.numpy()).astype(np.float32)).astype(np.float32)
    assert np.array_equal(lat.numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(_noise(enc, 9, 8, 7)[2:5], z) and np.array_equal(_noise(enc, 1, 11, 7)[0], z[1])
    assert not np.array_equal(_noise(enc, 3, 10, 8), z) and not np.array_equal(_noise(enc, 3, 11, 7), z)
    big = _noise(enc, 4096, 0, 3)
    assert abs(float(big.mean())) < 0.01 and abs(float(big.std()) - 1.0) < 0.01 and np.isfinite(big).all()
    assert len(np.unique(big)) > 0.99 * big.size


def test_encoder_class_surface(enc_and_weights):
    enc, _sd = enc_and_weights
    px = _images(2, (48, 64), 61).to(DEV)
    a = enc.encode(px)
    b = enc.forward(px.unsqueeze(1))
    assert a.shape == (2, 64) and torch.equal(a, b) and enc.get_latent_dims_size() == 64
    z, means, std = enc.encode_all(px)
    enc.config.return_sampled_latent = False
    try:
        assert torch.equal(enc.encode(px), means) and not torch.equal(means, z)
    finally:
        enc.config.return_sampled_latent = True
    with pytest.raises(NotImplementedError):
        enc.decode(a)
    assert enc.envs_per_chunk(1024) == (1024 << 20) // enc.bytes_per_env() == 157 and enc.envs_per_chunk(8) == 8
    ws, ws_bytes = enc._workspace_for(8)
    assert ws_bytes == 8 * enc.bytes_per_env() <= ws.numel()  # a batch inside the budget is one chunk
    # the workspace layout: eleven 256-byte aligned buffers, one per layer, that grow with the chunk
    offsets = []
    for layer in range(11):
        w, b, off = C.c_void_p(), C.c_void_p(), C.c_size_t()
        _lib().check(enc._lib.agx_vae_layer_info(enc._handle, layer, 3, C.byref(w), C.byref(b), C.byref(off)), "agx_vae_layer_info")
        assert w.value and b.value and off.value % 256 == 0
        offsets.append(off.value)
    floats = [co * h * w for (co, (h, w)) in ((vae_ref.weight_shape(n)[0], vae_ref.GEOMETRY_270x480[n]) for n in vae_ref.ORDER)]
    assert offsets[0] == 0 and all(b - a >= 3 * 4 * f for a, b, f in zip(offsets, offsets[1:], floats))
    assert int(enc._lib.agx_vae_workspace_bytes(enc._handle, 3)) >= offsets[-1] + 3 * 4 * 128
    # another interpolation mode: F.interpolate into a buffer, identity tables
    enc.config.interpolation_mode = "bilinear"
    try:
        eps = torch.zeros((2, 64), device=DEV)
        got = enc.encode_all(px, eps=eps)[1]
        resized = torch.nn.functional.interpolate(px.unsqueeze(1), (270, 480), mode="bilinear")
        want = _encode_raw(enc, resized[:, 0].contiguous(), eps=eps)[1]
        assert torch.equal(got.cpu(), want)
    finally:
        enc.config.interpolation_mode = "nearest"
