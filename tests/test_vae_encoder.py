"""CPU: the host side of the VAE depth-image encoder (aerial_gym_simulator_amd/utils/vae/vae_image_encoder.py and the host
functions of csrc/agx_vae.hip): state-dict cleaning and selection with their errors, the derived layer geometry, the nearest index
tables against torch's own resize, the weight repack, the alias import path, the config."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import vae_ref

from aerial_gym_simulator_amd.utils.vae import vae_image_encoder as vie


def _gen(seed=5):
    return torch.Generator().manual_seed(seed)


def test_state_dict_cleaning_and_selection():
    sd = vae_ref.random_state_dict(_gen(), prefix="module.dronet.")
    sd["module.img_decoder.dense.weight"] = torch.zeros(3, 3)
    sd["module.img_decoder.dense.bias"] = torch.zeros(3)
    clean = vie.clean_state_dict(sd)
    assert "encoder.conv0.weight" in clean and "img_decoder.dense.weight" in clean and not any("module." in k or "dronet." in k for k in clean)
    weights, biases = vie.select_encoder_tensors(clean)
    assert len(weights) == len(biases) == 11
    for name, w, b in zip(vie.LAYER_NAMES, weights, biases):
        assert tuple(w.shape) == vae_ref.weight_shape(name) and tuple(b.shape) == (vae_ref.weight_shape(name)[0],)
        assert torch.equal(w, sd[f"module.dronet.{name}.weight"]) and torch.equal(b, sd[f"module.dronet.{name}.bias"])
        assert w.is_contiguous() and w.dtype is torch.float32
    assert vie.LAYER_NAMES == vae_ref.ORDER


def test_missing_and_misshapen_keys_are_named():
    sd = vae_ref.random_state_dict(_gen())
    bad = dict(sd)
    del bad["encoder.conv1_jump_3.bias"]
    with pytest.raises(KeyError, match="encoder.conv1_jump_3.bias"):
        vie.select_encoder_tensors(bad)
    bad = dict(sd)
    bad["encoder.dense0.weight"] = torch.zeros(512, 2303)
    with pytest.raises(ValueError, match="encoder.dense0.weight"):
        vie.select_encoder_tensors(bad)


def test_missing_weight_file_says_where_it_lives(tmp_path):
    with pytest.raises(FileNotFoundError, match="aerial_gym/utils/vae/weights"):
        vie.load_encoder_state(str(tmp_path / "nothing.pth"))


def test_weight_file_round_trip(tmp_path):
    sd = vae_ref.random_state_dict(_gen(), prefix="module.dronet.")
    sd["module.img_decoder.x.weight"] = torch.zeros(2)
    path = str(tmp_path / "w.pth")
    torch.save(sd, path)
    weights, biases = vie.load_encoder_state(path)
    assert all(torch.equal(w, sd[f"module.dronet.{n}.weight"]) for n, w in zip(vie.LAYER_NAMES, weights))
    assert all(torch.equal(b, sd[f"module.dronet.{n}.bias"]) for n, b in zip(vie.LAYER_NAMES, biases))


def test_layer_geometry_of_the_reference_resolution():
    assert vie.layer_geometry((270, 480)) == vae_ref.GEOMETRY_270x480
    h, w = 270, 480  # the same from the layer table
    for name, src in (("conv0", None), ("conv0_1", "conv0"), ("conv1_0", "conv0_1"), ("conv1_1", "conv1_0"), ("conv0_jump_2", "conv0_1"),
                      ("conv2_0", "conv1_1"), ("conv2_1", "conv2_0"), ("conv1_jump_3", "conv1_1"), ("conv3_0", "conv2_1")):
        ih, iw = (h, w) if src is None else vae_ref.GEOMETRY_270x480[src]
        assert vae_ref.out_hw(name, ih, iw) == vae_ref.GEOMETRY_270x480[name], name
    assert vie.CONV_LAYERS == vae_ref.CONVS and vie.DENSE_LAYERS == vae_ref.DENSE


@pytest.mark.parametrize("res", [(240, 480), (270, 320), (64, 48), (4, 4), (540, 960)])
def test_image_res_that_does_not_end_in_3x6_is_refused(res):
    with pytest.raises(ValueError, match="3 x 6"):
        vie.layer_geometry(res)


def test_create_validates_before_it_touches_the_device():
    from aerial_gym_simulator_amd import _lib

    lib = _lib.load()
    sd = vae_ref.random_state_dict(_gen())
    weights, biases = vie.select_encoder_tensors(sd)
    wp = (C.c_void_p * 11)(*[w.data_ptr() for w in weights])
    bp = (C.c_void_p * 11)(*[b.data_ptr() for b in biases])
    handle = C.c_void_p()
    assert lib.agx_vae_create(wp, bp, 270, 480, 32, C.byref(handle)) == -1 and b"latent_dims" in lib.agx_last_error()
    assert lib.agx_vae_create(wp, bp, 64, 48, 64, C.byref(handle)) == -1 and b"3 x 6" in lib.agx_last_error()
    assert not handle.value


@pytest.mark.parametrize("src", [(48, 64), (270, 480), (135, 240), (300, 500)])
def test_nearest_index_tables_are_torchs_resize(src):
    dst = (270, 480)
    rm, cm = vie.nearest_index_tables(src, dst)
    assert rm.dtype is torch.int32 and tuple(rm.shape) == (270,) and tuple(cm.shape) == (480,)
    x = torch.rand((2, 1) + src, generator=_gen(9))
    want = torch.nn.functional.interpolate(x, dst, mode="nearest")
    assert torch.equal(x[:, :, rm.long()][:, :, :, cm.long()], want)
    if src == dst:
        assert torch.equal(rm, torch.arange(270, dtype=torch.int32)) and torch.equal(cm, torch.arange(480, dtype=torch.int32))


@pytest.mark.parametrize("name", list(vae_ref.ORDER))
def test_weight_repack_round_trips(name):
    shape = vae_ref.weight_shape(name)
    w = torch.rand(shape, generator=_gen(3)).numpy()
    packed = vie.pack_weight(w)
    k = vae_ref.fan_in(name)
    k8 = (k + 7) // 8 * 8
    assert packed.shape == (k8 * shape[0],)
    p2 = packed.reshape(k8, shape[0])
    assert np.array_equal(p2[:k], w.reshape(shape[0], k).T) and not p2[k:].any()  # k-major, the tail zero
    assert np.array_equal(vie.unpack_weight(packed, shape), w)


def test_alias_import_path(monkeypatch):
    import sys

    from conftest import ROOT

    monkeypatch.syspath_prepend(ROOT)
    # (a test file that ran earlier may have put shells of the reference's modules under these names: import the alias afresh)
    for k in [k for k in sys.modules if k == "aerial_gym" or k.startswith("aerial_gym.")]:
        monkeypatch.delitem(sys.modules, k)
    from aerial_gym.utils.vae.vae_image_encoder import VAEImageEncoder, clean_state_dict

    assert VAEImageEncoder is vie.VAEImageEncoder and clean_state_dict is vie.clean_state_dict
    for method in ("encode", "forward", "decode", "get_latent_dims_size"):
        assert callable(getattr(VAEImageEncoder, method))


def test_the_encoder_is_part_of_the_built_library():
    from aerial_gym_simulator_amd import _build, _lib

    assert "agx_vae.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "agx_vae.hip"))
    _build.build_library()
    assert _build.binary_is_current()
    lib = _lib.load()
    for name in ("agx_vae_create", "agx_vae_destroy", "agx_vae_encode", "agx_vae_workspace_bytes", "agx_vae_conv2d", "agx_vae_linear",
                 "agx_vae_sample", "agx_vae_noise", "agx_vae_place_latents"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION >= 22 and _lib.MATH_EXPM1 == 5


def test_config_names_the_upstream_weight_file_and_keeps_the_encoder_off():
    from aerial_gym_simulator_amd.config.task_config import navigation_task_config as cfg

    vc = cfg.vae_config
    assert vc.use_vae is False and vc.latent_dims == 64 and vc.image_res == (270, 480) and vc.interpolation_mode == "nearest"
    assert vc.model_file == "ICRA_test_set_more_sim_data_kld_beta_3_LD_64_epoch_49.pth"
    assert os.path.normpath(vc.model_folder).endswith(os.path.join("aerial_gym_simulator_amd", "utils", "vae", "weights"))
    assert not os.path.exists(os.path.join(vc.model_folder, vc.model_file))  # the file itself is not shipped


def test_expm1_restatement_has_no_cancellation_near_zero():
    """the k = 0 branch of expm1_cw returns r + r^2 p(r): check the polynomial here in float64 against libm"""
    coeffs = [float.fromhex(c) for c in ("0x1.288088c0e67a5p-22", "0x1.72c79824255e0p-19", "0x1.a019c971b4d98p-16", "0x1.a019ad55d1aa7p-13",
                                         "0x1.6c16c1739a511p-10", "0x1.1111111c5719ap-7", "0x1.5555555554ca7p-5", "0x1.5555555553b48p-3", "0x1p-1")]
    r = np.concatenate([-np.logspace(-30, np.log10(0.3465), 4000), np.logspace(-30, np.log10(0.3465), 4000)])
    p = np.full_like(r, coeffs[0])
    for c in coeffs[1:]:
        p = p * r + c
    q = r + r * r * p
    # A float64 value with relative error e rounds to another float32 than the exact one for about 2 e / 2^-24 of all arguments.
    # The GPU test asks for the nearest float on more than 99.999 % of its sweep: e < 1e-5 * 2^-25 = 3e-13 keeps that with room;
    # a cancelling form (exp(r) - 1) would sit at 1e-16 / |r|, i.e. above it for every |r| < 3e-4.
    err = np.max(np.abs(q - np.expm1(r)) / np.abs(np.expm1(r)))
    print("max relative error of r + r^2 p(r) vs expm1:", err)
    assert err < 1e-5 * 2.0 ** -25
