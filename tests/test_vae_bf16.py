"""CPU: the host side of the VAE encoder's bf16 path (csrc/agx_vae_bf16.hip): the weight packing (k order, round to nearest even,
the dense0 column permutation, the zero tail) against a numpy restatement, every refusal of the single-layer entry points before
any device call, the new symbols in header, ctypes table and library, and the kernel's code object."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import vae_bf16_ref as bref
import vae_ref
from conftest import ROOT

import codeobj
from aerial_gym_simulator_amd import _build, _lib
from aerial_gym_simulator_amd.utils.vae import vae_image_encoder as vie

NEW_SYMBOLS = ("agx_vae_packed_bf16_elems", "agx_vae_pack_weight_bf16", "agx_vae_unpack_weight_bf16", "agx_vae_conv2d_bf16",
               "agx_vae_linear_bf16", "agx_vae_create_precision", "agx_vae_precision")


def _gen(seed=5):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------- pack and unpack
@pytest.mark.parametrize("name", list(vae_ref.ORDER))
def test_pack_is_the_numpy_restatement_and_unpack_returns_the_rounded_weights(name):
    shape = bref.PACK_SHAPE[name]
    w = ((torch.rand(shape, generator=_gen(3)) * 2 - 1) * 3).numpy()
    packed = vie.pack_weight_bf16(w)
    k = vae_ref.fan_in(name)
    kp = (k + 15) // 16 * 16
    assert packed.dtype == np.uint16 and packed.shape == (shape[0] * kp,)
    assert np.array_equal(packed, bref.pack_ref(w))
    p2 = packed.reshape(shape[0], kp)
    assert not p2[:, k:].any()  # the zero tail (conv0: 25 -> 32; every other K is a multiple of 16)
    assert (kp > k) == (name == "conv0")
    back = vie.unpack_weight_bf16(packed, shape)
    assert np.array_equal(back.view(np.uint32), torch.from_numpy(w).bfloat16().float().numpy().view(np.uint32))


def test_dense0_columns_go_from_torchs_chw_to_the_stored_hwc_order():
    w = torch.arange(512 * 2304, dtype=torch.float32).reshape(512, 2304) % 251  # small integers: bf16 numbers, the column readable
    packed = bref.widen(vie.pack_weight_bf16(w.reshape(512, 128, 3, 6).numpy())).reshape(512, 2304)
    # stored column (h, w, c) holds torch's column (c, h, w): the flattened [3][6][128] activation meets its own weight
    for h, ww, c in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (2, 5, 127), (1, 3, 77)):
        assert np.array_equal(packed[:, (h * 6 + ww) * 128 + c], w[:, (c * 3 + h) * 6 + ww].numpy()), (h, ww, c)
    x = vae_ref.exact_grid((2, 128, 3, 6), 1 / 16, _gen(8))
    flat_hwc = x.permute(0, 2, 3, 1).reshape(2, 2304)
    assert torch.equal(flat_hwc.double() @ torch.from_numpy(packed).double().T, x.flatten(1).double() @ w.double().T)
    # a plain [out, in] weight (dense1) keeps its column order
    w1 = torch.rand((128, 512), generator=_gen(9)).numpy()
    assert np.array_equal(vie.pack_weight_bf16(w1).reshape(128, 512), bref.rne_bits(w1))


def test_rounding_is_to_nearest_with_ties_to_even():
    one = np.float32(1.0).view(np.uint32)
    cases = {
        one + 0x8000: 0x3F80,          # exactly between 1 and 1 + 2^-7: the even one below
        one + 0x18000: 0x3F82,         # exactly between 1 + 2^-7 and 1 + 2^-6: the even one above
        one + 0x8001: 0x3F81,          # just above the tie
        one + 0x7FFF: 0x3F80,          # just below it
        one + 0x17FFF: 0x3F81,
        0xBF800000 + 0x8000: 0xBF80,   # the same ties, negative
        0xBF800000 + 0x18000: 0xBF82,
        0x3FFF8000: 0x4000,            # a tie that carries into the exponent: 1.99609375 + half an ulp -> 2
        0x7F7FFFFF: 0x7F80,            # the largest float rounds to infinity, as IEEE rounding does
        0x00000000: 0x0000, 0x80000000: 0x8000, 0x7F800000: 0x7F80,
    }
    bits = np.array(list(cases), np.uint32)
    w = np.zeros((32, 16), np.float32)
    w.reshape(-1)[:len(bits)] = bits.view(np.float32)
    packed = vie.pack_weight_bf16(w)
    assert [int(v) for v in packed[:len(bits)]] == list(cases.values())
    assert np.array_equal(packed, bref.rne_bits(w).reshape(-1))
    assert np.array_equal(packed, torch.from_numpy(w).bfloat16().view(torch.int16).numpy().view(np.uint16).reshape(-1))  # torch's own rounding
    nan = vie.pack_weight_bf16(np.full((32, 16), np.nan, np.float32))
    assert np.isnan(bref.widen(nan)).all()


def test_pack_refuses_bad_arguments():
    lib = _lib.load()
    S = _lib.AgxVaeConv(cin=0, cout=32, kh=1, kw=1)
    assert lib.agx_vae_packed_bf16_elems(C.byref(S)) == 0 and lib.agx_vae_packed_bf16_elems(None) == 0
    buf = np.zeros(64, np.float32)
    assert lib.agx_vae_pack_weight_bf16(C.byref(S), buf.ctypes.data, buf.ctypes.data) == -1 and b"agx_vae_pack_weight_bf16" in lib.agx_last_error()
    S.cin = 8
    assert lib.agx_vae_pack_weight_bf16(C.byref(S), None, buf.ctypes.data) == -1
    assert lib.agx_vae_unpack_weight_bf16(C.byref(S), buf.ctypes.data, None) == -1 and b"agx_vae_unpack_weight_bf16" in lib.agx_last_error()


# ------------------------------------------------------------------------------------------------------------- refusals
A = 0x10000  # a 16-byte aligned address that is never dereferenced: every call below is refused before any device call


def _shape(**kw):
    d = dict(cin=32, cout=32, kh=3, kw=3, stride=1, pad_h=1, pad_w=1, in_h=8, in_w=8, out_h=8, out_w=8, src_h=8, src_w=8)
    d.update(kw)
    return _lib.AgxVaeConv(**d)


def _conv(x=A, w=A, bias=A, add=None, y=A, shape="default", flags=0, row_map=None, col_map=None):
    S = _shape() if shape == "default" else shape
    lib = _lib.load()
    code = lib.agx_vae_conv2d_bf16(2, x, w, bias, add, y, C.byref(S) if S is not None else None, flags, row_map, col_map, None)
    return code, lib.agx_last_error().decode()


IMAGE = dict(cin=1, kh=5, kw=5, stride=2, pad_h=2, pad_w=2, out_h=4, out_w=4)
REFUSALS = {
    "null x": (dict(x=None), "null buffer"),
    "null w_packed": (dict(w=None), "null buffer"),
    "null bias": (dict(bias=None), "null buffer"),
    "null y": (dict(y=None), "null buffer"),
    "null shape": (dict(shape=None), "null buffer"),
    "cout 48": (dict(shape=_shape(cout=48)), "cout = 48"),
    "cin 12 without the image flag": (dict(shape=_shape(cin=12)), "cin = 12"),
    "cin 1 without the image flag": (dict(shape=_shape(**IMAGE)), "cin = 1"),
    "image flag with cin 32": (dict(flags=_lib.VAE_IN_IMAGE_F32), "cin = 32"),
    "index tables without the image flag": (dict(row_map=A, col_map=A), "row_map"),
    "one index table": (dict(shape=_shape(**IMAGE), flags=_lib.VAE_IN_IMAGE_F32, row_map=A), "row_map and col_map"),
    "misaligned x": (dict(x=A + 8), "x must be 16-byte aligned"),
    "misaligned image x": (dict(x=A + 2, shape=_shape(**IMAGE), flags=_lib.VAE_IN_IMAGE_F32), "x must be 4-byte aligned"),
    "misaligned w_packed": (dict(w=A + 2), "w_packed must be 16-byte aligned"),
    "misaligned add": (dict(add=A + 4), "add must be 16-byte aligned"),
    "misaligned y": (dict(y=A + 8), "y must be 16-byte aligned"),
    "unknown flag bit": (dict(flags=8), "flags = 8"),
    "unknown flag bits": (dict(flags=_lib.VAE_ELU | 64), "flags = 65"),
    "wrong output size": (dict(shape=_shape(out_h=7)), "out 7 x 8"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_single_layer_entries_refuse_before_any_device_call(case):
    kw, message = REFUSALS[case]
    code, text = _conv(**kw)
    assert code == -1 and text.startswith("agx_vae_conv2d_bf16:") and message in text, (case, code, text)


def test_linear_refusals():
    lib = _lib.load()
    call = lambda fin, fout, flags=0, x=A, y=A: (lib.agx_vae_linear_bf16(3, x, A, A, y, fin, fout, flags, None), lib.agx_last_error().decode())  # noqa: E731
    for args, message in (((12, 32), "cin = 12"), ((16, 40), "cout = 40"), ((16, 32, 16), "flags = 16"), ((16, 32, 0, A + 4), "x must be"),
                          ((16, 32, _lib.VAE_OUT_F32, A, A + 8), "y must be"), ((16, 32, 0, None), "null buffer")):
        code, text = call(*args)
        assert code == -1 and message in text, (args, text)
    code, text = call(16, 32, _lib.VAE_IN_IMAGE_F32)
    assert code == -1 and text.startswith("agx_vae_linear_bf16:") and "AGX_VAE_IN_IMAGE_F32" in text


def test_create_refuses_an_unknown_precision_before_it_touches_the_device():
    lib = _lib.load()
    weights, biases = vie.select_encoder_tensors(vae_ref.random_state_dict(_gen()))
    wp = (C.c_void_p * 11)(*[w.data_ptr() for w in weights])
    bp = (C.c_void_p * 11)(*[b.data_ptr() for b in biases])
    handle = C.c_void_p()
    assert lib.agx_vae_create_precision(wp, bp, 270, 480, 64, 2, C.byref(handle)) == -1 and b"precision = 2" in lib.agx_last_error()
    assert lib.agx_vae_create_precision(wp, bp, 270, 480, 32, _lib.VAE_BF16, C.byref(handle)) == -1 and b"latent_dims" in lib.agx_last_error()
    assert lib.agx_vae_create_precision(wp, bp, 64, 48, 64, _lib.VAE_BF16, C.byref(handle)) == -1 and b"3 x 6" in lib.agx_last_error()
    assert not handle.value and lib.agx_vae_precision(None) == -1


def test_encoder_class_refuses_an_unknown_precision_and_the_config_defaults_to_fp32(tmp_path):
    import types

    from aerial_gym_simulator_amd.config.task_config import navigation_task_config as cfg

    assert cfg.vae_config.precision == "fp32" and set(vie.PRECISIONS) == {"fp32", "bf16"}
    config = types.SimpleNamespace(latent_dims=64, model_folder=str(tmp_path), model_file="none.pth", image_res=(270, 480),
                                   interpolation_mode="nearest", return_sampled_latent=True, precision="fp16")
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):  # (before the weight file is looked for)
        vie.VAEImageEncoder(config, device="cpu")


# -------------------------------------------------------------------------------------------------------------- symbols
def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "aerial_gym_hip.h")).read()
    _build.build_library()
    assert "agx_vae_bf16.hip" in _build.SOURCES and _build.binary_is_current()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 25 == lib.agx_abi_version() and "#define AGX_ABI_VERSION 25" in header
    enum = lambda name: int(re.search(r"\b%s = (\d+)" % name, header).group(1))  # noqa: E731
    assert (enum("AGX_VAE_FP32"), enum("AGX_VAE_BF16")) == (_lib.VAE_FP32, _lib.VAE_BF16) == (0, 1)
    assert (enum("AGX_VAE_ELU"), enum("AGX_VAE_OUT_F32"), enum("AGX_VAE_IN_IMAGE_F32")) == (_lib.VAE_ELU, _lib.VAE_OUT_F32, _lib.VAE_IN_IMAGE_F32) == (1, 2, 4)


# ---------------------------------------------------------------------------------------------------------- code object
@pytest.mark.skipif(not codeobj.tools_available(), reason="objcopy / ROCm LLVM tools not found")
def test_the_bf16_kernel_has_no_scratch_and_issues_the_bf16_matrix_instruction():
    _build.build_library()
    obj = os.path.join(_build.LIB_DIR, "agx_vae_bf16.o")
    meta = {n: r for n, r in codeobj.kernel_metadata(obj).items() if "k_vae_conv_bf16<" in n}
    assert len(meta) == 9  # channel tiles {1, 2, 4} x {NHWC cin % 16, NHWC cin % 8, fp32 image}
    for name, r in meta.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0 and r["vgpr_count"] <= 256, (name, r)
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "vae.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([os.path.join(codeobj.LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        f"--targets={codeobj.TARGET}", f"--output={co}"], check=True)
        asm = subprocess.run([os.path.join(codeobj.LLVM_BIN, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    per_kernel, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
        elif cur and "k_vae_conv_bf16" in cur:
            rec = per_kernel.setdefault(cur, {"mfma": 0, "scratch": 0})
            rec["mfma"] += "v_mfma_f32_32x32x16_bf16" in line
            rec["scratch"] += "scratch_" in line
    assert len(per_kernel) == 9 and all(r["mfma"] >= 1 and r["scratch"] == 0 for r in per_kernel.values()), per_kernel
