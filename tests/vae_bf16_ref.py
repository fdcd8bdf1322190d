"""Test helper: the bf16 path of the VAE encoder on top of vae_ref.py -- bf16 rounding and the weight packing restated in numpy,
the [B, H, W, C] layout, and the bounds the bf16 kernels are held to.  Nothing here touches a GPU or reads a file."""
import numpy as np
import torch
import vae_ref

# the shape each layer's weight is packed under: torch's, but dense0 as [512, 128, 3, 6] (it reads conv3_0's [3, 6, 128] output flattened)
PACK_SHAPE = {name: vae_ref.weight_shape(name) for name in vae_ref.ORDER}
PACK_SHAPE["dense0"] = (512, 128, 3, 6)


def rne_bits(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even, in integer arithmetic (finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(t):
    """a float32 tensor rounded to the nearest bf16 number, as float32"""
    return t.float().bfloat16().float()


def pack_ref(w):
    """[Cout, Cin, kh, kw] (or [out, in]) -> [Cout][Kp] bf16 bits: k = (kh, kw, ci) with ci fastest, Kp = K up to 16, zero tail"""
    w = np.asarray(w, np.float32)
    if w.ndim == 2:
        w = w[:, :, None, None]
    cout, k = w.shape[0], int(np.prod(w.shape[1:]))
    kp = (k + 15) // 16 * 16
    out = np.zeros((cout, kp), np.uint16)
    out[:, :k] = rne_bits(np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(cout, k))
    return out.reshape(-1)


def to_nhwc(x):
    """[B, C, H, W] float32 of bf16 numbers -> [B, H, W, C] torch.bfloat16, contiguous (the conversion must be exact)"""
    y = x.permute(0, 2, 3, 1).contiguous().bfloat16()
    assert torch.equal(y.float(), x.permute(0, 2, 3, 1)), "not bf16 numbers"
    return y


def from_nhwc(y):
    """[B, H, W, C] (bf16 or float32) -> [B, C, H, W] float32"""
    return y.float().permute(0, 3, 1, 2).contiguous()


def bound_f32(name, mag, ref64, elu):
    """fp32 output: twice vae_ref.bound.  That bound assumes every partial sum is rounded to nearest (error <= u per addition); a
    matrix instruction that truncates its internal sums errs at most 2 u per addition."""
    return 2.0 * vae_ref.bound(name, mag, ref64, elu)


def bound_bf16(name, mag, ref64, elu):
    """bf16 output: the fp32 value v that was rounded satisfies |v - ref| <= B (bound_f32), and the round to nearest adds at most
    half a bf16 ulp of v: 2^-8 |v| <= 2^-8 (|ref| + B)"""
    b = bound_f32(name, mag, ref64, elu)
    return b + 2.0 ** -8 * (ref64.abs() + b)
